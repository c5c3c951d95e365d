"""Meshes the topology tests share: hand-built ones with known answers, grids whose level sets have known topology, ribbons whose
vertex numbering makes deep union-find trees, and the permutation of a mesh."""
import numpy as np
import torch

from shapegan_amd.mesh import MeshBatch, marching_cubes
from shapegan_amd.util import get_voxel_coordinates

TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
TET_F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int64)      # outward: volume + 1/6


def tet(shift=0.0):
    return TET_V + np.float32(shift), TET_F.copy()


def join(*meshes):
    """One mesh of several: vertices concatenated, faces shifted."""
    verts, faces, base = [], [], 0
    for v, f in meshes:
        verts.append(v)
        faces.append(f + base)
        base += len(v)
    return np.concatenate(verts), np.concatenate(faces)


def hand_meshes():
    """name -> (vertices, faces)."""
    tv, tf = tet()
    shared = (np.concatenate([tv, tet(0.0)[0][1:] * -1]), np.concatenate([tf, np.array([[0, 4, 5], [0, 6, 4], [0, 5, 6], [4, 6, 5]])]))
    flipped = tf.copy()
    flipped[3] = flipped[3][::-1]
    return {
        "two_tetrahedra": join(tet(), tet(3.0)),
        "open_triangle": (tv[:3].copy(), np.array([[0, 1, 2]], dtype=np.int64)),
        "unreferenced_vertex": (np.concatenate([tv[:1] + 9, tv]), tf + 1),
        "shared_vertex": shared,
        "one_flipped": (tv.copy(), flipped),
        "out_of_range": (tv.copy(), np.concatenate([tf[:2], np.array([[0, 1, 9], [-1, 2, 3]]), tf[2:]])),
        "degenerate": join(tet(), (tv[:2] + 5, np.array([[0, 0, 1]], dtype=np.int64))),
        "no_triangles": (tv.copy(), np.zeros((0, 3), dtype=np.int64)),
        "nothing": (np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int64)),
    }


def pack(meshes, device="cpu", seed=0):
    """MeshBatch of a list of (vertices, faces); the normals are seeded noise (the compaction must copy their bits)."""
    verts = np.concatenate([np.asarray(v, dtype=np.float32).reshape(-1, 3) for v, _ in meshes])
    faces = np.concatenate([np.asarray(f, dtype=np.int64).reshape(-1, 3) for _, f in meshes])
    vo = np.cumsum([0] + [len(v) for v, _ in meshes])
    to = np.cumsum([0] + [len(f) for _, f in meshes])
    normals = torch.randn((len(verts), 3), generator=torch.Generator().manual_seed(seed))
    return MeshBatch(torch.from_numpy(verts).to(device), normals.to(device), torch.from_numpy(faces).to(device),
                     torch.from_numpy(vo).to(device), torch.from_numpy(to).to(device))


def hand_batch(device="cpu"):
    """Every hand mesh, with empty shapes first, in the middle and last."""
    h = hand_meshes()
    order = ["nothing", "two_tetrahedra", "open_triangle", "no_triangles", "unreferenced_vertex", "shared_vertex", "nothing",
             "one_flipped", "out_of_range", "degenerate", "nothing"]
    return order, pack([h[k] for k in order], device)


def radius(R):
    return np.linalg.norm(get_voxel_coordinates(R).astype(np.float64), axis=1).reshape(R, R, R)


def two_spheres_grid(R=32):
    p = get_voxel_coordinates(R).astype(np.float64)
    a = np.linalg.norm(p - np.array([0.45, 0, 0]), axis=1) - 0.3
    b = np.linalg.norm(p + np.array([0.45, 0, 0]), axis=1) - 0.25
    return np.minimum(a, b).reshape(R, R, R).astype(np.float32)


def shell_grid(R=32, outer=0.8, inner=0.4):
    """A ball with a spherical void: the outer sphere and, inside it, a cavity."""
    r = radius(R)
    return np.maximum(r - outer, inner - r).astype(np.float32)


def mesh_grids(grids, device="cpu"):
    g = torch.as_tensor(np.asarray(grids), dtype=torch.float32).to(device)
    h = 2.0 / (g.shape[-1] - 1)      # get_voxel_coordinates: index i sits at -1 + i h; the padding adds one layer in front
    return marching_cubes(g, level=0.0, spacing=h, origin=-1.0 - h, pad=True, pad_value=1.0)


def noise_grids(S, R, seed):
    return torch.rand((S, R, R, R), generator=torch.Generator().manual_seed(seed)) * 2 - 1


def ribbon(triangles, seed):
    """A strip of `triangles` triangles (i, i+1, i+2), consistently oriented, its vertices then renumbered by a seeded permutation:
    one open component whose union-find trees grow deep.  (vertices, faces)."""
    n = triangles + 2
    i = np.arange(n)
    verts = np.stack([i * 1e-3, (i % 2).astype(np.float64), np.zeros(n)], axis=1).astype(np.float32)
    t = np.arange(triangles)
    faces = np.stack([t, t + 1, t + 2], axis=1)
    odd = t % 2 == 1
    faces[odd] = faces[odd][:, [1, 0, 2]]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).numpy()      # old index -> new index
    out = np.empty_like(verts)
    out[perm] = verts
    return out, perm[faces].astype(np.int64)


def permuted(batch, seed):
    """A one-shape batch with its vertices renumbered and its triangles shuffled (seeded) -> (batch, perm), perm: old vertex index ->
    new index."""
    assert len(batch) == 1
    g = torch.Generator().manual_seed(seed)
    dev = batch.vertices.device
    V, F = batch.vertices.shape[0], batch.faces.shape[0]
    perm = torch.randperm(V, generator=g).to(dev)
    order = torch.randperm(F, generator=g).to(dev)
    verts, norms = torch.empty_like(batch.vertices), torch.empty_like(batch.normals)
    verts[perm] = batch.vertices
    norms[perm] = batch.normals
    return MeshBatch(verts, norms, perm[batch.faces][order].contiguous(), batch.vert_offsets.clone(), batch.tri_offsets.clone()), perm


def same_batches(a, b):
    return (torch.equal(a.vert_offsets.cpu(), b.vert_offsets.cpu()) and torch.equal(a.tri_offsets.cpu(), b.tri_offsets.cpu())
            and torch.equal(a.faces.cpu(), b.faces.cpu())
            and torch.equal(a.vertices.cpu().view(torch.int32), b.vertices.cpu().view(torch.int32))
            and torch.equal(a.normals.cpu().view(torch.int32), b.normals.cpu().view(torch.int32)))


def equals_reference(batch, arrays):
    """True when a MeshBatch holds exactly the arrays of topology_reference.compact."""
    got = (batch.vertices, batch.normals, batch.faces, batch.vert_offsets, batch.tri_offsets)
    return all(g.shape == tuple(r.shape) and np.array_equal(g.cpu().numpy().view(np.int32 if r.dtype == np.float32 else r.dtype),
                                                           r.view(np.int32 if r.dtype == np.float32 else r.dtype))
               for g, r in zip(got, arrays))
