"""Meshes and settings the simplification tests share: hand-built meshes that reach every special case, a tessellated cube whose
corners lie on cell faces, a jittered icosphere, marching-cubes meshes; and the comparison of a package result with another."""
import numpy as np
import torch

from shapegan_amd.mesh import MeshBatch, marching_cubes

TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
TET_F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int64)      # outward


def vertex_normals(verts, faces):
    """Area-weighted vertex normals (float32): coherent, so no cluster's sum cancels."""
    v = verts.astype(np.float64)
    n = np.zeros_like(v)
    fn = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    for k in range(3):
        np.add.at(n, faces[:, k], fn)
    length = np.linalg.norm(n, axis=1, keepdims=True)
    return (n / np.where(length > 0, length, 1)).astype(np.float32)


def hand_meshes():
    """name -> (vertices, faces, normals or None)."""
    nan_v = np.concatenate([TET_V, [[np.nan, 0.5, 0.5]]]).astype(np.float32)
    return {
        "one_triangle": (TET_V[:3].copy(), np.array([[0, 1, 2]], dtype=np.int64), None),
        "tetrahedron": (TET_V.copy(), TET_F.copy(), None),
        # vertices 0 and 1 share a cell at cells = 2 and carry opposite normals: their cluster's normal is zero
        "opposite_normals": (np.array([[0, 0, 0], [0.1, 0.1, 0.1], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32),
                             np.array([[0, 3, 2], [1, 2, 4], [0, 4, 3], [2, 3, 4]], dtype=np.int64),
                             np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)),
        "unreferenced_vertex": (np.concatenate([TET_V[:1] + 0.4, TET_V]), TET_F + 1, None),
        "out_of_range": (TET_V.copy(), np.concatenate([TET_F[:2], np.array([[0, 1, 9], [-1, 2, 3]]), TET_F[2:]]), None),
        "zero_area": (np.concatenate([TET_V, [[0.5, 0.5, 0]]]).astype(np.float32),
                      np.concatenate([TET_F, np.array([[1, 4, 2]])]), None),      # vertex 4 lies on the side 1 - 2
        "nan_coordinate": (nan_v, np.concatenate([TET_F, np.array([[1, 2, 4]])]), None),
        "no_triangles": (TET_V.copy(), np.zeros((0, 3), dtype=np.int64), None),
        "nothing": (np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int64), None),
    }


def pack(meshes, device="cpu"):
    """MeshBatch of a list of (vertices, faces, normals or None: area-weighted vertex normals)."""
    verts = np.concatenate([np.asarray(m[0], dtype=np.float32).reshape(-1, 3) for m in meshes])
    faces = np.concatenate([np.asarray(m[1], dtype=np.int64).reshape(-1, 3) for m in meshes])
    normals = []
    for m in meshes:
        v, f = np.asarray(m[0], dtype=np.float32).reshape(-1, 3), np.asarray(m[1], dtype=np.int64).reshape(-1, 3)
        if len(m) > 2 and m[2] is not None:
            normals.append(np.asarray(m[2], dtype=np.float32))
        else:
            ok = ((f >= 0) & (f < len(v))).all(axis=1) if len(f) else np.zeros(0, dtype=bool)
            normals.append(np.nan_to_num(vertex_normals(np.nan_to_num(v), f[ok])) if len(v) else np.zeros((0, 3), np.float32))
    vo = np.cumsum([0] + [len(np.asarray(m[0]).reshape(-1, 3)) for m in meshes])
    to = np.cumsum([0] + [len(np.asarray(m[1]).reshape(-1, 3)) for m in meshes])
    return MeshBatch(torch.from_numpy(verts).to(device), torch.from_numpy(np.concatenate(normals).reshape(-1, 3)).to(device),
                     torch.from_numpy(faces).to(device), torch.from_numpy(vo).to(device), torch.from_numpy(to).to(device))


HAND_ORDER = ["nothing", "one_triangle", "tetrahedron", "no_triangles", "opposite_normals", "unreferenced_vertex", "nothing",
              "out_of_range", "zero_area", "nan_coordinate", "nothing"]


def hand_batch(device="cpu"):
    """Every hand mesh, with empty shapes first, in the middle and last."""
    h = hand_meshes()
    return pack([h[k] for k in HAND_ORDER], device)


def cube(quads=8):
    """The unit cube [0, 1]^3, every face `quads` x `quads` quads of two triangles, welded, outward: (vertices, faces, normals)."""
    index, verts, faces = {}, [], []

    def vid(p):
        key = tuple(int(round(c * quads)) for c in p)
        if key not in index:
            index[key] = len(verts)
            verts.append([k / quads for k in key])
        return index[key]
    for axis in range(3):
        for side in (0, 1):
            u, w = (axis + 1) % 3, (axis + 2) % 3
            for i in range(quads):
                for j in range(quads):
                    def corner(a, b):
                        p = [0.0, 0.0, 0.0]
                        p[axis], p[u], p[w] = float(side), (i + a) / quads, (j + b) / quads
                        return vid(p)
                    q = [corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)]
                    if side == 0:
                        q = q[::-1]
                    faces += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    v, f = np.array(verts, dtype=np.float32), np.array(faces, dtype=np.int64)
    return v, f, vertex_normals(v, f)


def icosphere(level=4, radius=0.8, jitter=0.01, seed=0):
    """An icosahedron subdivided `level` times (20 * 4^level triangles) on the sphere of `radius`, every radius then scaled by
    1 + jitter * u, u uniform in [-1, 1] (seeded): (vertices, faces, normals = the unit directions)."""
    t = (1 + 5 ** 0.5) / 2
    v = [[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t], [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
         [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, out = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = out
    unit = np.array(v)
    r = radius * (1 + jitter * np.random.RandomState(seed).uniform(-1, 1, size=len(unit)))
    return (unit * r[:, None]).astype(np.float32), np.array(f, dtype=np.int64), unit.astype(np.float32)


def sphere_mesh(R=16, r=0.6, device="cpu"):
    """Marching cubes of test_mesh.sphere_grid: a MeshBatch of one shape."""
    from test_mesh import sphere_grid
    g = torch.from_numpy(sphere_grid(R, r))[None].to(device)
    h = 2.0 / (R - 1)
    return marching_cubes(g, level=0.0, spacing=h, origin=-1.0 - h, pad=True, pad_value=1.0)


def concat(batches):
    """One MeshBatch of several (on one device), shapes in order."""
    vo, to = [batches[0].vert_offsets], [batches[0].tri_offsets]
    for b in batches[1:]:
        vo.append(b.vert_offsets[1:] + vo[-1][-1])
        to.append(b.tri_offsets[1:] + to[-1][-1])
    return MeshBatch(torch.cat([b.vertices for b in batches]), torch.cat([b.normals for b in batches]),
                     torch.cat([b.faces for b in batches]), torch.cat(vo), torch.cat(to))


def shape_of(batch, s):
    """Shape s of a batch as a batch of one."""
    vo, to = batch.vert_offsets.cpu().numpy(), batch.tri_offsets.cpu().numpy()
    dev = batch.vertices.device
    return MeshBatch(batch.vertices[vo[s]:vo[s + 1]].contiguous(), batch.normals[vo[s]:vo[s + 1]].contiguous(),
                     batch.faces[to[s]:to[s + 1]].contiguous(), torch.tensor([0, vo[s + 1] - vo[s]], dtype=torch.int64, device=dev),
                     torch.tensor([0, to[s + 1] - to[s]], dtype=torch.int64, device=dev))


def same_batches(a, b):
    """Bit-identical: offsets, faces, and the bits of vertices and normals."""
    return (torch.equal(a.vert_offsets.cpu(), b.vert_offsets.cpu()) and torch.equal(a.tri_offsets.cpu(), b.tri_offsets.cpu())
            and torch.equal(a.faces.cpu(), b.faces.cpu())
            and torch.equal(a.vertices.cpu().contiguous().view(torch.int32), b.vertices.cpu().contiguous().view(torch.int32))
            and torch.equal(a.normals.cpu().contiguous().view(torch.int32), b.normals.cpu().contiguous().view(torch.int32)))


def to_device(batch, device):
    return MeshBatch(batch.vertices.to(device), batch.normals.to(device), batch.faces.to(device), batch.vert_offsets.to(device),
                     batch.tri_offsets.to(device))


# (name, keyword arguments) of the forms every mesh is run in
FORMS = [("cells", {"cells": 4}), ("cell", {"cell": 0.3, "origin": (-1.05, -1.0, -0.95)}), ("mean", {"cells": 4, "placement": "mean"})]


# ---- the cases both tiers run: name -> (builder of a CPU MeshBatch, keyword arguments) ---------------------------------------------------
def _mixed():
    h = hand_meshes()
    return pack([icosphere(), h["nothing"], cube(), h["tetrahedron"], h["one_triangle"]])


BUILDERS = {"hand": hand_batch, "cube": lambda: pack([cube()]), "icosphere": lambda: pack([icosphere()]),
            "sphere16": sphere_mesh, "mixed": _mixed}
CASES = {}
for _form, _kw in FORMS + [("cells1", {"cells": 1}), ("cells2", {"cells": 2})]:
    CASES["hand-" + _form] = ("hand", _kw)
for _c in (2, 3, 5):
    CASES["cube-%d" % _c] = ("cube", {"cells": _c})
CASES["cube-3-mean"] = ("cube", {"cells": 3, "placement": "mean"})
for _c in (4, 6, 10):
    CASES["icosphere-%d" % _c] = ("icosphere", {"cells": _c})
CASES["icosphere-6-mean"] = ("icosphere", {"cells": 6, "placement": "mean"})
CASES["icosphere-1"] = ("icosphere", {"cells": 1})      # one cluster owns every vertex and every corner record: the long runs
CASES["icosphere-target"] = ("icosphere", {"target_triangles": 500})
CASES["sphere16-cells"] = ("sphere16", {"cells": 8})
CASES["sphere16-cell"] = ("sphere16", {"cell": 0.25})
CASES["mixed-cells"] = ("mixed", {"cells": [6, 3, 3, 4, 2]})
CASES["mixed-target"] = ("mixed", {"target_triangles": [500, 5, 100, 10, 0]})      # the tetrahedron (4 <= 10) comes back unchanged
HAND_CASES = tuple(k for k in CASES if k.startswith("hand"))

_built, _references = {}, {}


def built(name, device="cpu"):
    """The batch of BUILDERS[name], made once per device."""
    key = (name, str(device))
    if key not in _built:
        if str(device) == "cpu":
            _built[key] = BUILDERS[name]()
        else:
            _built[key] = to_device(built(name), device)
    return _built[key]


def reference(case):
    """simplify_reference.simplify of a case, computed once."""
    import simplify_reference as R
    if case not in _references:
        name, kw = CASES[case]
        _references[case] = R.simplify(built(name), **kw)
    return _references[case]


def check_case_against_reference(case, device="cpu"):
    """The package on `device` against the reference: keys, cluster numbers and offsets equal, then simplify_reference.check_against;
    info equal.  Returns (the result, the worst error / tolerance of positions and normals)."""
    import simplify_reference as R
    from shapegan_amd import simplify as SM
    name, kw = CASES[case]
    batch, ref = built(name, device), reference(case)
    got, info = SM.simplify_meshes(batch, **kw)
    assert info["cells"].tolist() == (ref["cells"] if "cell" not in kw else np.full(len(batch), R.MAX_CELLS)).tolist(), "cells"
    assert np.array_equal(info["cell"].numpy().view(np.int32), ref["cell"].view(np.int32)), "cell"
    assert info["triangles_after"].tolist() == np.diff(ref["tri_offsets"]).tolist()
    assert info["triangles_before"].tolist() == np.diff(batch.tri_offsets.cpu().numpy()).tolist()
    # the grid the package settled on, through its own stages: keys and cluster numbers
    p = SM._Packed(batch)
    cells = np.where(ref["unchanged"], 1, ref["cells"]) if "cell" not in kw else np.full(len(batch), R.MAX_CELLS)
    if "cell" in kw:
        grid = SM._Grid(np.tile(np.asarray(kw.get("origin", (-1, -1, -1)), dtype=np.float32), (len(batch), 1)), ref["cell"], cells)
    else:
        lo, hi = (t.cpu().numpy() for t in SM.bounding_boxes(batch))
        grid = SM._box_grid(lo, hi, cells)
    keys, _, _, _, vertex_cluster, co = SM._clusters(p, grid.upload(p.dev))
    assert np.array_equal(keys.cpu().numpy(), ref["keys"]), "keys"
    assert np.array_equal(vertex_cluster.cpu().numpy(), ref["vertex_cluster"]), "cluster numbering"
    assert np.array_equal(co.cpu().numpy(), ref["cluster_offsets"]), "cluster offsets"
    worst = R.check_against(got, ref, left_out=1.0 if name in ("hand", "mixed") else 0.01)
    print("[simplify] %s on %s: worst error / tolerance: positions %.3f, normals %.3f" % (case, device, worst[0], worst[1]))
    return got, worst
