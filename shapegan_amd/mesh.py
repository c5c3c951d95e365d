"""Batched marching cubes and surface sampling (csrc/mesh.hip; CPU tensors run on the C++ twin).

Replaces skimage.measure.marching_cubes_lewiner + trimesh of model/sdf_net.py:97-116 and metrics.py:31-46.  Neither library is
needed: `Mesh` carries the trimesh attribute names the reference's callers use (vertices, faces, vertex_normals, area,
area_faces, sample), and `Mesh.to_trimesh()` converts when trimesh happens to be installed.

    batch = marching_cubes(grids, level=0.0, spacing=(h, h, h), origin=(-1, -1, -1))     # grids [S,R0,R1,R2] or [R0,R1,R2]
    batch.mesh(0)                  # Mesh (numpy) of shape 0
    batch.sample_surface(2048)     # [S, 2048, 3] on the grids' device

Coordinates: position = (padded index + t) * spacing + origin, where with pad=True the padded index 0 is the virtual shell of
pad_value around each grid (the reference's np.pad(voxels, 1, constant_values=1)).  Conventions of the output (welding, order,
orientation): include/shapegan_hip.h, K12.

Host synchronisation: marching_cubes reads the two totals back from the device ONCE per call (per chunk of a batch that exceeds
the int32 limits) between the counting and the emitting launches, to size its outputs.  Meshing is therefore not meant for graph
capture.  Sampling does not synchronise.
"""
import os

import numpy as np
import torch

from . import lib as L
from .lib import check, f32c, ptr, stream

_INDEX_LIMIT = 2147483647 // 24      # S * P0 * P1 * P2 per call (include/shapegan_hip.h, K12)


def _triple(x):
    if np.isscalar(x):
        return (float(x),) * 3
    x = tuple(float(v) for v in x)
    if len(x) != 3:
        raise ValueError("expected a scalar or three values, got %r" % (x,))
    return x


def max_shapes_per_call(shape, pad=True):
    """Largest number of grids of `shape` (R0, R1, R2) that one meshing call takes (int32 indices inside the kernels)."""
    p = int(bool(pad))
    cells = (shape[0] + 2 * p) * (shape[1] + 2 * p) * (shape[2] + 2 * p)
    return _INDEX_LIMIT // cells


class Mesh(object):
    """One triangle mesh in numpy: vertices [V,3] float32, faces [F,3] int64, vertex_normals [V,3] float32."""

    def __init__(self, vertices, faces, vertex_normals=None):
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float32)
        self.faces = np.ascontiguousarray(faces, dtype=np.int64)
        self.vertex_normals = None if vertex_normals is None else np.ascontiguousarray(vertex_normals, dtype=np.float32)

    @property
    def area_faces(self):
        tri = self.vertices[self.faces].astype(np.float64)
        return np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) / 2

    @property
    def area(self):
        return float(self.area_faces.sum())

    @property
    def face_normals(self):
        tri = self.vertices[self.faces].astype(np.float64)
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-300)

    def sample(self, count, generator=None):
        """`count` points uniformly distributed over the surface (trimesh.Trimesh.sample), numpy [count, 3]: uniforms from
        torch.rand with `generator` (the default CPU generator when None), sampled by the C++ twin."""
        v = torch.from_numpy(self.vertices)
        f = torch.from_numpy(self.faces)
        vo = torch.tensor([0, v.shape[0]], dtype=torch.int64)
        to = torch.tensor([0, f.shape[0]], dtype=torch.int64)
        u = torch.rand((1, int(count), 3), generator=generator)
        return sample_packed(v, f, vo, to, u)[0][0].numpy()

    def apply_transform(self, matrix):
        """trimesh.Trimesh.apply_transform: vertices through the homogeneous 4x4 `matrix`; the normals through its 3x3 part, made
        unit length again; the winding reversed when that part mirrors.  In place; returns self."""
        m = np.asarray(matrix, dtype=np.float64)
        if m.shape != (4, 4):
            raise ValueError("apply_transform: expected a 4x4 matrix, got %s" % (m.shape,))
        v = self.vertices.astype(np.float64) @ m[:3, :3].T + m[:3, 3]
        self.vertices = np.ascontiguousarray(v, dtype=np.float32)
        if self.vertex_normals is not None:
            n = self.vertex_normals.astype(np.float64) @ m[:3, :3].T
            length = np.linalg.norm(n, axis=1, keepdims=True)
            self.vertex_normals = np.ascontiguousarray(np.divide(n, length, out=np.zeros_like(n), where=length > 0), dtype=np.float32)
        if np.linalg.det(m[:3, :3]) < 0:
            self.faces = np.ascontiguousarray(self.faces[:, ::-1])
        return self

    def apply_translation(self, translation):
        """trimesh.Trimesh.apply_translation: vertices += translation [3].  In place; returns self."""
        t = np.asarray(translation, dtype=np.float64).reshape(3)
        self.vertices = np.ascontiguousarray(self.vertices.astype(np.float64) + t, dtype=np.float32)
        return self

    def export(self, path):
        """Writes the mesh by the extension of `path`: .obj (text; v, vn and f a//a lines, 9 significant digits, so float32 reads
        back exactly), .stl (binary: per triangle its face normal and its three corners, unwelded) or .ply (binary little endian:
        x y z [nx ny nz] per vertex, one uchar-counted int32 index list per face)."""
        ext = os.path.splitext(str(path))[1].lower()
        v, f, n = self.vertices, self.faces, self.vertex_normals
        if ext == ".obj":
            with open(path, "w") as fh:
                fh.writelines("v %.9g %.9g %.9g\n" % tuple(r) for r in v.tolist())
                if n is not None:
                    fh.writelines("vn %.9g %.9g %.9g\n" % tuple(r) for r in n.tolist())
                pattern = "f %d//%d %d//%d %d//%d\n" if n is not None else "f %d %d %d\n"
                rep = 2 if n is not None else 1
                fh.writelines(pattern % tuple(np.repeat(r, rep)) for r in (f + 1).tolist())
        elif ext == ".stl":
            rec = np.zeros(f.shape[0], dtype=[("normal", "<f4", 3), ("corners", "<f4", (3, 3)), ("attr", "<u2")])
            rec["normal"] = self.face_normals.astype(np.float32) if f.shape[0] else 0
            rec["corners"] = v[f]
            with open(path, "wb") as fh:
                fh.write(b"shapegan_amd binary STL".ljust(80, b" "))
                fh.write(np.uint32(f.shape[0]).tobytes())
                fh.write(rec.tobytes())
        elif ext == ".ply":
            props = "".join("property float %s\n" % c for c in (("x", "y", "z") + (("nx", "ny", "nz") if n is not None else ())))
            head = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%selement face %d\n"
                    "property list uchar int vertex_indices\nend_header\n" % (v.shape[0], props, f.shape[0]))
            vert = v if n is None else np.concatenate([v, n], axis=1)
            rec = np.zeros(f.shape[0], dtype=[("count", "u1"), ("index", "<i4", 3)])
            rec["count"] = 3
            rec["index"] = f
            with open(path, "wb") as fh:
                fh.write(head.encode("ascii"))
                fh.write(np.ascontiguousarray(vert, dtype="<f4").tobytes())
                fh.write(rec.tobytes())
        else:
            raise ValueError("export: unknown mesh format %r (.obj, .stl and .ply are written)" % ext)
        return path

    # ---- topology: the trimesh names, computed by the C++ twin (shapegan_amd.topology) ------------------------------------------------
    def _components(self):
        from . import topology
        normals = self.vertex_normals if self.vertex_normals is not None else np.zeros_like(self.vertices)
        batch = MeshBatch(torch.from_numpy(self.vertices), torch.from_numpy(normals), torch.from_numpy(self.faces),
                          torch.tensor([0, self.vertices.shape[0]], dtype=torch.int64),
                          torch.tensor([0, self.faces.shape[0]], dtype=torch.int64))
        return batch, topology.components(batch)

    def split(self):
        """trimesh.Trimesh.split: the connected components as a list of Mesh, in the order of their lowest vertex index."""
        from . import topology
        batch, comps = self._components()
        out = []
        for c in range(len(comps)):
            mask = torch.zeros(len(comps), dtype=torch.bool)
            mask[c] = True
            piece = topology.keep_components(batch, comps, mask).mesh(0)
            if self.vertex_normals is None:
                piece.vertex_normals = None
            out.append(piece)
        return out

    @property
    def body_count(self):
        return len(self._components()[1])

    @property
    def is_watertight(self):
        """Every edge is shared by exactly two triangles that run along it in opposite directions (and there is a triangle)."""
        comps = self._components()[1]
        return bool(len(comps) > 0 and comps.watertight.all())

    @property
    def volume(self):
        """The signed volume enclosed: positive for outward-facing closed surfaces."""
        return float(self._components()[1].volume.sum())

    @property
    def euler_number(self):
        """Referenced vertices - distinct edges + triangles."""
        return int(self._components()[1].euler.sum())

    def simplify(self, **options):
        """The mesh simplified by quadric vertex clustering on the C++ twin: shapegan_amd.simplify.simplify_meshes of a batch of one
        (cell= / cells= / target_triangles=, placement=).  A mesh without vertex normals comes back without them."""
        from . import simplify
        normals = self.vertex_normals if self.vertex_normals is not None else np.zeros_like(self.vertices)
        batch = MeshBatch(torch.from_numpy(self.vertices), torch.from_numpy(normals), torch.from_numpy(self.faces),
                          torch.tensor([0, self.vertices.shape[0]], dtype=torch.int64),
                          torch.tensor([0, self.faces.shape[0]], dtype=torch.int64))
        out = simplify.simplify_meshes(batch, **options)[0].mesh(0)
        if self.vertex_normals is None:
            out.vertex_normals = None
        return out

    def to_trimesh(self):
        import trimesh
        return trimesh.Trimesh(vertices=self.vertices, faces=self.faces, vertex_normals=self.vertex_normals, process=False)


class MeshBatch(object):
    """S meshes packed on one device: vertices / normals [V,3] float32, faces [F,3] int64 (local to each shape), vert_offsets /
    tri_offsets [S+1] int64 (shape s: vertices [vert_offsets[s], vert_offsets[s+1]), triangles likewise)."""

    def __init__(self, vertices, normals, faces, vert_offsets, tri_offsets):
        self.vertices, self.normals, self.faces = vertices, normals, faces
        self.vert_offsets, self.tri_offsets = vert_offsets, tri_offsets
        self._host_offsets = None

    def __len__(self):
        return self.vert_offsets.shape[0] - 1

    def _offsets(self):
        if self._host_offsets is None:
            self._host_offsets = (self.vert_offsets.cpu().numpy(), self.tri_offsets.cpu().numpy())
        return self._host_offsets

    def triangle_counts(self):
        return self.tri_offsets[1:] - self.tri_offsets[:-1]

    def mesh(self, i):
        vo, to = self._offsets()
        return Mesh(self.vertices[vo[i]:vo[i + 1]].cpu().numpy(), self.faces[to[i]:to[i + 1]].cpu().numpy(),
                    self.normals[vo[i]:vo[i + 1]].cpu().numpy())

    def meshes(self):
        v, n, f = self.vertices.cpu().numpy(), self.normals.cpu().numpy(), self.faces.cpu().numpy()
        vo, to = self._offsets()
        return [Mesh(v[vo[i]:vo[i + 1]], f[to[i]:to[i + 1]], n[vo[i]:vo[i + 1]]) for i in range(len(self))]

    def components(self):
        """shapegan_amd.topology.components of this batch."""
        from . import topology
        return topology.components(self)

    def clean(self, rule=True):
        """The MeshBatch of the components `rule` keeps (shapegan_amd.topology.clean_meshes)."""
        from . import topology
        return topology.clean_meshes(self, rule)[0]

    def simplify(self, **options):
        """The MeshBatch simplified by quadric vertex clustering (shapegan_amd.simplify.simplify_meshes: cell= / cells= /
        target_triangles=, placement=)."""
        from . import simplify
        return simplify.simplify_meshes(self, **options)[0]

    def sample_surface(self, count, generator=None, return_empty=False):
        """[S, count, 3] points on the device of the meshes, area-weighted; uniforms [S, count, 3] from torch.rand with
        `generator` (made on the generator's device, then moved).  Rows of a shape without triangles are zeros; with
        return_empty also the int32 flags [S] (1: no triangles)."""
        dev = self.vertices.device
        gdev = generator.device if generator is not None else dev
        u = torch.rand((len(self), int(count), 3), generator=generator, device=gdev).to(dev)
        out, empty = sample_packed(self.vertices, self.faces, self.vert_offsets, self.tri_offsets, u)
        return (out, empty) if return_empty else out


def sample_packed(vertices, faces, vert_offsets, tri_offsets, uniforms):
    """sg_mesh_sample on packed meshes: uniforms [S, P, 3] -> (points [S, P, 3], empty [S] int32)."""
    S, P = uniforms.shape[0], uniforms.shape[1]
    dev = uniforms.device
    F = faces.shape[0]
    vertices, faces, uniforms = f32c(vertices), faces.contiguous(), f32c(uniforms)
    out = torch.empty((S, P, 3), dtype=torch.float32, device=dev)
    empty = torch.empty(S, dtype=torch.int32, device=dev)
    lib = L.load()
    ws = L.workspace("mesh_sample", lib.sg_mesh_sample_workspace_bytes(S, F), dev)
    try:
        check(lib.sg_mesh_sample(ptr(vertices), ptr(faces), ptr(vert_offsets), ptr(tri_offsets), S, F,
                                 ptr(uniforms), P, ptr(out), ptr(empty), ptr(ws), ws.numel(), stream()), "mesh_sample")
    finally:
        L.reset_call_state()
    return out, empty


def _mc_chunk(grids, level, spacing, origin, pad, pad_value):
    S, R0, R1, R2 = grids.shape
    dev = grids.device
    lib = L.load()
    nbytes = lib.sg_mc_workspace_bytes(S, R0, R1, R2, int(pad))
    if nbytes == 0:
        raise RuntimeError("marching_cubes: %d grids of %s exceed the int32 index limits of one call" % (S, (R0, R1, R2)))
    ws = L.workspace("mc", nbytes, dev)
    vo = torch.empty(S + 1, dtype=torch.int64, device=dev)
    to = torch.empty(S + 1, dtype=torch.int64, device=dev)
    try:
        check(lib.sg_mc_count(ptr(grids), S, R0, R1, R2, level, int(pad), pad_value, ptr(vo), ptr(to), ptr(ws), ws.numel(),
                              stream()), "mc_count")
    finally:
        L.reset_call_state()
    # the one device -> host read of a meshing call: the totals size the outputs
    V, F = (int(x) for x in torch.stack([vo[S], to[S]]).cpu())
    verts = torch.empty((V, 3), dtype=torch.float32, device=dev)
    norms = torch.empty((V, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((F, 3), dtype=torch.int64, device=dev)
    try:
        check(lib.sg_mc_emit(ptr(grids), S, R0, R1, R2, level, int(pad), pad_value, *spacing, *origin, ptr(vo), ptr(to),
                             ptr(verts), ptr(norms), ptr(faces), V, F, ptr(ws), ws.numel(), stream()), "mc_emit")
    finally:
        L.reset_call_state()
    return verts, norms, faces, vo, to


def marching_cubes(grids, level=0.0, spacing=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), pad=True, pad_value=1.0, upscale=None,
                   redistance=False):
    """Meshes one grid [R0,R1,R2] or a batch [S,R0,R1,R2] (torch tensor or numpy array; CPU tensors run on the twin) at `level`
    and returns a MeshBatch on the grids' device.  Batches beyond the int32 limits of one call are split.
    upscale: a zoom factor (4: create_plot.py:826-828).  Every grid is zoomed by the cubic B-spline of shapegan_amd.voxelzoom before
    it is meshed, the pad goes around the zoomed grid, and spacing and origin are adjusted so that the first and the last sample of
    every axis stay where they were: the mesh stays in the same box.  None: the grids are meshed as they are.
    redistance: True, or the world distance one grid unit stands for (True: 0.1, the grids of datasets.py:7-40).  Every grid is first
    redistanced about its zero level (shapegan_amd.voxeldist.redistance_grids with this call's spacing; the values next to the
    surface are kept) and divided by that scale again, so it stays in grid units and holds distances beyond its truncation: a `level`
    outside [-1, 1] is then an offset surface (choose pad_value beyond it).  It comes before upscale.  False: the call as it was."""
    if isinstance(grids, np.ndarray):
        grids = torch.from_numpy(grids)
    if grids.dim() == 3:
        grids = grids.unsqueeze(0)
    if grids.dim() != 4:
        raise ValueError("marching_cubes: expected [R0,R1,R2] or [S,R0,R1,R2], got %s" % (tuple(grids.shape),))
    grids = f32c(grids)
    spacing, origin = _triple(spacing), _triple(origin)
    level, pad_value = float(level), float(pad_value)
    S = grids.shape[0]
    shape = tuple(grids.shape[1:])
    coarse_spacing = spacing
    if upscale is not None:
        from . import voxelzoom
        fine = voxelzoom.zoom_size(shape, upscale)
        scale = tuple((n - 1) / (N - 1) if N > 1 else 1.0 for n, N in zip(shape, fine))
        # sample i of the coarse grid sits at (i + pad) * spacing + origin, sample I of the fine one at (I + pad) * spacing' + origin'
        origin = tuple(o + int(bool(pad)) * (s - s * k) for o, s, k in zip(origin, spacing, scale))
        spacing = tuple(s * k for s, k in zip(spacing, scale))
        shape = fine
    per = max_shapes_per_call(shape, pad)
    if per < 1:
        raise RuntimeError("marching_cubes: one grid of %s exceeds the int32 index limits" % (shape,))

    def chunk(s):
        part = grids[s:s + per]
        if redistance:
            from . import voxeldist
            scale = 0.1 if redistance is True else float(redistance)
            part = voxeldist.redistance_grids(part, 0.0, coarse_spacing, scale, True) / scale
        return part if upscale is None else voxelzoom.zoom_grids(part, size=shape)

    parts = [_mc_chunk(chunk(s), level, spacing, origin, pad, pad_value) for s in range(0, S, per)]
    if len(parts) == 1:
        return MeshBatch(*parts[0])
    vo = [parts[0][3]]
    to = [parts[0][4]]
    for p in parts[1:]:
        vo.append(p[3][1:] + vo[-1][-1])
        to.append(p[4][1:] + to[-1][-1])
    return MeshBatch(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), torch.cat([p[2] for p in parts]),
                     torch.cat(vo), torch.cat(to))
