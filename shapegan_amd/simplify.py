"""Mesh simplification on the device of the meshes (csrc/simplify.hip; CPU tensors run on the C++ twin): vertex clustering on a
uniform grid with quadric placement (Lindstrom 2000, Garland-Heckbert quadrics), one pass over a whole MeshBatch.

What trimesh users take from simplify_*: nothing after marching cubes could make a mesh smaller, and a 256^3 chair has of the order
of a million triangles.

    small, info = simplify_meshes(batch, cells=32)                 # 32 cells along the largest side of each shape's bounding box
    small, info = simplify_meshes(batch, cell=0.05)                # cells of edge 0.05 from a fixed origin: batch-independent
    small, info = simplify_meshes(batch, target_triangles=2000)    # per shape a grid that leaves at most 2000 triangles

The contract (csrc/simplify_core.h): the vertices of a shape that share a grid cell become ONE vertex, placed where the planes of the
triangles around the cell agree best (a regularised 3x3 solve about the cell centre, clamped to the cell: continuous in the input) or,
with placement="mean", at their mean; its normal is the normalised sum of their normals; a triangle survives iff its three corners
lie in three different cells, keeping its order and winding; cells that no surviving triangle names are dropped.  Coincident duplicate
triangles are KEPT (two sheets closer than a cell collapse onto each other; removing them is out of scope).  A shape may come out
empty.  Every sum has one order, so GPU and twin agree bit for bit.

The grid of a shape.  cell=: edge length h and `origin`, up to 16384 cells per axis (vertices beyond are clamped into the last cell).
cells=: origin = the minimum of the shape's bounding box, h = its largest side / cells in float32; a shape without extent (no
vertices, or a single point) gets h = 1, one cell.  Refused before any launch: more than 16384 cells, an h that is not a positive
finite number, more than one of cell / cells / target_triangles, 2^20 shapes or more, 2^31 vertices or triangles or more.

Host synchronisation: cells= and target_triangles= read the bounding boxes once; every round of the target search reads the per-shape
counts once; every call reads the number of clusters once and the new offsets once.  The two sorts (vertex keys, stably; corner
records) are torch.sort.
"""
import numpy as np
import torch

from . import lib as L
from .lib import check, f32c, ptr, stream
from .mesh import MeshBatch

MAX_CELLS = L.abi.core_defines("simplify_core.h")["SG_SIMPLIFY_MAX_CELLS"]
MAX_SHAPES = 1 << 20
PLACEMENTS = {"quadric": 0, "mean": 1}
_ONE = np.float32(1.0)


def _ints(nbytes, device):
    """Scratch that holds flags, positions and offsets: a typed integer tensor, never a byte workspace."""
    return torch.empty(max(int(nbytes) // 4, 1), dtype=torch.int32, device=device)


class _Packed(object):
    """The contiguous arrays of a batch and its sizes, checked against the limits of one call."""

    def __init__(self, batch):
        self.verts, self.norms, self.faces = f32c(batch.vertices), f32c(batch.normals), batch.faces.contiguous()
        self.vo, self.to = batch.vert_offsets.contiguous(), batch.tri_offsets.contiguous()
        self.dev = self.verts.device
        self.S, self.V, self.F = len(batch), self.verts.shape[0], self.faces.shape[0]
        if not 1 <= self.S < MAX_SHAPES or self.V >= 2 ** 31 or self.F >= 2 ** 31:
            raise ValueError("simplify_meshes: %d shapes / %d vertices / %d triangles exceed the limits of one call (2^20 shapes, "
                             "2^31 vertices or triangles)" % (self.S, self.V, self.F))


class _Grid(object):
    """Per shape, on the host: origin [S,3] f32, h and 1 / h [S] f32, cells per axis [S]; checked, then uploaded."""

    def __init__(self, origin, h, cells):
        self.origin = np.ascontiguousarray(origin, dtype=np.float32)
        self.h = np.ascontiguousarray(h, dtype=np.float32)
        self.cells = np.ascontiguousarray(cells, dtype=np.int64)
        if (self.cells < 1).any() or (self.cells > MAX_CELLS).any():
            raise ValueError("simplify_meshes: cells per axis must lie in [1, %d], got %d .. %d" % (MAX_CELLS, self.cells.min(), self.cells.max()))
        if not (np.isfinite(self.h) & (self.h > 0)).all():
            raise ValueError("simplify_meshes: the cell size must be a positive finite number")
        if not np.isfinite(self.origin).all():
            raise ValueError("simplify_meshes: the grid origin must be finite")
        self.inv_h = _ONE / self.h

    def upload(self, dev):
        cell = np.stack([self.h, self.inv_h], axis=1)
        return (torch.from_numpy(self.origin).to(dev), torch.from_numpy(np.ascontiguousarray(cell)).to(dev),
                torch.from_numpy(self.cells.astype(np.int32)).to(dev))


def bounding_boxes(batch):
    """(lo, hi) [S,3] float32 on the batch's device: the bounding box of the finite coordinates of every shape, zeros for a shape (or
    an axis) without one."""
    p = _Packed(batch)
    lo = torch.empty((p.S, 3), dtype=torch.float32, device=p.dev)
    hi = torch.empty((p.S, 3), dtype=torch.float32, device=p.dev)
    try:
        check(L.load().sg_simplify_bounds(ptr(p.verts), ptr(p.vo), p.S, p.V, ptr(lo), ptr(hi), stream()), "simplify_bounds")
    finally:
        L.reset_call_state()
    return lo, hi


def _box_grid(lo, hi, cells):
    """The grid of `cells` [S] cells along the largest side of the boxes lo, hi [S,3] (numpy float32)."""
    side = (hi - lo).max(axis=1).astype(np.float32)
    with np.errstate(all="ignore"):
        h = side / cells.astype(np.float32)
    h = np.where(np.isfinite(h) & (h > 0), h, _ONE).astype(np.float32)
    return _Grid(lo, h, cells)


def _keys(p, grid):
    origin, cell, cells = grid
    keys = torch.empty(p.V, dtype=torch.int64, device=p.dev)
    try:
        check(L.load().sg_simplify_keys(ptr(p.verts), ptr(p.vo), p.S, p.V, ptr(origin), ptr(cell), ptr(cells), ptr(keys), stream()),
              "simplify_keys")
    finally:
        L.reset_call_state()
    return keys


def surviving_triangles(batch, grid):
    """[S] int32 on the batch's device: the triangles each shape would keep on `grid` (a _Grid), from the keys alone."""
    p = batch if isinstance(batch, _Packed) else _Packed(batch)
    keys = _keys(p, grid.upload(p.dev))
    counts = torch.empty(p.S, dtype=torch.int32, device=p.dev)
    try:
        check(L.load().sg_simplify_count(ptr(p.faces), ptr(p.vo), ptr(p.to), p.S, p.V, p.F, ptr(keys), ptr(counts), stream()),
              "simplify_count")
    finally:
        L.reset_call_state()
    return counts


def _search(p, lo, hi, before, target):
    """Per shape the cells in [1, 16384] of a bisection on the surviving count: lo = 1 leaves nothing, hi = 16384 is taken to leave too
    much; mid = (lo + hi) // 2 moves lo when its count is <= target, else hi; the answer is lo.  All shapes advance in the same rounds
    (14), one read of the counts per round.  The count is not monotone in the cells: the answer leaves <= target, not the most."""
    active = before > target
    low, high = np.ones(p.S, dtype=np.int64), np.full(p.S, MAX_CELLS, dtype=np.int64)
    while active.any() and (high - low)[active].max() > 1:
        mid = np.where(active, (low + high) // 2, 1)
        counts = surviving_triangles(p, _box_grid(lo, hi, mid)).cpu().numpy().astype(np.int64)      # the round's device -> host read
        fits = counts <= target
        moving = active & (high - low > 1)
        low = np.where(moving & fits, mid, low)
        high = np.where(moving & ~fits, mid, high)
    return np.where(active, low, 1), ~active


def _clusters(p, grid):
    """(keys [V] int64, sorted_keys, order [V] int64, sorted_cluster, vertex_cluster [V] int32, cluster_offsets [S+1] int64) of the
    packed batch on the uploaded grid: the keys sorted stably, the clusters numbered in key order."""
    lib = L.load()
    dev, S, V = p.dev, p.S, p.V
    keys = _keys(p, grid)
    sorted_keys, order = torch.sort(keys, stable=True)
    ws = _ints(lib.sg_simplify_clusters_workspace_bytes(S, V), dev)
    sorted_cluster = torch.empty(V, dtype=torch.int32, device=dev)
    vertex_cluster = torch.empty(V, dtype=torch.int32, device=dev)
    co = torch.empty(S + 1, dtype=torch.int64, device=dev)
    try:
        check(lib.sg_simplify_clusters(ptr(sorted_keys), ptr(order), ptr(p.vo), S, V, ptr(sorted_cluster), ptr(vertex_cluster), ptr(co),
                                       ptr(ws), ws.numel() * 4, stream()), "simplify_clusters")
    finally:
        L.reset_call_state()
    return keys, sorted_keys, order, sorted_cluster, vertex_cluster, co


def _run(p, grid, placement):
    """The simplified MeshBatch of the packed batch on the uploaded grid."""
    lib = L.load()
    dev, S, V, F = p.dev, p.S, p.V, p.F
    origin, cell, cells = grid
    _, sorted_keys, order, sorted_cluster, vertex_cluster, co = _clusters(p, grid)
    C = int(co[S])      # a device -> host read: the number of clusters sizes everything below
    corner_sorted = None
    if placement == PLACEMENTS["quadric"]:
        corner_keys = torch.empty((F, 3), dtype=torch.int64, device=dev)
        try:
            check(lib.sg_simplify_corners(ptr(p.faces), ptr(p.vo), ptr(p.to), S, V, F, ptr(vertex_cluster), ptr(corner_keys), stream()),
                  "simplify_corners")
        finally:
            L.reset_call_state()
        corner_sorted = torch.sort(corner_keys.reshape(-1)).values
    cv = torch.empty((C, 3), dtype=torch.float32, device=dev)
    cn = torch.empty((C, 3), dtype=torch.float32, device=dev)
    try:
        check(lib.sg_simplify_place(ptr(p.verts), ptr(p.norms), ptr(p.faces), ptr(p.vo), ptr(p.to), S, V, F, ptr(sorted_keys), ptr(order),
                                    ptr(sorted_cluster), ptr(corner_sorted), C, ptr(origin), ptr(cell), placement, ptr(cv), ptr(cn),
                                    stream()), "simplify_place")
    finally:
        L.reset_call_state()
    ws = _ints(lib.sg_simplify_faces_workspace_bytes(S, C, F), dev)
    nvo = torch.empty(S + 1, dtype=torch.int64, device=dev)
    nto = torch.empty(S + 1, dtype=torch.int64, device=dev)
    try:
        check(lib.sg_simplify_faces_count(ptr(p.faces), ptr(p.vo), ptr(p.to), S, V, F, ptr(vertex_cluster), ptr(co), C, ptr(nvo), ptr(nto),
                                          ptr(ws), ws.numel() * 4, stream()), "simplify_faces_count")
    finally:
        L.reset_call_state()
    host = torch.stack([nvo, nto]).cpu().numpy()      # a device -> host read: the totals size the outputs
    Vn, Fn = int(host[0, S]), int(host[1, S])
    out_v = torch.empty((Vn, 3), dtype=torch.float32, device=dev)
    out_n = torch.empty((Vn, 3), dtype=torch.float32, device=dev)
    out_f = torch.empty((Fn, 3), dtype=torch.int64, device=dev)
    try:
        check(lib.sg_simplify_faces_emit(ptr(cv), ptr(cn), ptr(p.faces), ptr(p.vo), ptr(p.to), S, V, F, ptr(vertex_cluster), C, ptr(nvo),
                                         ptr(out_v), ptr(out_n), ptr(out_f), Vn, Fn, ptr(ws), ws.numel() * 4, stream()),
              "simplify_faces_emit")
    finally:
        L.reset_call_state()
    out = MeshBatch(out_v, out_n, out_f, nvo, nto)
    out._host_offsets = (host[0].copy(), host[1].copy())
    return out


def _splice(p, simplified, unchanged):
    """The batch that takes the shapes of `unchanged` (bool [S], numpy) from the packed original and the others from `simplified`
    (where the unchanged shapes are empty): rows gathered in shape order, the offsets re-summed."""
    dev, S = p.dev, p.S
    keep = torch.from_numpy(unchanged).to(dev)
    ids = torch.arange(S, dtype=torch.int64, device=dev)

    def merge(rows_o, off_o, rows_s, off_s):
        n_o, n_s = off_o[1:] - off_o[:-1], off_s[1:] - off_s[:-1]
        ids_o = torch.repeat_interleave(ids, n_o, output_size=rows_o[0].shape[0])
        ids_s = torch.repeat_interleave(ids, n_s, output_size=rows_s[0].shape[0])
        taken = keep[ids_o]
        perm = torch.sort(torch.cat([ids_s, ids_o[taken]]), stable=True).indices
        off = torch.zeros(S + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(torch.where(keep, n_o, n_s), 0)
        return [torch.cat([s, o[taken]])[perm].contiguous() for o, s in zip(rows_o, rows_s)], off

    (verts, norms), vo = merge((p.verts, p.norms), p.vo, (simplified.vertices, simplified.normals), simplified.vert_offsets)
    (faces,), to = merge((p.faces,), p.to, (simplified.faces,), simplified.tri_offsets)
    return MeshBatch(verts, norms, faces, vo, to)


def _per_shape(value, S, what):
    a = np.asarray(value)
    if a.ndim == 0:
        a = np.full(S, a)
    if a.shape != (S,) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("simplify_meshes: %s must be an integer or one integer per shape (%d), got %r" % (what, S, value))
    return a.astype(np.int64)


def simplify_meshes(batch, cell=None, origin=(-1.0, -1.0, -1.0), cells=None, target_triangles=None, placement="quadric"):
    """(the simplified MeshBatch, info) of `batch`; exactly one of
        cell=h                  cells of edge h from `origin`: a shape's result does not depend on the rest of the batch;
        cells=k                 k cells (an int, or one per shape) along the largest side of each shape's own bounding box;
        target_triangles=t      per shape (an int, or one per shape) the cells of a bisection over [1, 16384] on the surviving count
                                whose result has at most t triangles (not the most possible: the count is not monotone); a shape that
                                already has at most t triangles is returned unchanged.
    placement: "quadric" or "mean".  info: per shape, tensors [S] on the CPU: "cells" (int64; 0 for a shape returned unchanged),
    "cell" (float32: its h), "triangles_before", "triangles_after" (int64).  Coincident duplicate triangles are kept."""
    if sum(x is not None for x in (cell, cells, target_triangles)) != 1:
        raise ValueError("simplify_meshes: give exactly one of cell=, cells=, target_triangles=")
    if placement not in PLACEMENTS:
        raise ValueError("simplify_meshes: placement is 'quadric' or 'mean', got %r" % (placement,))
    p = _Packed(batch)
    S = p.S
    before = (p.to[1:] - p.to[:-1]).cpu().numpy().astype(np.int64)
    unchanged = np.zeros(S, dtype=bool)
    if cell is not None:
        o = np.asarray(origin, dtype=np.float32).reshape(-1)
        if o.shape != (3,):
            raise ValueError("simplify_meshes: origin has three coordinates, got %r" % (origin,))
        grid = _Grid(np.tile(o, (S, 1)), np.full(S, cell, dtype=np.float32), np.full(S, MAX_CELLS))
    else:
        if cells is not None:
            k = _per_shape(cells, S, "cells")
            if (k < 1).any() or (k > MAX_CELLS).any():      # before the launch that reads the boxes
                raise ValueError("simplify_meshes: cells per axis must lie in [1, %d], got %d .. %d" % (MAX_CELLS, k.min(), k.max()))
        else:
            target = _per_shape(target_triangles, S, "target_triangles")
            if (target < 0).any():
                raise ValueError("simplify_meshes: target_triangles cannot be negative")
        lo, hi = (t.cpu().numpy() for t in bounding_boxes(batch))      # the device -> host read of the boxes
        if cells is None:
            k, unchanged = _search(p, lo, hi, before, target)
        grid = _box_grid(lo, hi, k)
    out = _run(p, grid.upload(p.dev), PLACEMENTS[placement])
    if unchanged.any():
        out = _splice(p, out, unchanged)
    after = out._offsets()[1]
    info = {"cells": torch.from_numpy(np.where(unchanged, 0, grid.cells)), "cell": torch.from_numpy(grid.h.copy()),
            "triangles_before": torch.from_numpy(before), "triangles_after": torch.from_numpy(np.diff(after).astype(np.int64))}
    return out, info


def simplify_option(value):
    """The keyword arguments of simplify_meshes behind a `simplify=` value: an int is target_triangles, a dict the arguments
    themselves; None / False: no simplification (None is returned)."""
    if value is None or value is False:
        return None
    if isinstance(value, dict):
        return dict(value)
    if isinstance(value, (int, np.integer)) and not isinstance(value, bool):
        return {"target_triangles": int(value)}
    raise ValueError("simplify: expected an int (target_triangles) or a dict of simplify_meshes' arguments, got %r" % (value,))


def apply_option(batch, value):
    """`batch` simplified as `simplify=value` asks (simplify_option); the batch itself when it asks for nothing."""
    options = simplify_option(value)
    return batch if options is None else simplify_meshes(batch, **options)[0]
