"""Bodies shared by tests/test_brickgrid.py (the twin) and tests/test_gpu_brickgrid.py (the HIP kernels): the narrow-band driver
(shapegan_amd/brickgrid.py) on analytic fields pushed through its `evaluate` callable, against the numpy restatement of the rule
(tests/brickgrid_reference.py) and against marching cubes of the dense grid.

A field is built from elementwise float32 tensor operations, one rounding each, so a point has the same bits wherever it stands in
a call: the dense grid is the field on the whole lattice in lattice order.  The shapes of a batch differ (their parameters are
indexed by shape_index); with S = 3 the last one is empty (no crossing).
"""
import numpy as np
import torch

import brickgrid_reference as REF
from shapegan_amd import brickgrid as BG
from shapegan_amd.mesh import marching_cubes

RES = (8, 16, 24, 32)
BRICKS = (4, 8)
SHAPES = (1, 3)


def combos(min_bricks_per_axis=1):
    return [(R, B, S) for R in RES for B in BRICKS for S in SHAPES if R % B == 0 and R // B >= min_bricks_per_axis]


def h_of(R):
    return 2.0 / (R - 1)


# ---- fields: f(points [N,3], shape_index [N]) -> [N] ---------------------------------------------------------------------------------
def _per_shape(values, dev):
    return torch.tensor(values, dtype=torch.float32, device=dev)


def _dist(p, c):
    d = p - c
    return torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])


def sphere(dev, S, radius=0.55, centre=(0.1, -0.05, 0.15)):
    """shape 0: the sphere; shape 1: smaller and elsewhere; the last of three: radius < 0, no crossing."""
    r = _per_shape([radius, 0.6 * radius, -0.5][:S] if S > 1 else [radius], dev)
    c = _per_shape([list(centre), [-0.2, 0.25, -0.1], [0.0, 0.0, 0.0]][:S], dev)

    def f(p, sid):
        s = sid.long()
        return _dist(p, c[s]) - r[s]
    return f


def torus(dev, S):
    major = _per_shape([0.55, 0.4, 0.5][:S], dev)
    minor = _per_shape([0.2, 0.22, -0.3][:S], dev)

    def f(p, sid):
        s = sid.long()
        q = torch.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) - major[s]
        return torch.sqrt(q * q + p[:, 2] * p[:, 2]) - minor[s]
    return f


def two_spheres(dev, S):
    """two balls in opposite octants: their bricks are not adjacent when there are at least 4 bricks per axis"""
    r = _per_shape([0.3, 0.22, -0.4][:S], dev)
    a = torch.tensor([-0.55, -0.55, -0.55], device=dev)
    b = torch.tensor([0.55, 0.5, 0.6], device=dev)

    def f(p, sid):
        return torch.minimum(_dist(p, a), _dist(p, b)) - r[sid.long()]
    return f


def slab(dev, S):
    """|y - c| < t for all x and z: the inside reaches the border of the lattice"""
    c = _per_shape([0.05, -0.3, 0.0][:S], dev)
    t = _per_shape([0.3, 0.2, -0.2][:S], dev)

    def f(p, sid):
        s = sid.long()
        return torch.abs(p[:, 1] - c[s]) - t[s]
    return f


def no_crossing(dev, S):
    o = _per_shape([0.5, 0.7, 0.9][:S], dev)

    def f(p, sid):
        return _dist(p, torch.zeros(3, device=dev)) + o[sid.long()]
    return f


def big_sphere(dev, S):
    """reaches beyond |p| = 1.1: under the sphere_only mask the mask makes the crossing"""
    return sphere(dev, S, radius=1.3, centre=(0.0, 0.0, 0.0))


def rod(dev, R, B):
    """A rod one cell thick (radius 0.6 h around one lattice line) that runs along x through the middle of a row of bricks, between
    their corners, and ends in a ball that does reach brick corners.  One shape."""
    ax = np.linspace(-1.0, 1.0, R)
    h = h_of(R)
    line = B + B // 2 - 1 if R >= 2 * B else B // 2 - 1            # a lattice line 3 (B = 8) / 1 (B = 4) points from the brick faces
    yc, zc = float(ax[line]), float(ax[line])
    x0, x1 = float(ax[1]), float(ax[R - B // 2 - 2])
    ball = torch.tensor([x1, yc, zc], device=dev)
    radius_ball = 0.75 * B * h

    def f(p, sid):
        t = torch.clamp(p[:, 0], min=x0, max=x1) - p[:, 0]
        dy, dz = p[:, 1] - yc, p[:, 2] - zc
        d_rod = torch.sqrt(t * t + dy * dy + dz * dz) - 0.6 * h
        return torch.minimum(d_rod, _dist(p, ball) - radius_ball)
    return f


def floater(dev, R):
    """A ball of radius 1.2 h in the middle of the 8-brick (1, 1, 1) plus a large ball far from it (R = 32).  One shape."""
    ax = np.linspace(-1.0, 1.0, R)
    h = h_of(R)
    m = float(ax[11] + ax[12]) / 2
    small = torch.tensor([m, m, m], device=dev)
    large = torch.tensor([0.5, 0.5, 0.45], device=dev)

    def f(p, sid):
        return torch.minimum(_dist(p, small) - 1.2 * h, _dist(p, large) - 0.3)
    return f


FIELDS = {"sphere": sphere, "torus": torus, "two_spheres": two_spheres, "slab": slab, "no_crossing": no_crossing}


# ---- running ---------------------------------------------------------------------------------------------------------------------------
def lattice(R, dev):
    ax = BG.axis_tables(R, dev)
    return torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()


def unit_sphere_mask(R):
    from shapegan_amd.util import get_voxel_coordinates
    return torch.from_numpy(np.linalg.norm(get_voxel_coordinates(R), axis=1) < 1.1)


def dense_grid(field, S, R, dev, mask=None):
    p = lattice(R, dev)
    sid = torch.arange(S, dtype=torch.int32, device=dev).repeat_interleave(p.shape[0])
    d = field(p.repeat(S, 1), sid).reshape(S, R, R, R).clone()
    if mask is not None:
        d[:, ~mask.reshape(R, R, R).to(dev)] = 1.0
    return d


def run(field, S, R, B, dev, level=0.0, band=None, pad=True, mask=None):
    calls = []

    def evaluate(points, sid):
        calls.append(points.shape[0])
        return field(points, sid)
    res = BG.narrow_band_grids(evaluate, S, R, dev, brick=B, level=level, band=band, pad=pad, mask=mask)
    res.calls = calls
    return res


def mesh_of(grid, R, level, pad):
    return marching_cubes(grid, level=level, spacing=2.0 / R, origin=-1.0, pad=pad, pad_value=1.0)


def assert_same_mesh(a, b):
    for name in ("vert_offsets", "tri_offsets", "vertices", "normals", "faces"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape and torch.equal(x, y), "marching cubes differ in " + name


def assert_closed(batch):
    for s in range(len(batch)):
        m = batch.mesh(s)
        if m.faces.shape[0] == 0:
            continue
        e = np.sort(np.concatenate([m.faces[:, [0, 1]], m.faces[:, [1, 2]], m.faces[:, [2, 0]]]), axis=1)
        _, counts = np.unique(e, axis=0, return_counts=True)
        assert (counts == 2).all(), "shape %d: %d edges are not shared by exactly two triangles" % (s, int((counts != 2).sum()))


def check_against_reference(res, dense, B, level, band, pad, mask=None):
    """states, fills, lists and per-round counts equal the restatement exactly; the grid is the dense grid in the active bricks and
    the fill elsewhere"""
    ref = REF.narrow_band(dense.cpu().numpy(), B, level=level, band=band, pad=pad, mask=None if mask is None else mask.cpu().numpy())
    assert np.array_equal((res.state != 0).cpu().numpy(), ref["state"])
    assert np.array_equal(res.fill.cpu().numpy(), ref["fill"])
    assert res.stats["rounds"] == len(ref["rounds"]) and res.stats["bricks_per_round"] == [len(r) for r in ref["rounds"]]
    for got, want in zip(res.round_lists, ref["rounds"]):
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(res.grid.cpu().numpy(), ref["grid"])
    assert res.stats["active_bricks"] == ref["state"].sum(axis=1).tolist()
    ppb = B ** 3
    assert res.calls == [8 * ref["state"].size] + [len(r) * ppb for r in ref["rounds"]]
    return ref


def check_field(name, dev, R, B, S, level=0.0, pad=True, masked=False, band=None):
    """one field: the restatement, mesh equality and closedness"""
    field = big_sphere(dev, S) if name == "big_sphere" else FIELDS[name](dev, S)
    mask = unit_sphere_mask(R) if masked else None
    dense = dense_grid(field, S, R, dev, mask)
    res = run(field, S, R, B, dev, level=level, band=band, pad=pad, mask=mask)
    check_against_reference(res, dense, B, level, res.stats["band"], pad, mask)
    nb_mesh, dense_mesh = mesh_of(res.grid, R, level, pad), mesh_of(dense, R, level, pad)
    assert_same_mesh(nb_mesh, dense_mesh)
    if pad:
        assert_closed(nb_mesh)
    return res, nb_mesh


def check_rod(dev, R, B):
    field = rod(dev, R, B)
    dense = dense_grid(field, 1, R, dev)
    res = run(field, 1, R, B, dev, band=0.0)
    check_against_reference(res, dense, B, 0.0, 0.0, True)
    assert res.stats["rounds"] >= 3, res.stats
    assert res.stats["evaluated_points"][0] < R ** 3
    nb_mesh = mesh_of(res.grid, R, 0.0, True)
    assert_same_mesh(nb_mesh, mesh_of(dense, R, 0.0, True))
    assert_closed(nb_mesh)
    assert nb_mesh.faces.shape[0] > 0


def triangles(mesh):
    """the triangles of a Mesh as rows of 9 float32 coordinates (vertex order kept)"""
    return mesh.vertices[mesh.faces].reshape(-1, 9)


def missing_triangles_lie_in_inactive_bricks(nb_mesh, dense_mesh, state, R, B, strict=True):
    """Every narrow-band triangle is a dense triangle, and every vertex of a dense triangle that is missing sits on a crossing edge
    whose lattice end points belong to inactive bricks: both of them (strict: the piece lies strictly inside inactive bricks), or at
    least one (the piece's own lattice points lie in inactive bricks, its surface may reach the edges that leave them).  An end point
    in the virtual shell of 1 belongs to no brick.  -> the number of missing triangles.  (Meshes of one shape, padded, spacing 2 / R,
    origin -1.)"""
    nt, dt = triangles(nb_mesh), triangles(dense_mesh)
    as_set = lambda t: set(map(bytes, np.ascontiguousarray(t)))
    have, all_dense = as_set(nt), as_set(dt)
    assert have <= all_dense, "the narrow-band mesh has a triangle the dense mesh lacks"
    missing = np.array([i for i, row in enumerate(np.ascontiguousarray(dt)) if bytes(row) not in have], dtype=np.int64)
    nbx = R // B
    st = np.asarray(state).reshape(nbx, nbx, nbx) != 0
    # padded index = (position + 1) R / 2, lattice index = padded index - 1; two of a vertex's three are whole numbers (up to the
    # rounding of a float32 position, far below 1e-4), the third lies between the edge's end points
    u = (dt[missing].reshape(-1, 3).astype(np.float64) + 1.0) * R / 2.0 - 1.0
    inactive = []
    for end in (np.floor(u + 1e-4).astype(int), np.ceil(u - 1e-4).astype(int)):
        lattice = ((end >= 0) & (end < R)).all(axis=1)
        q = np.clip(end, 0, R - 1) // B
        inactive.append(np.where(lattice, ~st[q[:, 0], q[:, 1], q[:, 2]], strict))
    ok = (inactive[0] & inactive[1]) if strict else (inactive[0] | inactive[1])
    assert ok.all(), "a missing triangle has a vertex on an edge between evaluated points"
    return len(missing)


def check_floater(dev):
    R, B = 32, 8
    field = floater(dev, R)
    dense = dense_grid(field, 1, R, dev)
    dense_mesh = mesh_of(dense, R, 0.0, True)
    res = run(field, 1, R, B, dev, band=0.0)
    check_against_reference(res, dense, B, 0.0, 0.0, True)
    nb_mesh = mesh_of(res.grid, R, 0.0, True)
    assert_closed(nb_mesh)
    gone = missing_triangles_lie_in_inactive_bricks(nb_mesh.mesh(0), dense_mesh.mesh(0), res.state[0].cpu().numpy(), R, B)
    assert gone > 0 and not bool(res.state[0, (1 * 4 + 1) * 4 + 1]), "with band = 0 the floater is not found"
    found = run(field, 1, R, B, dev)          # the default band
    assert bool(found.state[0, (1 * 4 + 1) * 4 + 1])
    assert_same_mesh(mesh_of(found.grid, R, 0.0, True), dense_mesh)


def check_refusals(dev):
    import pytest
    calls = []

    def evaluate(points, sid):
        calls.append(1)
        return torch.zeros(points.shape[0], device=points.device)
    with pytest.raises(ValueError):
        BG.narrow_band_grids(evaluate, 1, 20, dev, brick=8)
    with pytest.raises(ValueError):
        BG.narrow_band_grids(evaluate, 1, 16, dev, brick=2)
    with pytest.raises(ValueError):
        BG.narrow_band_grids(evaluate, 1, 16, dev, brick=8, mask=torch.ones(15 ** 3, dtype=torch.bool))
    with pytest.raises(ValueError):
        BG.narrow_band_grids(evaluate, 0, 16, dev, brick=8)
    assert not calls, "a refused call reached the field"
    # the ABI refuses the same before any launch
    from shapegan_amd import lib as L
    lib = L.load()
    t = torch.zeros(64, dtype=torch.float32, device=dev)
    i = torch.zeros(64, dtype=torch.int32, device=dev)
    try:
        for S, Rr, Bb in ((1, 20, 8), (1, 16, 2), (0, 16, 8)):
            assert lib.sg_brick_seed(L.ptr(t), None, S, Rr, Bb, 0.0, 0.0, 1, L.ptr(i), L.ptr(t), L.ptr(i), L.ptr(t), L.stream()) == -1
            assert lib.sg_brick_compact_workspace_bytes(S, Rr, Bb) == 0
    finally:
        L.reset_call_state()


def check_determinism(dev):
    field = torus(dev, 3)
    a = run(field, 3, 24, 4, dev)
    b = run(field, 3, 24, 4, dev)
    assert torch.equal(a.grid, b.grid) and torch.equal(a.state, b.state) and torch.equal(a.fill, b.fill)
    assert len(a.round_lists) == len(b.round_lists) and all(torch.equal(x, y) for x, y in zip(a.round_lists, b.round_lists))


# ---- poison ------------------------------------------------------------------------------------------------------------------------------
def poison_snapshot(dev, R, B, S):
    res = run(two_spheres(dev, S), S, R, B, dev)
    return [res.grid.clone(), res.state.clone(), res.fill.clone()] + [r.clone() for r in res.round_lists]


def check_poison(dev):
    """The grid, states and fills are written in full and the lists up to their counts, with NaN (or zeros) in every fresh allocation
    and workspace; two runs are bit-identical; a small call right after a large one equals the small call alone."""
    from poison import poisoned
    plain = poison_snapshot(dev, 32, 4, 3)
    with poisoned() as p:
        first = poison_snapshot(dev, 32, 4, 3)
        p.renew()
        second = poison_snapshot(dev, 32, 4, 3)
        p.check_canaries()
    for got in (first, second):
        assert len(got) == len(plain)
        for a, b in zip(got, plain):
            assert not torch.isnan(a.float()).any(), "an output element was not written"
            assert torch.equal(a, b)
    alone = poison_snapshot(dev, 8, 4, 1)
    with poisoned() as p:
        poison_snapshot(dev, 32, 4, 3)
        after = poison_snapshot(dev, 8, 4, 1)
        p.check_canaries()
    assert len(after) == len(alone) and all(torch.equal(a, b) for a, b in zip(after, alone))
