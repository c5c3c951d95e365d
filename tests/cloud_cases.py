"""Inputs and checks of the point-cloud SDF tests (K19), shared by the twin tier (tests/test_cloudsdf.py) and the GPU tier
(tests/test_gpu_cloudsdf.py).  References come from tests/cloud_reference.py (float64, numpy only), computed once per case and shared.

Every batch has an empty shape first, in the middle and last.  Cloud sizes sit on the edges of the kernel: the list length K, the query
tile and the LDS stage (both read from the header)."""
import functools

import numpy as np
import torch

import cloud_reference as R
from shapegan_amd import cloudsdf as C
from shapegan_amd import lib as L

TILE, STAGE, MAX_K = C.QUERY_TILE, C.STAGE, C.MAX_K
KS = (1, 8, 9, 11, 16, 17, 32)          # every list form, at and just above its edge
ERR_ARG = -1
U = 2.0 ** -24
D2_BOUND = 2.0 ** -21                   # 8 x the few units of 2^-24 of the six roundings of sg_pc_d2


def cloud_sizes():
    """0 first, in the middle and last; 1; K and K + 1 for every K of KS; the query tile and the LDS stage -1 / +0 / +1; 2 stages + 3."""
    small = sorted(set([1] + [k for K in KS for k in (K, K + 1)]))
    return [0] + small + [0, TILE - 1, TILE, TILE + 1, STAGE - 1, STAGE, STAGE + 1, 2 * STAGE + 3, 0]


def query_sizes():
    """Unrelated to the cloud sizes: 0, 1 and TILE + 1 (and a few more) meet small and large clouds alike."""
    cycle = [3, TILE + 1, 0, 1, 7]
    return [cycle[i % len(cycle)] for i in range(len(cloud_sizes()) - 2)] + [2 * TILE + 5, 0]


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def lattice_points(rng, n):
    """Multiples of 2^-6 in [-2, 2]; half of them on the coarse sub-lattice of multiples of 2^-1, so that distances tie massively and
    points coincide."""
    fine = rng.integers(-128, 129, size=(n, 3)).astype(np.float64) / 64.0
    coarse = rng.integers(-4, 5, size=(n, 3)).astype(np.float64) / 2.0
    return np.where(rng.random((n, 1)) < 0.5, coarse, fine).astype(np.float32)


def lattice_normals(rng, n):
    """Multiples of 2^-2 in [-1, 1] (products with lattice differences are exact in fp32), some of them (0, 0, 0)."""
    nrm = rng.integers(-4, 5, size=(n, 3)).astype(np.float32) / 4.0
    nrm[rng.random(n) < 0.1] = 0.0
    return nrm


@functools.lru_cache(maxsize=None)
def batch(kind, self_query):
    """(points, cloud offsets, queries, query offsets) as numpy arrays; one batch serves every K."""
    rng = np.random.default_rng((7 if kind == "lattice" else 13) + (1 if self_query else 0))
    sizes = cloud_sizes()
    co = offsets(sizes)
    make = lattice_points if kind == "lattice" else (lambda g, n: g.uniform(-1, 1, size=(n, 3)).astype(np.float32))
    points = make(rng, int(co[-1]))
    if kind == "lattice":
        for s, n in enumerate(sizes):      # duplicates of the first point of every cloud, among them one right behind it
            if n >= 3:
                points[co[s] + 1] = points[co[s]]
                points[co[s] + n - 1] = points[co[s]]
    if self_query:
        return points, co, points, co
    qo = offsets(query_sizes())
    queries = make(rng, int(qo[-1]))
    if kind == "lattice":
        for s in range(len(sizes)):        # some queries ON cloud points
            if sizes[s] and qo[s + 1] > qo[s]:
                queries[qo[s]] = points[co[s] + sizes[s] // 2]
    return points, co, queries, qo


@functools.lru_cache(maxsize=None)
def reference_order(kind, self_query):
    """The first MAX_K + 1 of the order (d2, index) of every query: one float64 pass serves every K."""
    p, co, q, qo = batch(kind, self_query)
    return R.knn(p, co, q, qo, MAX_K, exclude_self=self_query, extra=1)


def reference_knn(kind, K, self_query):
    idx, d2 = reference_order(kind, self_query)
    return idx[:, :K + 1], d2[:, :K + 1]


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- raw calls: the C ABI with its return code ----------------------------------------------------------------------------------------------
def raw_knn(dev, points, co, queries, qo, K, exclude_self, alloc_k=None):
    p, c, q, o = t(points, dev), t(co, dev), t(queries, dev), t(qo, dev)
    k = max(1, min(K, MAX_K)) if alloc_k is None else alloc_k
    idx = torch.full((len(queries), k), -7, dtype=torch.int32, device=dev)
    d2 = torch.full((len(queries), k), -7.0, dtype=torch.float32, device=dev)
    try:
        rc = L.load().sg_cloud_knn(L.ptr(p), L.ptr(c), L.ptr(q), L.ptr(o), len(co) - 1, len(points), len(queries), K, int(exclude_self),
                                   L.ptr(idx), L.ptr(d2), L.stream())
    finally:
        L.reset_call_state()
    return rc, idx, d2


def run_knn(dev, kind, K, self_query):
    p, co, q, qo = batch(kind, self_query)
    idx, d2 = C.knn_ragged(t(p, dev), t(co, dev), t(q, dev), t(qo, dev), K, exclude_self=self_query)
    return idx.cpu().numpy(), d2.cpu().numpy()


# ---- checks ------------------------------------------------------------------------------------------------------------------------------
def check_lattice_exact(dev, K, self_query):
    idx, d2 = run_knn(dev, "lattice", K, self_query)
    ref_idx, ref_d2 = reference_knn("lattice", K, self_query)
    assert np.array_equal(idx, ref_idx[:, :K])
    assert np.array_equal(d2.astype(np.float64), ref_d2[:, :K])
    if self_query:      # the duplicate right behind the first point of a cloud is its nearest neighbour, at distance 0
        _, co, _, _ = batch("lattice", True)
        for s, n in enumerate(cloud_sizes()):
            if n >= 3:
                assert idx[co[s], 0] == 1 and d2[co[s], 0] == 0 and idx[co[s] + 1, 0] == 0
                assert not (idx[co[s]:co[s + 1]] == np.arange(n)[:, None]).any()


def gap_rows(ref_d2, K):
    """Queries whose K-th and (K + 1)-th float64 distances are further apart than the bound (or that have no (K + 1)-th)."""
    a, b = ref_d2[:, K - 1], ref_d2[:, K]
    with np.errstate(invalid="ignore"):
        return ~np.isfinite(b) | (b - a > D2_BOUND * b)


def check_random_reference_has_gaps(K, self_query):
    _, ref_d2 = reference_knn("random", K, self_query)
    assert gap_rows(ref_d2, K).mean() >= 0.95


def check_random_against_float64(dev, K, self_query):
    idx, d2 = run_knn(dev, "random", K, self_query)
    ref_idx, ref_d2 = reference_knn("random", K, self_query)
    ref_idx, ref_k = ref_idx[:, :K], ref_d2[:, :K]
    assert np.array_equal(np.isfinite(d2), np.isfinite(ref_k)) and np.array_equal(idx >= 0, ref_idx >= 0)
    fin = np.isfinite(ref_k)
    err = np.abs(d2.astype(np.float64)[fin] - ref_k[fin])
    print("K=%d worst relative d2 error %.3g (bound %.3g)" % (K, (err / ref_k[fin]).max() if err.size else 0.0, D2_BOUND))
    assert (err <= D2_BOUND * ref_k[fin]).all()
    with np.errstate(invalid="ignore"):
        assert (np.diff(d2, axis=1)[np.isfinite(d2[:, 1:])] >= 0).all()
    rows = gap_rows(ref_d2, K)
    assert rows.mean() >= 0.95
    assert np.array_equal(np.sort(idx[rows], axis=1), np.sort(ref_idx[rows], axis=1))


def check_bitwise_equal(a, b):
    for x, y in zip(a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.dtype == y.dtype
        assert np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)


def check_batch_independence(dev, K):
    """The same cloud alone and at each position among others: the same bits."""
    rng = np.random.default_rng(5)
    cloud = rng.uniform(-1, 1, size=(STAGE + 37, 3)).astype(np.float32)
    others = [rng.uniform(-1, 1, size=(n, 3)).astype(np.float32) for n in (0, 300, 5)]
    alone = C.knn_ragged(t(cloud, dev), t(offsets([len(cloud)]), dev), t(cloud, dev), t(offsets([len(cloud)]), dev), K, exclude_self=True)
    for pos in range(len(others) + 1):
        parts = others[:pos] + [cloud] + others[pos:]
        co = offsets([len(x) for x in parts])
        pts = np.concatenate(parts)
        idx, d2 = C.knn_ragged(t(pts, dev), t(co, dev), t(pts, dev), t(co, dev), K, exclude_self=True)
        check_bitwise_equal([x.cpu().numpy() for x in alone], [idx[co[pos]:co[pos + 1]].cpu().numpy(), d2[co[pos]:co[pos + 1]].cpu().numpy()])


def nonfinite_batch():
    rng = np.random.default_rng(11)
    sizes = [0, STAGE + 5, 40, 0, 3, 0]
    co = offsets(sizes)
    points = rng.uniform(-1, 1, size=(int(co[-1]), 3)).astype(np.float32)
    bad = rng.choice(len(points), 60, replace=False)
    points[bad[:20], 0] = np.nan
    points[bad[20:40], 1] = np.inf
    points[bad[40:], 2] = -np.inf
    points[co[4]:co[5]] = np.nan                       # a cloud of nothing finite
    qo = offsets([2, TILE + 9, 5, 4, 3, 0])
    queries = rng.uniform(-1, 1, size=(int(qo[-1]), 3)).astype(np.float32)
    queries[qo[1] + 3] = np.nan
    queries[qo[1] + 4, 1] = np.inf
    queries[qo[1] + 5] = 3e38                           # d2 overflows to +inf
    return points, co, queries, qo


def run_nonfinite(dev, K=16):
    p, co, q, qo = nonfinite_batch()
    idx, d2 = C.knn_ragged(t(p, dev), t(co, dev), t(q, dev), t(qo, dev), K)
    sidx, sd2 = C.knn_ragged(t(p, dev), t(co, dev), t(p, dev), t(co, dev), K, exclude_self=True)
    out = [x.cpu().numpy() for x in (idx, d2, sidx, sd2)]
    for which, (i, d, o) in enumerate(((out[0], out[1], qo), (out[2], out[3], co))):
        for s in range(len(co) - 1):
            rows = slice(int(o[s]), int(o[s + 1]))
            assert (i[rows] >= -1).all() and (i[rows] < co[s + 1] - co[s]).all()
        assert np.isfinite(d[i >= 0]).all() and np.isposinf(d[i < 0]).all()
    assert (out[0][qo[4]:qo[5]] == -1).all() and (out[0][qo[1] + 3:qo[1] + 6] == -1).all()
    return out


def check_argument_errors(dev):
    p, co, q, qo = batch("lattice", False)
    assert raw_knn(dev, p, co, q, qo, 0, False)[0] == ERR_ARG
    assert raw_knn(dev, p, co, q, qo, MAX_K + 1, False)[0] == ERR_ARG
    assert raw_knn(dev, p, co, q, qo, 8, True, alloc_k=8)[0] == ERR_ARG            # unequal runs
    same_total = offsets([len(p)] + [0] * (len(co) - 2))                          # equal totals, different runs
    assert raw_knn(dev, p, co, p, same_total, 8, True)[0] == ERR_ARG
    rc, idx, d2 = raw_knn(dev, p, co, p, co, 8, True)
    assert rc == 0 and (idx.cpu().numpy() != -7).all()
    bad = co.copy()
    bad[10] = bad[11] + 1                                                          # a run of negative length
    assert raw_knn(dev, p, bad, q, qo, 8, False)[0] == ERR_ARG
    idx = torch.zeros((len(p), 8), dtype=torch.int32, device=dev)
    for K in (0, MAX_K + 1):
        pts, offs, nrm, var = t(p, dev), t(co, dev), torch.zeros((len(p), 3), device=dev), torch.zeros(len(p), device=dev)
        try:
            rc = L.load().sg_cloud_normals(L.ptr(pts), L.ptr(offs), len(co) - 1, len(p), L.ptr(idx), K, None, 0, L.ptr(nrm), L.ptr(var), L.stream())
        finally:
            L.reset_call_state()
        assert rc == ERR_ARG
    for wrong in (t(p.astype(np.float64), dev), t(p, dev)[:, :2], t(p, dev).t()):      # the Python wrappers refuse what a pointer would misread
        try:
            C.knn_ragged(wrong, t(co, dev), t(q, dev), t(qo, dev), 8)
        except ValueError:
            continue
        raise AssertionError("knn_ragged accepted %s %s" % (wrong.dtype, tuple(wrong.shape)))
    try:
        C.knn_ragged(t(p, dev), t(co.astype(np.int32), dev), t(q, dev), t(qo, dev), 8)
    except ValueError:
        pass
    else:
        raise AssertionError("knn_ragged accepted int32 offsets")
    with_k = dict(points=t(p, dev), normals=t(p, dev), co=t(co, dev), q=t(q, dev), qo=t(qo, dev))
    for K in (0, MAX_K + 1):
        sdf = torch.zeros(len(q), dtype=torch.float32, device=dev)
        try:
            rc = L.load().sg_cloud_sdf(L.ptr(with_k["points"]), L.ptr(with_k["normals"]), L.ptr(with_k["co"]), L.ptr(with_k["q"]),
                                       L.ptr(with_k["qo"]), len(co) - 1, len(p), len(q), K, L.ptr(sdf), None, L.stream())
        finally:
            L.reset_call_state()
        assert rc == ERR_ARG


# ---- normals ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def normal_batch():
    """A Fibonacci sphere of radius 0.5, a noisy plane, empty shapes around them: (points, offsets)."""
    rng = np.random.default_rng(3)
    sphere = R.fibonacci_sphere(TILE * 3 + 11).astype(np.float32)
    plane = np.stack([rng.uniform(-0.5, 0.5, 700), rng.uniform(-0.5, 0.5, 700), rng.normal(0, 0.002, 700)], axis=1).astype(np.float32)
    parts = [np.zeros((0, 3), np.float32), sphere, np.zeros((0, 3), np.float32), plane, np.zeros((0, 3), np.float32)]
    return np.concatenate(parts), offsets([len(x) for x in parts])


def run_normals(dev, points, co, K, view=None, per_point=False):
    p, c = t(points, dev), t(co, dev)
    idx, _ = C.knn_ragged(p, c, p, c, K, exclude_self=True)
    n, var = C.normals_ragged(p, c, idx, None if view is None else t(np.asarray(view, dtype=np.float32), dev), per_point)
    return idx.cpu().numpy(), n.cpu().numpy(), var.cpu().numpy()


@functools.lru_cache(maxsize=None)
def reference_normals(K):
    """From the float64 eigh of the neighbour sets of the float64 k-NN of the batch (which the exact-order tests tie to the kernels')."""
    points, co = normal_batch()
    idx, _ = R.knn(points, co, points, co, K, exclude_self=True)
    return (idx,) + R.normals(points, co, idx)


def check_normals_against_float64(dev, K):
    points, co = normal_batch()
    idx, n, var = run_normals(dev, points, co, K)
    ref_idx, ref_n, lam, count = reference_normals(K)
    same = (np.sort(idx, axis=1) == np.sort(ref_idx, axis=1)).all(axis=1)      # the sets may differ only at a near-tie of the K-th
    assert same.mean() > 0.99
    trace = lam.sum(axis=1)
    gap = lam[:, 1] - lam[:, 0]
    ok = gap >= 0.01 * trace
    assert ok.mean() >= 0.9                                                     # the reference alone
    rows = ok & same
    length = np.linalg.norm(n.astype(np.float64), axis=1)
    assert np.abs(length[rows] - 1).max() < 8 * U
    sin = np.linalg.norm(np.cross(n[rows].astype(np.float64), ref_n[rows]), axis=1) / length[rows]
    bound = 16 * (K + 1) * U * trace[rows] / gap[rows]
    print("K=%d worst sin(angle) / bound = %.3g" % (K, (sin / bound).max()))
    assert (sin <= bound).all()
    assert np.abs(var[rows] - lam[rows, 0] / trace[rows]).max() < 1e-4
    # unoriented: the component of largest magnitude is positive
    big = np.abs(n[rows]).argmax(axis=1)
    assert (n[rows][np.arange(rows.sum()), big] > 0).all()


def check_normal_views(dev, K=16):
    """All three forms of `view`: per shape a position, per shape a direction, per point."""
    points, co = normal_batch()
    S, N = len(co) - 1, len(points)
    _, free, _ = run_normals(dev, points, co, K)
    centre = np.zeros((S, 4), np.float32)
    centre[:, 3] = 1                                                             # a scanner AT the centre: sphere normals point inward
    _, inward, _ = run_normals(dev, points, co, K, centre)
    up = np.tile(np.array([0, 0, 1, 0], np.float32), (S, 1))                     # toward +z from far away
    _, upward, _ = run_normals(dev, points, co, K, up)
    per_point = np.concatenate([points * 4, np.ones((N, 1), np.float32)], axis=1)   # a scanner outside, over every point
    _, outward, _ = run_normals(dev, points, co, K, per_point, True)
    sphere = slice(int(co[1]), int(co[2]))
    plane = slice(int(co[3]), int(co[4]))
    radial = points[sphere] / np.linalg.norm(points[sphere], axis=1, keepdims=True)
    assert ((inward[sphere] * radial).sum(axis=1) < -0.9).all()
    assert ((outward[sphere] * radial).sum(axis=1) > 0.9).all()
    assert (upward[plane][:, 2] > 0.9).mean() > 0.95 and (upward[plane][:, 2] >= 0).all()
    for oriented, view in ((inward, np.repeat(centre, np.diff(co), axis=0)), (upward, np.repeat(up, np.diff(co), axis=0)), (outward, per_point)):
        # the same line as the unoriented normal, the side from the contract's rule on the normal the kernel made
        assert np.array_equal(np.abs(oriented), np.abs(free))
        e = view[:, :3].astype(np.float64) - view[:, 3:4].astype(np.float64) * points
        dot = (oriented.astype(np.float64) * e).sum(axis=1)
        assert (dot >= -1e-6).all()


def degenerate_batch():
    """Collinear neighbourhoods, coincident points, clouds of 1 and 2 points (fewer than 3 samples), a good one for contrast."""
    line = np.stack([np.arange(40) / 64.0, np.zeros(40), np.zeros(40)], axis=1).astype(np.float32)
    same = np.tile(np.array([[0.25, -0.5, 0.75]], np.float32), (20, 1))
    one, two = np.array([[0.5, 0.5, 0.5]], np.float32), np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    rng = np.random.default_rng(8)
    good = (rng.integers(-64, 65, size=(60, 3)) / 64.0).astype(np.float32)
    parts = [np.zeros((0, 3), np.float32), line, same, np.zeros((0, 3), np.float32), one, two, good, np.zeros((0, 3), np.float32)]
    return np.concatenate(parts), offsets([len(x) for x in parts])


def check_degenerate_normals(dev, K=8):
    points, co = degenerate_batch()
    _, n, var = run_normals(dev, points, co, K)
    flat = slice(0, int(co[6]))
    assert (n[flat] == 0).all() and (var[flat] == -1).all()
    good = slice(int(co[6]), int(co[7]))
    assert np.abs(np.linalg.norm(n[good], axis=1) - 1).max() < 1e-6 and (var[good] >= 0).all()


def check_translation_invariance(dev, K=16):
    points, co = translation_batch()
    moved = points + np.array([0.75, -0.5, 0.25], np.float32)                    # exact in fp32 on the lattice
    assert np.array_equal(moved.astype(np.float64), points.astype(np.float64) + np.array([0.75, -0.5, 0.25]))
    a, b = run_normals(dev, points, co, K), run_normals(dev, moved, co, K)
    check_bitwise_equal(a, b)
    assert (np.linalg.norm(a[1], axis=1) > 0.5).mean() > 0.9


def translation_batch():
    rng = np.random.default_rng(21)
    co = offsets([0, 500, 0, TILE + 3, 0])
    return (rng.integers(-64, 65, size=(int(co[-1]), 3)) / 64.0).astype(np.float32), co


def tie_cloud():
    """Two neighbourhoods whose answer is decided by a tie rule, every number exact in fp32; point 0 (the origin) with all the others as
    its neighbours is the one that is looked at.
    equal eigenvalues: samples (+-a, 0, 0), (0, +-a, 0), (0, 0, +-b): the sums are diagonal, xx = yy < zz, no rotation happens and the
      two smallest eigenvalues tie: the LOWEST column, (1, 0, 0).
    equal components: samples +-(a, a, 0), +-(e, -e, 0), (0, 0, +-b), e < a: xx = yy and xy > 0, so the one rotation has theta = 0, t = 1 and
      s = c bit for bit; the smallest eigenvalue has the column (c, -c, 0), whose two components tie in magnitude: the LOWEST axis is made
      positive, (+, -, 0) — the highest-axis rule would give (-, +, 0)."""
    a, e, b = 0.5, 0.25, 1.0
    first = np.array([[0, 0, 0], [a, 0, 0], [-a, 0, 0], [0, a, 0], [0, -a, 0], [0, 0, b], [0, 0, -b]], np.float32)
    second = np.array([[0, 0, 0], [a, a, 0], [-a, -a, 0], [e, -e, 0], [-e, e, 0], [0, 0, b], [0, 0, -b]], np.float32)
    return np.concatenate([first, second]), offsets([0, len(first), 0, len(second), 0])


def check_tie_rules(dev):
    points, co = tie_cloud()
    _, n, var = run_normals(dev, points, co, 6)
    assert np.array_equal(n[co[1]], np.array([1, 0, 0], np.float32)) and var[co[1]] == np.float32(0.5 / 3.0)      # 2 a^2 / (4 a^2 + 2 b^2)
    x, y, z = n[co[3]]
    assert x > 0 and y == -x and z == 0 and abs(float(x) - 0.5 ** 0.5) < 1e-7
    # K = 8 > the 6 neighbours there are: the same neighbourhood through -1 slots
    _, n8, _ = run_normals(dev, points, co, 8)
    assert np.array_equal(n8[[co[1], co[3]]], n[[co[1], co[3]]])


def normal_outputs(dev):
    """Everything the normals kernel makes on the test inputs, for the GPU-equals-twin comparison: every K form, no view, a position per
    shape, a direction (w = 0) per shape, a view per point of both kinds, the translated lattice cloud, the degenerate and the tie cases."""
    out = []
    points, co = normal_batch()
    S, N = len(co) - 1, len(points)
    position = np.tile(np.array([0.1, 0.2, 2.0, 1.0], np.float32), (S, 1))
    direction = np.tile(np.array([0.6, 0.0, 0.8, 0.0], np.float32), (S, 1))
    rng = np.random.default_rng(41)
    per_point = np.concatenate([rng.normal(size=(N, 3)), (rng.random((N, 1)) < 0.5)], axis=1).astype(np.float32)      # w = 0 and w = 1 mixed
    for K in (3, 8, 16, 32):
        for view, pp in ((None, False), (position, False), (direction, False), (per_point, True)):
            out += list(run_normals(dev, points, co, K, view, pp))
    moved, mco = translation_batch()
    out += list(run_normals(dev, moved, mco, 16)) + list(run_normals(dev, moved + np.array([0.75, -0.5, 0.25], np.float32), mco, 16))
    out += list(run_normals(dev, *degenerate_batch(), 8)) + list(run_normals(dev, *tie_cloud(), 6))
    return out


# ---- sg_cloud_sdf ----------------------------------------------------------------------------------------------------------------------------
def run_sdf(dev, points, normals, co, queries, qo, K):
    sdf, nearest = C.sdf_ragged(t(points, dev), t(normals, dev), t(co, dev), t(queries, dev), t(qo, dev), K, want_nearest=True)
    return sdf.cpu().numpy(), nearest.cpu().numpy()


@functools.lru_cache(maxsize=None)
def sdf_batch(kind):
    p, co, q, qo = batch(kind, False)
    rng = np.random.default_rng(77)
    if kind == "lattice":
        n = lattice_normals(rng, len(p))
    else:
        n = rng.normal(size=(len(p), 3)).astype(np.float32)
    return p, n, co, q, qo


def check_sdf_lattice_composition(dev, K):
    """Exactly the composition knn -> gather -> vote of the reference: every step is exact in fp32 on the lattice but the final sqrt."""
    p, n, co, q, qo = sdf_batch("lattice")
    sdf, nearest = run_sdf(dev, p, n, co, q, qo, K)
    ref, ref_nearest = R.sdf(p, n, co, q, qo, K)
    assert np.array_equal(nearest, ref_nearest)
    assert np.array_equal(sdf, ref.astype(np.float32))                           # sqrtf of an exact d2 = the rounded float64 root
    empty = np.concatenate([np.arange(qo[s], qo[s + 1]) for s in range(len(co) - 1) if co[s + 1] == co[s]])
    assert np.isposinf(sdf[empty]).all() and (nearest[empty] == -1).all()
    small = np.concatenate([np.arange(qo[s], qo[s + 1]) for s in range(len(co) - 1) if 0 < co[s + 1] - co[s] < K] or [np.zeros(0, int)])
    if K > 1:
        assert len(small)                                                        # n_valid < K is on the path
    assert (sdf < 0).any() and (sdf > 0).any()


def check_tied_vote(dev):
    """An even K whose votes tie is not inside; one more negative vote is."""
    p = np.array([[0, 0, 0.25], [0, 0, -0.25], [0.5, 0, 0], [-0.5, 0, 0]], np.float32)
    up, down = [0, 0, 1], [0, 0, -1]
    q = np.array([[0, 0, 0]], np.float32)
    co, qo = offsets([0, 4, 0]), offsets([0, 1, 0])
    # t_j = (q - p_j) . n_j:  -0.25, -0.25 for the two samples on the axis with normals up / down; 0 for the others
    tie = np.array([up, down, up, down], np.float32)                             # votes: -, -, 0, 0 -> 2 of 4: not inside
    assert run_sdf(dev, p, tie, co, q, qo, 4)[0][0] == np.float32(0.25)
    assert run_sdf(dev, p, tie, co, q, qo, 2)[0][0] == np.float32(-0.25)         # the two nearest alone: 2 of 2
    three = tie.copy()
    three[2] = [1, 0, 0]                                                         # (q - p_2) . n = -0.5: 3 of 4
    assert run_sdf(dev, p, three, co, q, qo, 4)[0][0] == np.float32(-0.25)
    assert run_sdf(dev, p, three, co, q, qo, 32)[0][0] == np.float32(-0.25)      # n_valid = 4 < K


def covering_radius_bound(p64, radius=0.5):
    """A tight upper bound, in float64, of the covering radius of samples on the sphere: the largest chord distance from a point of
    the sphere to its nearest sample.  That distance is 1-Lipschitz, so its maximum lies within rho of a probe whose value is within
    rho of the largest probe value, rho bounding the probes' own covering radius (a Fibonacci set of M probes: the side of a square of
    a probe's share of the area, 1.6 times the circumradius of a hexagon of that area).  Around every such probe a tangent grid of
    step rho / 6 covers the disc of radius 1.1 rho; a grid point's distance is taken to the probe's 8 nearest samples only, which can
    only make it larger.  The bound is the largest grid value plus the grid's half diagonal, plus the samples' own distance from
    the sphere."""
    probes = R.fibonacci_sphere(24 * len(p64), radius)
    value, near = np.empty(len(probes)), np.empty((len(probes), 8), dtype=np.int64)
    for i in range(0, len(probes), 4096):
        d = R.pair_d2(probes[i:i + 4096], p64)
        near[i:i + 4096] = np.argpartition(d, 8, axis=1)[:, :8]
        value[i:i + 4096] = np.sqrt(d.min(axis=1))
    rho = radius * np.sqrt(4 * np.pi / len(probes))
    cand = np.nonzero(value >= value.max() - rho)[0]
    c = probes[cand]
    u = np.cross(c, np.where(np.abs(c[:, :1]) < 0.4, [[1.0, 0, 0]], [[0, 1.0, 0]]))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(c, u) / radius
    step = rho / 6
    ticks = np.arange(-7, 8) * step                                               # +-7 steps = 1.17 rho
    ga, gb = (g.reshape(-1) for g in np.meshgrid(ticks, ticks, indexing="ij"))
    fine = c[:, None, :] + ga[None, :, None] * u[:, None, :] + gb[None, :, None] * v[:, None, :]
    fine *= radius / np.linalg.norm(fine, axis=2, keepdims=True)
    d = np.sqrt(((fine[:, :, None, :] - p64[near[cand]][:, None, :, :]) ** 2).sum(axis=3).min(axis=2))
    return d.max() + step * np.sqrt(0.5) + np.abs(np.linalg.norm(p64, axis=1) - radius).max()


@functools.lru_cache(maxsize=None)
def sphere_case():
    """A Fibonacci sphere of radius 0.5 with exact outward normals, h = covering_radius_bound of the input points, and queries with
    | |q| - 0.5 | > h, inside and outside, a third of them within 1.5 h of the shell where the vote is hardest."""
    rng = np.random.default_rng(31)
    count = STAGE + 3
    points = R.fibonacci_sphere(count).astype(np.float32)
    p64 = points.astype(np.float64)
    h = covering_radius_bound(p64)
    normals = (p64 / np.linalg.norm(p64, axis=1, keepdims=True)).astype(np.float32)
    n = 4 * TILE + 9
    direction = rng.normal(size=(n, 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    lo = h * (1 + 1e-4)                                                          # beyond the rounding of the queries to float32
    d = np.where(rng.random(n) < 1 / 3, rng.uniform(lo, 1.5 * h, n), rng.uniform(lo, 0.5, n))
    radius = np.where(rng.random(n) < 0.5, 0.5 - d, 0.5 + d)
    queries = (direction * radius[:, None]).astype(np.float32)
    return points, normals, queries, h


def check_sphere_geometry(dev, K=11):
    """For every query with | |q| - 0.5 | > h: the sign is that of |q| - 0.5, and d_true <= |sdf| up to 2^-20.  The upper bound: with f the
    foot of q on the sphere and p the sample nearest to q (the one at the smallest angle from f, so |f - p| <= h),
    |q - p|^2 = d^2 + |f - p|^2 (1 -+ 2 d) for q inside / outside (q's radius is 0.5 -+ d, and |f - p|^2 = 0.5 (1 - cos angle)).
    INSIDE the assertion is the issue's, |sdf| <= sqrt(d_true^2 + h^2).  OUTSIDE that form is not a bound of the exact nearest-sample
    distance — a query at distance d over a point of the sphere that is h from its nearest sample is sqrt(d^2 + (1 + 2 d) h^2) from
    it —, so there the assertion is |sdf| <= sqrt(d_true^2 + (1 + 2 d_true) h^2): the one place where this test departs from the
    issue's text.  The figures against both forms are printed."""
    points, normals, queries, h = sphere_case()
    co, qo = offsets([0, len(points), 0]), offsets([0, len(queries), 0])
    sdf, _ = run_sdf(dev, points, normals, co, queries, qo, K)
    r = np.linalg.norm(queries.astype(np.float64), axis=1)
    true = np.abs(r - 0.5)
    inside, outside = r < 0.5, r > 0.5
    assert (true > h).all() and (inside & (true < 1.5 * h)).sum() > 50 and (outside & (true < 1.5 * h)).sum() > 50
    assert np.array_equal(np.sign(sdf), np.sign(r - 0.5))
    mag = np.abs(sdf.astype(np.float64))
    slack = 1 + 2.0 ** -20
    assert (mag * slack >= true).all()
    plain = np.sqrt(true ** 2 + h ** 2)
    exact_outside = np.sqrt(true ** 2 + (1 + 2 * true) * h ** 2)
    print("h = %.5g; inside: worst |sdf| / sqrt(d^2 + h^2) = %.6f; outside: worst |sdf| / sqrt(d^2 + h^2) = %.6f, / sqrt(d^2 + (1 + 2 d) h^2) = %.6f"
          % (h, (mag / plain)[inside].max(), (mag / plain)[outside].max(), (mag / exact_outside)[outside].max()))
    assert (mag[inside] <= plain[inside] * slack).all()
    assert (mag[outside] <= exact_outside[outside] * slack).all()


def sdf_outputs(dev):
    out = []
    for kind in ("lattice", "random"):
        for K in KS:
            out += list(run_sdf(dev, *sdf_batch(kind), K))
    return out


def knn_outputs(dev):
    out = []
    for kind in ("lattice", "random"):
        for K in KS:
            for self_query in (False, True):
                out += list(run_knn(dev, kind, K, self_query))
    return out


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def sphere_cloud(dev, count=900):
    p = R.fibonacci_sphere(count).astype(np.float32)
    n = (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)
    return t(p, dev), t(n, dev)


def check_voxels_equal_sdf_on_the_grid(dev):
    p, n = sphere_cloud(dev)
    single = C.CloudSDF(p, n)
    voxels = single.get_voxels(8)
    c = torch.linspace(-1.0, 1.0, 8, dtype=torch.float64)
    grid = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), dim=-1).reshape(-1, 3).float()
    assert voxels.shape == (8, 8, 8) and torch.equal(voxels.reshape(-1), single.get_sdf(grid))
    assert (voxels[0, 0, 0] > 0) and (voxels < 0).any()
    both = C.CloudSDF([p, torch.zeros((0, 3)), p[:300]], [n, torch.zeros((0, 3)), n[:300]], device=dev)
    grids = both.get_voxels(8)
    assert grids.shape == (3, 8, 8, 8) and torch.equal(grids[0], voxels) and torch.isposinf(grids[1]).all()
    assert torch.equal(grids[2].reshape(-1), C.CloudSDF(p[:300], n[:300]).get_sdf(grid))


def check_sample_sdf_near_surface(dev):
    from shapegan_amd.prepare import BadMeshException
    p, n = sphere_cloud(dev)
    cloud = C.CloudSDF([p, torch.zeros((0, 3)), p[:500] * 0.5], [n, torch.zeros((0, 3)), n[:500]], device=dev)
    number = 1000
    ns = int(number * 47 / 50) // 2
    a = cloud.sample_sdf_near_surface(number, generator=torch.Generator().manual_seed(4))
    b = cloud.sample_sdf_near_surface(number, generator=torch.Generator().manual_seed(4))
    other = cloud.sample_sdf_near_surface(number, generator=torch.Generator().manual_seed(5))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[0], other[0])
    points, sdf, ok = a
    assert points.shape == (3, number, 3) and sdf.shape == (3, number) and ok.tolist() == [True, False, True]
    # the two surface parts: the same cloud points under coarse and fine noise; the rest inside the unit sphere
    near = C.knn_ragged(cloud.points, cloud.offsets, points[0, :2 * ns].contiguous(), t(offsets([2 * ns, 0, 0]), dev), 1)[1].sqrt()
    assert float(near[:ns].max()) < 0.0025 * 6 and float(near[ns:].max()) < 0.00025 * 6
    assert float((points[0, :ns] - points[0, ns:2 * ns]).abs().max()) < 0.0025 * 12
    assert float(points[:, 2 * ns:].norm(dim=2).max()) < 1.0 and float(points[0, 2 * ns:].norm(dim=1).max()) > 0.8
    assert torch.isposinf(sdf[1]).all()
    single = C.CloudSDF(p, n)
    sp, ss = single.sample_sdf_near_surface(number, generator=torch.Generator().manual_seed(4))
    assert sp.shape == (number, 3) and ss.shape == (number,)
    try:
        C.CloudSDF(torch.zeros((0, 3), device=dev), torch.zeros((0, 3), device=dev)).sample_sdf_near_surface(100)
    except BadMeshException:
        pass
    else:
        raise AssertionError("an empty cloud is a bad cloud")


CUBE_V = np.array([[x, y, z] for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], dtype=np.float64)
CUBE_F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]],
                  dtype=np.int64)


def check_from_scans_cube(dev, K=16):
    """The cloud of ONE scan of a cube: every normal faces the scan; a point whose neighbourhood lies in one face has that face's normal
    within the accuracy bound of the normals test (float64 eigh of the same neighbours)."""
    from shapegan_amd import prepare
    scans = prepare.SurfaceScans((CUBE_V, CUBE_F), 1.0, scan_count=6, scan_resolution=48, device=dev)
    cloud = C.CloudSDF.from_scans(scans, keep=[0], k_normals=K)
    d = scans.directions[0]
    pts, nrm = cloud.points.cpu().numpy().astype(np.float64), cloud.normals.cpu().numpy().astype(np.float64)
    assert cloud.single and len(pts) > 300 and len(pts) == int(((scans.depth[0, 0] < 1.0).sum()))
    good = np.linalg.norm(nrm, axis=1) > 0.5
    assert good.mean() > 0.99 and (nrm[good] @ d > 0).all()
    visible = [(axis, sign) for axis in range(3) for sign in (-1.0, 1.0) if sign * d[axis] > 1e-6]
    on_face = np.stack([np.abs(pts[:, axis] - 0.5 * sign) < 1e-4 for axis, sign in visible], axis=1)
    assert on_face.any(axis=1).mean() > 0.99                                     # the scan sees nothing but the visible faces
    co = offsets([len(pts)])
    idx, _ = C.knn_ragged(cloud.points, cloud.offsets, cloud.points, cloud.offsets, K, exclude_self=True)
    idx = idx.cpu().numpy()
    ref_n, lam, _ = R.normals(cloud.points.cpu().numpy(), co, idx)
    trace, gap = lam.sum(axis=1), lam[:, 1] - lam[:, 0]
    checked = 0
    for f, (axis, sign) in enumerate(visible):
        inner = on_face[:, f] & on_face[idx, f].all(axis=1) & good & (gap >= 0.01 * trace)
        face_normal = np.zeros(3)
        face_normal[axis] = sign
        sin = np.linalg.norm(np.cross(nrm[inner], ref_n[inner]), axis=1)
        assert (sin <= 16 * (K + 1) * U * trace[inner] / gap[inner]).all()
        assert (nrm[inner] @ face_normal > 1 - 1e-5).all()                       # and the plane of the points IS the face (to the depth map's 2e-5)
        checked += int(inner.sum())
    assert checked > 0.5 * len(pts)
    # a partial cloud is a subset of the full one, view by view
    full = C.CloudSDF.from_scans(scans)
    assert full.N > cloud.N and torch.equal(full.points[:cloud.N], cloud.points)
    capped = C.CloudSDF.from_scans(scans, max_points=200, generator=torch.Generator().manual_seed(0))
    assert capped.N == 200


def check_view_is_in_the_files_frame(dev, tmp_path):
    """A cloud far from the origin of its file, seen by a sensor AT that origin: the half of a sphere around (0, 0, 5) that faces the origin.
    Its normals must face the sensor — outward — although (0, 0, 0) of the frame the cloud is rescaled to lies inside or behind it."""
    p = R.fibonacci_sphere(1500, 0.5)
    p = p[p[:, 2] < -0.2]                                                        # a cap that the origin sees in both files (3 * 0.5 * 0.5 / 5 = 0.15)
    outward = p / np.linalg.norm(p, axis=1, keepdims=True)
    np.save(str(tmp_path / "far.npy"), (p + [0.0, 0.0, 5.0]).astype(np.float32))
    np.save(str(tmp_path / "near.npy"), (p * 3 + [0.0, 0.0, 5.0]).astype(np.float32))
    cloud = C.CloudSDF.from_files(C.get_cloud_files(str(tmp_path)), view=(0.0, 0.0, 0.0), device=dev)
    assert cloud.S == 2 and not cloud.single and cloud.N == 2 * len(p)
    assert float(cloud.points.norm(dim=1).max()) <= 1 + 1e-6                     # rescaled to the unit sphere ...
    n = cloud.normals.cpu().numpy().astype(np.float64)
    for s in range(2):                                                           # ... with the normals of the file's frame
        dots = (n[s * len(p):(s + 1) * len(p)] * outward).sum(axis=1)
        assert (dots > 0).all() and np.median(dots) > 0.99
    centre = torch.tensor([[[0.0, 0.0, 0.3]], [[0.0, 0.0, 0.3]]])                # behind the cap, inside the sphere it is a part of
    front = torch.tensor([[[0.0, 0.0, -0.9]], [[0.0, 0.0, -0.9]]])
    assert (cloud.get_sdf(centre) < 0).all() and (cloud.get_sdf(front) > 0).all()


def check_load_cloud_round_trips(tmp_path):
    from shapegan_amd.mesh import Mesh
    rng = np.random.default_rng(2)
    p = rng.uniform(-1, 1, size=(57, 3)).astype(np.float32)
    n = rng.normal(size=(57, 3)).astype(np.float32)
    np.save(str(tmp_path / "a.npy"), p)
    np.save(str(tmp_path / "b.npy"), np.concatenate([p, n], axis=1))
    with open(str(tmp_path / "c.xyz"), "w") as fh:
        fh.write("# a comment\n")
        fh.writelines("%.9g %.9g %.9g\n" % tuple(r) for r in p.tolist())
    with open(str(tmp_path / "d.xyz"), "w") as fh:
        fh.writelines("%.9g %.9g %.9g %.9g %.9g %.9g\n" % tuple(r) for r in np.concatenate([p, n], axis=1).tolist())
    faces = np.array([[0, 1, 2], [2, 3, 4]], dtype=np.int64)
    Mesh(p, faces).export(str(tmp_path / "e.ply"))
    Mesh(p, faces, vertex_normals=n).export(str(tmp_path / "f.ply"))
    for name, with_normals in (("a.npy", False), ("b.npy", True), ("c.xyz", False), ("d.xyz", True), ("e.ply", False), ("f.ply", True)):
        points, normals = C.load_cloud(str(tmp_path / name))
        assert points.dtype == np.float32 and np.array_equal(points, p), name
        assert (normals is not None) == with_normals and (normals is None or np.array_equal(normals, n)), name
    assert [name.rsplit("/", 1)[-1] for name in C.get_cloud_files(str(tmp_path))] == ["a.npy", "b.npy", "c.xyz", "d.xyz", "e.ply", "f.ply"]
    np.save(str(tmp_path / "bad.npy"), np.zeros((4, 5), np.float32))
    for bad in ("bad.npy", "g.stl"):
        try:
            C.load_cloud(str(tmp_path / bad))
        except ValueError:
            continue
        raise AssertionError("%s was read" % bad)


CUBE_OBJ = "".join("v %g %g %g\n" % tuple(v) for v in CUBE_V) + "".join("f %d %d %d\n" % tuple(f + 1) for f in CUBE_F)


def check_command_line(dev, tmp_path, state):
    """--clouds, --models --partial 1 and the untouched --models call: finite codes [S, L] each."""
    from shapegan_amd import reconstruct
    torch.save(state, str(tmp_path / "sdf_net.to"))
    latent = state["layers1.0.weight"].shape[1] - 3
    clouds = tmp_path / "clouds"
    clouds.mkdir()
    p = R.fibonacci_sphere(400).astype(np.float32)
    np.save(str(clouds / "oriented.npy"), np.concatenate([p, p / np.linalg.norm(p, axis=1, keepdims=True)], axis=1))
    np.save(str(clouds / "second.npy"), np.concatenate([p[:150] * [1, 0.5, 1], p[:150] / np.linalg.norm(p[:150], axis=1, keepdims=True)], axis=1).astype(np.float32))
    common = ["--net", str(tmp_path / "sdf_net.to"), "--iterations", "3", "--points", "512", "--device", dev]
    assert reconstruct.main(common + ["--clouds", str(clouds), "--out", str(tmp_path / "from_clouds.to")]) == 0
    codes = torch.load(str(tmp_path / "from_clouds.to"))
    assert codes.shape == (2, latent) and torch.isfinite(codes).all() and codes.abs().max() > 0
    bare = tmp_path / "bare"
    bare.mkdir()
    np.save(str(bare / "unoriented.npy"), p)
    assert reconstruct.main(common + ["--clouds", str(bare), "--view", "0", "0", "3", "--out", str(tmp_path / "from_bare.to")]) == 0
    assert torch.load(str(tmp_path / "from_bare.to")).shape == (1, latent)
    models = tmp_path / "models" / "abc" / "models"
    models.mkdir(parents=True)
    (models / "model_normalized.obj").write_text(CUBE_OBJ)
    scan = ["--models", str(tmp_path / "models"), "--scan-count", "6", "--scan-resolution", "48"]
    assert reconstruct.main(common + scan + ["--partial", "1", "--out", str(tmp_path / "partial.to")]) == 0
    partial = torch.load(str(tmp_path / "partial.to"))
    assert partial.shape == (1, latent) and torch.isfinite(partial).all()
    assert reconstruct.main(common + scan + ["--out", str(tmp_path / "mesh.to")]) == 0
    whole = torch.load(str(tmp_path / "mesh.to"))
    assert whole.shape == (1, latent) and torch.isfinite(whole).all() and not torch.equal(whole, partial)
    for bad in (common + ["--out", "x"], common + scan + ["--clouds", str(clouds), "--out", "x"], common + ["--clouds", str(clouds), "--partial", "1", "--out", "x"]):
        try:
            reconstruct.main(bad)
        except SystemExit as e:
            assert e.code == 2
        else:
            raise AssertionError("accepted: %s" % bad)


def check_public_functions(dev):
    """knn and estimate_normals in their dense and ragged forms agree with the raw entry points."""
    rng = np.random.default_rng(17)
    dense = t(rng.uniform(-1, 1, size=(3, 50, 3)).astype(np.float32), dev)
    queries = t(rng.uniform(-1, 1, size=(3, 7, 3)).astype(np.float32), dev)
    co, qo = t(offsets([50] * 3), dev), t(offsets([7] * 3), dev)
    idx, d2 = C.knn(dense, queries, k=5)
    raw = C.knn_ragged(dense.reshape(-1, 3), co, queries.reshape(-1, 3), qo, 5)
    assert idx.shape == (3, 7, 5) and torch.equal(idx.reshape(-1, 5), raw[0]) and torch.equal(d2.reshape(-1, 5), raw[1])
    own = C.knn(dense, k=4)
    assert own[0].shape == (3, 50, 4) and not (own[0] == torch.arange(50, device=own[0].device)[None, :, None]).any()
    ragged = C.knn((dense.reshape(-1, 3), co), (queries.reshape(-1, 3), qo), k=5)
    assert ragged[0].shape == (21, 5) and torch.equal(ragged[0], raw[0])
    n, var = C.estimate_normals(dense, k=8, view=[0.0, 0.0, 5.0], return_variation=True)
    assert n.shape == (3, 50, 3) and var.shape == (3, 50)
    toward = torch.tensor([0.0, 0.0, 5.0], device=n.device) - dense
    assert ((n * toward).sum(dim=2) >= -1e-6).all() and ((n.norm(dim=2) - 1).abs() < 1e-5).all()
    flat = C.estimate_normals((dense.reshape(-1, 3), co), k=8, view=torch.tensor([0.0, 0.0, 5.0, 1.0]).expand(3, 4))
    assert torch.equal(flat, n.reshape(-1, 3))
    for bad in (0, MAX_K + 1):
        try:
            C.knn(dense, k=bad)
        except ValueError:
            continue
        raise AssertionError("k = %d was accepted" % bad)
