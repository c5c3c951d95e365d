"""Scores for generated point clouds: Chamfer distance, MMD, COV, 1-NNA and JSD (csrc/pointcloud.hip; CPU tensors run on the twin).

The reference stops at the clouds: metrics.py:18-46 writes them, rescaled to the half unit sphere, for the evaluation code of
Achlioptas et al. ("Learning Representations and Generative Models for 3D Point Clouds").  This module computes that code's
quantities on the clouds `metrics.sample_point_clouds` / `sample_from_voxels` return:

    scores = evaluate(generated, dataset)          # {'mmd_cd', 'cov_cd', 'one_nna_cd', 'jsd'}

    ab, ba = chamfer_matrix(generated, dataset)    # [Sa, Sb] float64 each; the Chamfer distance is ab + ba
    mmd, cov = mmd_cov(ab, ba)
    chamfer_distance(a, b)                         # [S] for matched batches

    evaluate(generated, dataset, emd=True)         # also 'mmd_emd', 'cov_emd', 'one_nna_emd'
    earth_movers_distance(a, b, eps=1e-4)          # [S] for matched batches of equal point count: within eps of the optimum
    emd_matrix(generated, dataset, eps=1e-4)       # [Sa, Sb] float64

Clouds are numpy arrays or tensors [S, P, 3] of any float type (cast to float32).  Tensors are computed on their own device, numpy
arrays on the device of the tensor they are paired with, or on `util.device` when there is none.  Distances are SQUARED, summed
over both directions of means (that code's convention).  The numerics of a pair, the tie rule and the summation order are part
of the C ABI: include/shapegan_hip.h, K13.  The reductions over the [Sa, Sb] matrices are small and stay in torch.

The earth mover's distance (csrc/emd.hip; K15) is that code's second family: the mean EUCLIDEAN distance, not squared, of the best
one-to-one matching of two clouds of the same point count (at most 2048), found by an auction that ends within `eps` per point of
the optimum: a bound, where that code's approxmatch has none.  The default eps = 1e-4 leaves three significant digits of the scores
of about 5e-2 that are usually quoted.
"""
import numpy as np
import torch

from . import lib as L
from . import util
from .lib import check, ptr, stream

_MAX_CLOUDS_PER_CALL = 65535      # include/shapegan_hip.h, K13


def _tensor(x, dev):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(x)
    elif not torch.is_tensor(x):
        x = torch.as_tensor(x)
    if x.dim() == 2:
        x = x.unsqueeze(0)
    if x.dim() != 3 or x.shape[2] != 3 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("expected clouds [S, P, 3] with S, P >= 1, got %s" % (tuple(x.shape),))
    return x.detach().to(dtype=torch.float32).to(dev).contiguous()


def _clouds(*xs):
    """float32 contiguous tensors on one device: that of the tensors among `xs` (they must agree), else util.device."""
    devs = {x.device for x in xs if torch.is_tensor(x)}
    if len(devs) > 1:
        raise RuntimeError("shapegan_amd.evaluation: the clouds live on different devices: %s" % sorted(str(d) for d in devs))
    dev = devs.pop() if devs else util.device
    return [_tensor(x, dev) for x in xs]


def _matrix_call(a, b, want_ab=True, want_ba=True):
    Sa, P, Sb, Q = a.shape[0], a.shape[1], b.shape[0], b.shape[1]
    dev = a.device
    lib = L.load()
    ab = torch.empty((Sa, Sb), dtype=torch.float64, device=dev) if want_ab else None
    ba = torch.empty((Sa, Sb), dtype=torch.float64, device=dev) if want_ba else None
    ws = L.workspace("chamfer_matrix", lib.sg_chamfer_matrix_workspace_bytes(Sa, Sb, P, Q), dev)
    try:
        check(lib.sg_chamfer_matrix(ptr(a), ptr(b), Sa, Sb, P, Q, ptr(ab), ptr(ba), ptr(ws), ws.numel(), stream()), "chamfer_matrix")
    finally:
        L.reset_call_state()
    return ab, ba


def _matrix(a, b, chunk=None, want_ab=True, want_ba=True):
    rows = min(int(chunk), _MAX_CLOUDS_PER_CALL) if chunk else _MAX_CLOUDS_PER_CALL
    if rows < 1:
        raise ValueError("chunk must be positive")
    cols = _MAX_CLOUDS_PER_CALL
    if a.shape[0] <= rows and b.shape[0] <= cols:
        return _matrix_call(a, b, want_ab, want_ba)
    blocks = [[_matrix_call(a[i:i + rows], b[j:j + cols], want_ab, want_ba) for j in range(0, b.shape[0], cols)]
              for i in range(0, a.shape[0], rows)]
    return tuple(torch.cat([torch.cat([blk[k] for blk in row], dim=1) for row in blocks], dim=0) if want else None
                 for k, want in enumerate((want_ab, want_ba)))


def chamfer_matrix(a, b, chunk=None):
    """(ab, ba), float64 [Sa, Sb] each: ab[i, j] is the mean over the points of a[i] of the squared distance to the nearest point
    of b[j], ba[i, j] the same from the points of b[j] to a[i].  `chunk`: clouds of `a` per library call (default: all)."""
    a, b = _clouds(a, b)
    return _matrix(a, b, chunk)


def nearest_neighbours(a, b):
    """Matched batches a [S, P, 3], b [S, Q, 3] -> (dist_a [S, P] float32, idx_a [S, P] int32, dist_b [S, Q], idx_b [S, Q]): the
    squared distance from every point to the nearest point of the other cloud and that point's index (the lowest of a tie)."""
    a, b = _clouds(a, b)
    if a.shape[0] != b.shape[0]:
        raise ValueError("matched batches need the same number of clouds, got %d and %d" % (a.shape[0], b.shape[0]))
    P, Q, dev = a.shape[1], b.shape[1], a.device
    outs = [[], [], [], []]
    lib = L.load()
    for s in range(0, a.shape[0], _MAX_CLOUDS_PER_CALL):
        ca, cb = a[s:s + _MAX_CLOUDS_PER_CALL], b[s:s + _MAX_CLOUDS_PER_CALL]
        S = ca.shape[0]
        da = torch.empty((S, P), dtype=torch.float32, device=dev)
        ia = torch.empty((S, P), dtype=torch.int32, device=dev)
        db = torch.empty((S, Q), dtype=torch.float32, device=dev)
        ib = torch.empty((S, Q), dtype=torch.int32, device=dev)
        try:
            check(lib.sg_chamfer_nearest(ptr(ca), ptr(cb), S, P, Q, ptr(da), ptr(ia), ptr(db), ptr(ib), stream()), "chamfer_nearest")
        finally:
            L.reset_call_state()
        for o, t in zip(outs, (da, ia, db, ib)):
            o.append(t)
    return tuple(o[0] if len(o) == 1 else torch.cat(o) for o in outs)


def chamfer_distance(a, b, return_indices=False):
    """[S] float64: mean_a min_b |a - b|^2 + mean_b min_a |a - b|^2 for matched batches; with return_indices also (idx_a, idx_b)."""
    da, ia, db, ib = nearest_neighbours(a, b)
    d = da.double().mean(dim=1) + db.double().mean(dim=1)
    return (d, ia, ib) if return_indices else d


_EMD_MAX_POINTS = L.abi.DEFINES["SG_EMD_MAX_POINTS"]            # include/shapegan_hip.h, K15
_EMD_STATUS = {1: "the auction reached the round cap (SG_EMD_ROUND_CAP)", 2: "eps is too small for the distances of this pair"}


def _emd_clouds(a, b, eps):
    devs = sorted({str(x.device) for x in (a, b) if torch.is_tensor(x)})
    if len(devs) > 1:
        raise ValueError("shapegan_amd.evaluation: the clouds live on different devices: %s" % devs)
    a, b = _clouds(a, b)
    if a.shape[1] != b.shape[1]:
        raise ValueError("the earth mover's distance needs clouds of the same point count, got %d and %d" % (a.shape[1], b.shape[1]))
    if a.shape[1] > _EMD_MAX_POINTS:
        raise ValueError("the earth mover's distance takes clouds of at most %d points, got %d" % (_EMD_MAX_POINTS, a.shape[1]))
    eps = float(eps)
    if not (eps > 0.0 and eps < float("inf")):
        raise ValueError("eps must be a positive finite number, got %r" % (eps,))
    # K15: integer costs d / (eps / 4) below 2^22.  The diagonal of the box around all finite points bounds every finite distance
    # (the factor covers the float32 roundings): a call that passes here has no pair with status 2.
    lo = torch.stack([torch.where(torch.isfinite(x), x, torch.full_like(x, float("inf"))).amin(dim=(0, 1)) for x in (a, b)]).amin(dim=0)
    hi = torch.stack([torch.where(torch.isfinite(x), x, torch.full_like(x, float("-inf"))).amax(dim=(0, 1)) for x in (a, b)]).amax(dim=0)
    span = (hi - lo).double().clamp_(min=0.0)
    smallest = float(torch.sqrt((span * span).sum())) * 2.0 ** -20 * (1 + 1e-6)
    if not eps >= max(smallest, 4.8e-38):
        raise ValueError("eps = %g is too small for clouds that span %g: the smallest eps accepted is %.3g" % (
            eps, float(span.max()), max(smallest, 4.8e-38)))
    return a, b, eps


def _emd_raise(status, name, pair_of):
    bad = status.reshape(-1).nonzero().flatten()
    if bad.numel():
        e = int(bad[0])
        code = int(status.reshape(-1)[e])
        raise RuntimeError("shapegan_amd.evaluation.%s: pair %s: %s (%d of %d pairs failed)" % (
            name, pair_of(e), _EMD_STATUS.get(code, "status %d" % code), bad.numel(), status.numel()))


def earth_movers_distance(a, b, eps=1e-4, return_matching=False):
    """[S] float64: for matched batches a, b [S, P, 3] the mean Euclidean distance of a one-to-one matching of the points of a[s] to
    the points of b[s] that is within `eps` (absolute, per point) of the best one; with return_matching also the matching
    [S, P] int32 (point i of a[s] goes to point match[s, i] of b[s]).  P <= 2048."""
    a, b, eps = _emd_clouds(a, b, eps)
    if a.shape[0] != b.shape[0]:
        raise ValueError("matched batches need the same number of clouds, got %d and %d" % (a.shape[0], b.shape[0]))
    P, dev = a.shape[1], a.device
    lib = L.load()
    values, matches = [], []
    for s in range(0, a.shape[0], _MAX_CLOUDS_PER_CALL):
        ca, cb = a[s:s + _MAX_CLOUDS_PER_CALL], b[s:s + _MAX_CLOUDS_PER_CALL]
        S = ca.shape[0]
        value = torch.empty((S,), dtype=torch.float64, device=dev)
        status = torch.empty((S,), dtype=torch.int32, device=dev)
        match = torch.empty((S, P), dtype=torch.int32, device=dev) if return_matching else None
        try:
            check(lib.sg_emd_match(ptr(ca), ptr(cb), S, P, eps, ptr(match), ptr(value), None, ptr(status), stream()), "emd_match")
        finally:
            L.reset_call_state()
        _emd_raise(status, "earth_movers_distance", lambda e, s=s: "%d" % (s + e))
        values.append(value)
        matches.append(match)
    value = values[0] if len(values) == 1 else torch.cat(values)
    return (value, matches[0] if len(matches) == 1 else torch.cat(matches)) if return_matching else value


def _emd_matrix_call(a, b, eps, symmetric, row0=0, col0=0):
    Sa, Sb, P, dev = a.shape[0], b.shape[0], a.shape[1], a.device
    lib = L.load()
    value = torch.empty((Sa, Sb), dtype=torch.float64, device=dev)
    status = torch.empty((Sa, Sb), dtype=torch.int32, device=dev)
    ws = L.workspace("emd_matrix", lib.sg_emd_matrix_workspace_bytes(Sa, Sb, P), dev)
    try:
        check(lib.sg_emd_matrix(ptr(a), ptr(b), Sa, Sb, P, eps, 1 if symmetric else 0, ptr(value), ptr(status), ptr(ws), ws.numel(),
                                stream()), "emd_matrix")
    finally:
        L.reset_call_state()
    _emd_raise(status, "emd_matrix", lambda e: "(%d, %d)" % (row0 + e // Sb, col0 + e % Sb))
    return value


def _emd_matrix(a, b, eps, chunk=None, symmetric=False):
    rows = min(int(chunk), _MAX_CLOUDS_PER_CALL) if chunk else _MAX_CLOUDS_PER_CALL
    if rows < 1:
        raise ValueError("chunk must be positive")
    if symmetric and (a.shape != b.shape or a.data_ptr() != b.data_ptr()) and not torch.equal(a, b):
        raise ValueError("symmetric=True takes the same set twice")
    Sa, Sb = a.shape[0], b.shape[0]
    if Sa <= rows and Sb <= _MAX_CLOUDS_PER_CALL:
        return _emd_matrix_call(a, b, eps, symmetric)
    if not symmetric:
        return torch.cat([torch.cat([_emd_matrix_call(a[i:i + rows], b[j:j + _MAX_CLOUDS_PER_CALL], eps, False, i, j)
                                     for j in range(0, Sb, _MAX_CLOUDS_PER_CALL)], dim=1) for i in range(0, Sa, rows)], dim=0)
    # the blocks on the diagonal by the symmetric form, the blocks above it in full ([i][j] with a[i] as bidders, as the header has
    # it), the blocks below it as their transposes
    out = torch.zeros((Sa, Sa), dtype=torch.float64, device=a.device)
    for i in range(0, Sa, rows):
        out[i:i + rows, i:i + rows] = _emd_matrix_call(a[i:i + rows], a[i:i + rows], eps, True, i, i)
        for j in range(i + rows, Sa, rows):
            blk = _emd_matrix_call(a[i:i + rows], a[j:j + rows], eps, False, i, j)
            out[i:i + rows, j:j + rows] = blk
            out[j:j + rows, i:i + rows] = blk.t()
    return out


def emd_matrix(a, b, eps=1e-4, chunk=None, symmetric=False):
    """[Sa, Sb] float64: entry [i, j] is earth_movers_distance(a[i], b[j]), bit for bit.  symmetric=True (a and b are the same set):
    only i < j is computed, [j, i] is its copy and the diagonal 0.  `chunk`: clouds of `a` per library call (default: all)."""
    a, b, eps = _emd_clouds(a, b, eps)
    return _emd_matrix(a, b, eps, chunk, symmetric)


def occupancy_histogram(clouds, resolution=28):
    """int64 [R, R, R]: the points of all clouds per cell of the grid with centres -0.5 + i / (R - 1) per axis (nearest centre,
    clamped to the grid: a point outside the cube counts in the border cell)."""
    (c,) = _clouds(clouds)
    R = int(resolution)
    hist = torch.zeros((R, R, R), dtype=torch.int64, device=c.device)
    try:
        check(L.load().sg_occupancy_histogram(ptr(c), c.shape[0], c.shape[1], R, ptr(hist), stream()), "occupancy_histogram")
    finally:
        L.reset_call_state()
    return hist


def _t64(x):
    return (torch.from_numpy(x) if isinstance(x, np.ndarray) else torch.as_tensor(x)).to(torch.float64)


def _mmd_cov(d):
    mmd = d.min(dim=0).values.mean()
    cov = torch.unique(d.argmin(dim=1)).numel() / float(d.shape[1])
    return mmd, cov


def mmd_cov(ab, ba):
    """(MMD, COV) of d = ab + ba with rows = generated clouds and columns = dataset clouds: MMD is the mean over the columns of
    the column minimum (every dataset cloud's distance to its nearest generated one), COV the share of columns that are the
    nearest dataset cloud (the row argmin) of at least one generated cloud."""
    mmd, cov = _mmd_cov(_t64(ab) + _t64(ba))
    return float(mmd), cov


def _one_nn(d_gg, d_gr, d_rr):
    ng, nr = d_gr.shape
    if d_gg.shape != (ng, ng) or d_rr.shape != (nr, nr):
        raise ValueError("one_nn_accuracy: expected [G,G], [G,R], [R,R], got %s %s %s" % (tuple(d_gg.shape), tuple(d_gr.shape), tuple(d_rr.shape)))
    m = torch.cat([torch.cat([d_gg, d_gr], dim=1), torch.cat([d_gr.t(), d_rr], dim=1)], dim=0).clone()
    m.fill_diagonal_(float("inf"))
    label = torch.cat([torch.zeros(ng, dtype=torch.bool), torch.ones(nr, dtype=torch.bool)]).to(m.device)
    return (label[m.argmin(dim=1)] == label).double().mean()


def one_nn_accuracy(d_gg, d_gr, d_rr):
    """Accuracy of the leave-one-out 1-nearest-neighbour classifier over the union of the generated (G) and the dataset (R) clouds,
    from the distance matrices generated-generated [G,G], generated-dataset [G,R] and dataset-dataset [R,R]: the share of
    clouds whose nearest other cloud is of their own set.  0.5 is ideal, 1.0 means the sets are trivially told apart."""
    return float(_one_nn(_t64(d_gg), _t64(d_gr), _t64(d_rr)))


def _entropy(p):
    p = p[p > 0]
    return float(-(p * np.log2(p)).sum())


def jsd_of_histograms(ha, hb):
    """Jensen-Shannon divergence (base 2, float64 on the host) of two count arrays of the same shape."""
    p = np.asarray(ha, dtype=np.float64).reshape(-1)
    q = np.asarray(hb, dtype=np.float64).reshape(-1)
    p, q = p / p.sum(), q / q.sum()
    return _entropy((p + q) / 2) - (_entropy(p) + _entropy(q)) / 2


def jsd(a, b, resolution=28):
    """Jensen-Shannon divergence between the occupancy histograms of two sets of clouds (occupancy_histogram)."""
    a, b = _clouds(a, b)
    h = torch.stack([occupancy_histogram(a, resolution), occupancy_histogram(b, resolution)]).cpu().numpy()
    return jsd_of_histograms(h[0], h[1])


def evaluate(generated, dataset, resolution=28, chunk=None, emd=False, emd_eps=1e-4):
    """{'mmd_cd', 'cov_cd', 'one_nna_cd', 'jsd'} of generated clouds [G, P, 3] against dataset clouds [R, Q, 3].  Three Chamfer
    matrices (generated-dataset in both directions, and one direction each of the two symmetric ones) and two histograms on the
    device; three scalars and the histograms come back to the host.  emd=True (P = Q <= 2048) adds 'mmd_emd', 'cov_emd' and
    'one_nna_emd': the same scores on the earth mover's distance, every entry within emd_eps of the exact one (one full and two
    symmetric matrices)."""
    if emd:
        g, r, emd_eps = _emd_clouds(generated, dataset, emd_eps)
    else:
        g, r = _clouds(generated, dataset)
    ab, ba = _matrix(g, r, chunk)
    gg, _ = _matrix(g, g, chunk, want_ba=False)      # ba of a set against itself is the transpose of ab
    rr, _ = _matrix(r, r, chunk, want_ba=False)
    d_gr = ab + ba
    mmd, cov = _mmd_cov(d_gr)
    nna = _one_nn(gg + gg.t(), d_gr, rr + rr.t())
    mmd, nna = (float(v) for v in torch.stack([mmd, nna]).cpu())
    h = torch.stack([occupancy_histogram(g, resolution), occupancy_histogram(r, resolution)]).cpu().numpy()
    scores = {"mmd_cd": mmd, "cov_cd": cov, "one_nna_cd": nna, "jsd": jsd_of_histograms(h[0], h[1])}
    if emd:
        e_gr = _emd_matrix(g, r, emd_eps, chunk)
        mmd, cov = _mmd_cov(e_gr)
        nna = _one_nn(_emd_matrix(g, g, emd_eps, chunk, symmetric=True), e_gr, _emd_matrix(r, r, emd_eps, chunk, symmetric=True))
        mmd, nna = (float(v) for v in torch.stack([mmd, nna]).cpu())
        scores.update(mmd_emd=mmd, cov_emd=cov, one_nna_emd=nna)
    return scores
