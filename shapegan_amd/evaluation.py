"""Scores for generated point clouds: Chamfer distance, MMD, COV, 1-NNA and JSD (csrc/pointcloud.hip; CPU tensors run on the twin).

The reference stops at the clouds: metrics.py:18-46 writes them, rescaled to the half unit sphere, for the evaluation code of
Achlioptas et al. ("Learning Representations and Generative Models for 3D Point Clouds").  This module computes that code's
quantities on the clouds `metrics.sample_point_clouds` / `sample_from_voxels` return:

    scores = evaluate(generated, dataset)          # {'mmd_cd', 'cov_cd', 'one_nna_cd', 'jsd'}

    ab, ba = chamfer_matrix(generated, dataset)    # [Sa, Sb] float64 each; the Chamfer distance is ab + ba
    mmd, cov = mmd_cov(ab, ba)
    chamfer_distance(a, b)                         # [S] for matched batches

Clouds are numpy arrays or tensors [S, P, 3] of any float type (cast to float32).  Tensors are computed on their own device, numpy
arrays on the device of the tensor they are paired with, or on `util.device` when there is none.  Distances are SQUARED, summed
over both directions of means (that code's convention).  The numerics of a pair, the tie rule and the summation order are part
of the C ABI: include/shapegan_hip.h, K13.  The reductions over the [Sa, Sb] matrices are small and stay in torch.
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


def evaluate(generated, dataset, resolution=28, chunk=None):
    """{'mmd_cd', 'cov_cd', 'one_nna_cd', 'jsd'} of generated clouds [G, P, 3] against dataset clouds [R, Q, 3].  Three Chamfer
    matrices (generated-dataset in both directions, and one direction each of the two symmetric ones) and two histograms on the
    device; three scalars and the histograms come back to the host."""
    g, r = _clouds(generated, dataset)
    ab, ba = _matrix(g, r, chunk)
    gg, _ = _matrix(g, g, chunk, want_ba=False)      # ba of a set against itself is the transpose of ab
    rr, _ = _matrix(r, r, chunk, want_ba=False)
    d_gr = ab + ba
    mmd, cov = _mmd_cov(d_gr)
    nna = _one_nn(gg + gg.t(), d_gr, rr + rr.t())
    mmd, nna = (float(v) for v in torch.stack([mmd, nna]).cpu())
    h = torch.stack([occupancy_histogram(g, resolution), occupancy_histogram(r, resolution)]).cpu().numpy()
    return {"mmd_cd": mmd, "cov_cd": cov, "one_nna_cd": nna, "jsd": jsd_of_histograms(h[0], h[1])}
