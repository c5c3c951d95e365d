"""Poison-tier bodies of the point-cloud SDF entry points (tests/poison.py): each of the three writes every element of every output — the
-1 / +inf slots of short lists, the rows of empty shapes and a NULL `nearest` included —, changes no canary, and repeats bit for bit.
The entry points take no scratch: the results are their only stores."""
import numpy as np
import torch

import cloud_cases as K
from poison import poisoned
from shapegan_amd import cloudsdf as C

T, S = K.TILE, K.STAGE
# (cloud sizes, query sizes, k): edges of the list, the query tile and the stage; empty shapes first, in the middle and last
CASES = {
    "short-lists": ([0, 1, 5, 0, 9, 0], [0, 3, T + 1, 2, 1, 0], 8),
    "tile-edges": ([0, T - 1, T, 0, T + 1, 0], [0, T, T + 1, 4, T - 1, 0], 11),
    "stage-edges": ([0, S - 1, S, 0, S + 1, 2 * S + 3, 0], [0, 1, T + 1, 2, 5, 2 * T + 1, 0], 17),
    "k32": ([0, 31, 32, 0, 33, 0], [0, 2, 3, 1, T + 2, 0], 32),
    "all-empty": ([0, 0, 0], [0, 0, 0], 16),
    "empty-clouds": ([0, 0, 0], [1, T + 1, 2], 16),
}


def make(dev, case):
    sizes, qsizes, k = CASES[case]
    rng = np.random.default_rng(len(case))
    co, qo = K.offsets(sizes), K.offsets(qsizes)
    p = rng.uniform(-1, 1, size=(int(co[-1]), 3)).astype(np.float32)
    n = rng.normal(size=(int(co[-1]), 3)).astype(np.float32)
    q = rng.uniform(-1, 1, size=(int(qo[-1]), 3)).astype(np.float32)
    return [K.t(a, dev) for a in (p, n, co, q, qo)] + [k]


def snapshot(args):
    p, n, co, q, qo, k = args
    idx, d2 = C.knn_ragged(p, co, q, qo, k)
    sidx, sd2 = C.knn_ragged(p, co, p, co, k, exclude_self=True)
    nrm, var = C.normals_ragged(p, co, sidx)
    view = torch.ones((p.shape[0], 4), dtype=torch.float32, device=p.device)
    vnrm, vvar = C.normals_ragged(p, co, sidx, view, True)
    sdf, nearest = C.sdf_ragged(p, n, co, q, qo, k, want_nearest=True)
    alone = C.sdf_ragged(p, n, co, q, qo, k)      # nearest = NULL
    return [t.clone() for t in (idx, d2, sidx, sd2, nrm, var, vnrm, vvar, sdf, nearest, alone)]


def check_outputs_and_repeat(dev, case):
    args = make(dev, case)
    plain = snapshot(args)
    with poisoned() as p:
        first = snapshot(args)
        p.renew()
        second = snapshot(args)
        p.check_canaries()
    assert p.count >= 11
    for got in (first, second):
        for t, q in zip(got, plain):
            assert t.shape == q.shape and t.dtype == q.dtype
            if t.dtype.is_floating_point:
                assert not torch.isnan(t).any(), "an output element was not written"
                assert torch.equal(t.contiguous().view(torch.int32), q.contiguous().view(torch.int32))
            else:
                assert torch.equal(t, q)
    idx, d2 = first[0], first[1]
    assert ((idx == -1) == torch.isposinf(d2)).all()
    sizes, qsizes, k = CASES[case]
    co, qo = K.offsets(sizes), K.offsets(qsizes)
    for s in range(len(sizes)):
        rows = idx[int(qo[s]):int(qo[s + 1])]
        assert ((rows >= 0).sum(dim=1) == min(sizes[s], k)).all()      # finite inputs: a list is as long as its cloud allows
        if sizes[s] == 0 and qsizes[s]:
            assert torch.isposinf(first[8][int(qo[s]):int(qo[s + 1])]).all() and (first[9][int(qo[s]):int(qo[s + 1])] == -1).all()
    assert torch.equal(first[8], first[10])


def check_small_after_large(dev):
    """The large call's outputs lie where the small call's will: the small call must not see them."""
    big, small = make(dev, "stage-edges"), make(dev, "short-lists")
    alone = snapshot(small)
    with poisoned() as p:
        snapshot(big)
        after = snapshot(small)
        p.check_canaries()
    for a, c in zip(after, alone):
        if a.dtype == torch.float32:
            a, c = a.contiguous().view(torch.int32), c.contiguous().view(torch.int32)
        assert torch.equal(a, c)
