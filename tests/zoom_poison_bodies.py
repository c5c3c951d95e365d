"""Poison-tier bodies of the voxel-zoom entry points (tests/poison.py): the prefilter, the zoom in both orders and the sampler write
every element of every output, change no canary, and repeat bit for bit.  The entry points take no scratch: the results are their only
stores."""
import numpy as np
import torch

import zoom_cases as K
from poison import poisoned
from shapegan_amd import ops

# (grids S, input shape, output size, points per grid)
CASES = {
    "odd-width": (2, (6, 5, 9), (9, 7, 65), 33),
    "single-output": (2, (4, 3, 5), (1, 1, 1), 5),
    "single-input": (2, (1, 1, 1), (3, 1, 2), 4),
    "middle-constant": (3, (5, 6, 7), (11, 9, 13), 257),
    "lds-forms": (1, (32, 32, 32), (9, 16, 67), 300),
    "global-forms": (1, (40, 32, 32), (8, 8, 7), 300),
    "more-tiles": (2, (4, 4, 30), (19, 17, 133), 10),
}


def make(dev, case):
    S, shape, size, P = CASES[case]
    grids = np.stack([K.noise(len(case) + i, shape) for i in range(S)])
    if case == "middle-constant":
        grids[1] = 0.25
    rng = np.random.default_rng(len(case))
    pts = (rng.uniform(-0.05, 1.05, size=(S, P, 3)) * (np.array(shape) - 1)).astype(np.float32)      # some of them outside
    return K.t(grids, dev), K.t(pts, dev), size


def snapshot(args):
    grids, pts, size = args
    c = ops.spline_prefilter(grids)
    cubic, linear = ops.spline_zoom(c, size, 3), ops.spline_zoom(grids, size, 1)
    values, grad = ops.spline_sample(c, pts, True, 1.0)
    alone = ops.spline_sample(c, pts, False, 1.0)      # gradient = NULL
    return [x.clone() for x in (c, cubic, linear, values, grad, alone)]


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_outputs_and_repeat(dev, case):
    args = make(dev, case)
    plain = snapshot(args)
    with poisoned() as p:
        first = snapshot(args)
        p.renew()
        second = snapshot(args)
        p.check_canaries()
    assert p.count >= 12
    for got in (first, second):
        for x, q in zip(got, plain):
            assert not torch.isnan(x).any(), "an output element was not written"
            assert _same(x, q)
    assert _same(first[3], first[5])
    if case == "middle-constant":
        ulp = float(np.spacing(np.float32(0.25)))
        assert (first[1][1].double() - 0.25).abs().max() <= 4 * ulp and (first[2][1] == 0.25).all()


def check_small_after_large(dev):
    """The large call's outputs lie where the small call's will: the small call must not see them."""
    for large in ("global-forms", "lds-forms"):
        big, small = make(dev, large), make(dev, "single-output")
        alone = snapshot(small)
        with poisoned() as p:
            snapshot(big)
            after = snapshot(small)
            p.check_canaries()
        assert all(_same(a, c) for a, c in zip(after, alone))
