"""Poison-tier bodies of the distance-transform entry points (tests/poison.py): both site sets and the finishing step write every
element of every output — the optional nearest-site outputs included when they are requested —, change no canary, read nothing from the
workspace that the same call did not write, and repeat bit for bit."""
import numpy as np
import torch

import edt_cases as K
from poison import poisoned
from shapegan_amd import ops

# name -> (grids S, shape, spacing); the shapes of both kernel forms come from sg_edt_form
CASES = {
    "one-voxel": (2, (1, 1, 1), 1.0),
    "odd-width": (3, (6, 5, 9), (1.0, 2.0, 0.5)),
    "middle-empty": (3, (5, 6, 7), 1.0),
    "wide": (2, (3, 4, 130), 1.0),
    "lds-form": (2, None, 0.0625),
    "global-form": (2, None, 0.0625),
    "global-flat": (1, (1, 70, 471), 1.0),
}


def shape_of(case):
    small, large = K.threshold_shapes()
    return {"lds-form": small, "global-form": large}.get(case, CASES[case][1])


def make(dev, case):
    S, _, spacing = CASES[case]
    shape = shape_of(case)
    big = int(np.prod(shape)) > 4096
    grids = np.stack([K._blobs(len(case) + i, shape, 3) if big else K.noise(len(case) + i, shape) for i in range(S)])
    if case == "middle-empty":
        grids[1] = 1.0
    return K.t(grids, dev), spacing


def snapshot(args):
    grids, spacing = args
    vsq, idx = ops.edt_voxels(grids, 0.0, True, spacing, nearest=True)
    csq, pos = ops.edt_crossings(grids, 0.0, spacing, closest=True)
    alone_v, alone_c = ops.edt_voxels(grids, 0.0, True, spacing), ops.edt_crossings(grids, 0.0, spacing)      # the optional outputs NULL
    signed, band, root = ops.edt_finish(grids, csq, 0.0), ops.edt_finish(grids, csq, 0.0, 0.1, True), ops.edt_finish(None, vsq)
    return [x.clone() for x in (vsq, idx, csq, pos, alone_v, alone_c, signed, band, root)]


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
    assert p.count >= 18
    for got in (first, second):
        for x, q in zip(got, plain):
            assert _same(x, q)
    vsq, idx, csq, pos, alone_v, alone_c, signed, band, root = first
    assert _same(vsq, alone_v) and _same(csq, alone_c)
    if case == "middle-empty":
        assert torch.isinf(vsq[1]).all() and (idx[1] == -1).all() and torch.isnan(pos[1]).all()
        rest = [0, 2]
    elif case == "one-voxel":      # a single voxel has no edge: no crossing
        assert torch.isinf(csq).all() and torch.isnan(pos).all()
        rest = []
    else:
        rest = list(range(vsq.shape[0]))
    # NaN is the poison: wherever a grid has sites no output holds one; the indices are written (the poison is -1 on the CPU, 0 on
    # the GPU, and only a site that is voxel 0 may be named 0)
    for x in (vsq, alone_v, signed, band, root):
        assert not torch.isnan(x).any(), "an output element was not written"
    for s in rest:
        assert not torch.isnan(pos[s]).any() and not torch.isnan(csq[s]).any() and (idx[s] >= 0).all()
        assert (args[0][s].reshape(-1)[idx[s].reshape(-1).long()] < 0).all()


def check_small_after_large(dev):
    """The large call's outputs and workspace lie where the small call's will: the small call must not see them."""
    for large in ("global-form", "lds-form"):
        big, small = make(dev, large), make(dev, "odd-width")
        alone = snapshot(small)
        with poisoned() as p:
            snapshot(big)
            after = snapshot(small)
            p.check_canaries()
        assert all(_same(a, c) for a, c in zip(after, alone))
    # and with the real, cached workspace: the large call leaves its values in the buffer the small call is handed
    big, small = make(dev, "global-form"), make(dev, "global-flat")
    alone = snapshot(small)
    snapshot(big)
    assert all(_same(a, c) for a, c in zip(snapshot(small), alone))
