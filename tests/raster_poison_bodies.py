"""Shared by tests/test_poison_twin_raster.py (C++ twin) and tests/test_gpu_unwritten_raster.py (HIP kernels): the rasteriser's stages
under tests/poison.py.  Every output and every piece of integer scratch of rendering/raster.py comes from `torch.empty`, so under
poison each starts as NaN (floats), -1 (integers on the CPU) or zero (integers on the GPU) between canary bands.

  bodies   the stage checks of tests/test_raster_stages.py (setup, bins, visibility, shadow pass, shade) run unchanged under poison
           with the bands intact afterwards;
  outputs  no NaN in any float output; the integer outputs (flags, dropped counts, tile counts, offsets, non-empty tiles, ids, image)
           equal the unpoisoned run exactly, the lists as sets;
  twice    the same form again with the poison renewed and the first run's blocks overwritten: bit-identical.
Nothing here accumulates floats atomically: no exemptions."""
import numpy as np
import torch

import test_raster_stages as ST
from poison import poisoned, run_poisoned
from shapegan_amd.rendering import MeshRenderer

FORMS = [("sliver", 40), ("torus16", 48), ("noise16", 40)]
FLOAT_KEYS = ("clip", "ground", "depth")
EXACT_KEYS = ("recs", "flags", "clip", "dropped", "ground", "tile_counts", "tile_offsets", "id", "depth")


def snapshot(device, name, width):
    _, light, cam, image = ST.draw(name, width, device)
    return light, cam, image


def same(a, b, what):
    for k in EXACT_KEYS:
        if b[k] is None:
            assert a[k] is None
        else:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), "%s: %s" % (what, k)
    assert a["nactive"] == b["nactive"] and np.array_equal(a["active"][:a["nactive"]], b["active"][:b["nactive"]]), what
    assert ST.bins_as_sets(a) == ST.bins_as_sets(b), what + ": bins"


def check_bodies(device):
    run_poisoned(ST.body_setup, device)
    for name, width in FORMS:
        run_poisoned(ST.body_case, name, width, device)
    run_poisoned(ST.check_single_triangles, "quad", 48, device, True, ST.CAMERA_VP)


def check_outputs_and_repeat(device, name, width):
    plain = snapshot(device, name, width)
    with poisoned() as p:
        first = snapshot(device, name, width)          # (numpy copies: renew() may scribble over the tensors)
        p.renew()
        second = snapshot(device, name, width)
        p.check_canaries()
    for view in first[:2]:
        for k in FLOAT_KEYS:
            if view[k] is not None:
                assert not np.isnan(view[k]).any(), "%s: NaN left in %s" % (name, k)
    for got in (first, second):
        same(got[0], plain[0], name + " light")
        same(got[1], plain[1], name + " camera")
        assert np.array_equal(got[2], plain[2]), name + ": image"


def check_renderer(device):
    grids = torch.stack([ST.sdf_grid("sphere"), torch.ones(16, 16, 16), ST.sdf_grid("noise")]).to(device)
    v = MeshRenderer(size=40, ssaa=2, shadow_size=64)
    plain = v.render_voxels(grids, return_tensor=True).cpu()
    with poisoned() as p:
        first = v.render_voxels(grids, return_tensor=True).cpu().clone()
        p.renew()
        second = v.render_voxels(grids, return_tensor=True).cpu().clone()
        p.check_canaries()
    assert torch.equal(first, plain) and torch.equal(second, plain)
