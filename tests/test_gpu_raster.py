"""The rasteriser on the device: every stage output bit-identical to the C++ twin on the same inputs (bins compared as sets: the order
inside a tile's list is the arrival order of an integer atomic and nothing depends on it), the stage checks against
tests/raster_reference.py repeated on device output, a batch rendered twice, and MeshRenderer on a generator's output."""
import numpy as np
import pytest
import torch

import test_raster as E2E
import test_raster_stages as ST
from shapegan_amd.rendering import MeshRenderer, raster

pytestmark = pytest.mark.gpu
DEV = "cuda"


def assert_views_identical(g, c, what):
    for k in ("recs", "flags", "clip", "dropped", "ground", "tile_counts", "tile_offsets", "id", "depth"):
        if c[k] is None:
            assert g[k] is None
            continue
        assert np.array_equal(g[k].view(np.uint8), c[k].view(np.uint8)), "%s: %s differs from the twin" % (what, k)
    assert g["nactive"] == c["nactive"] and np.array_equal(g["active"][:g["nactive"]], c["active"][:c["nactive"]])
    assert ST.bins_as_sets(g) == ST.bins_as_sets(c), what + ": bins"


def test_setup_on_the_device_equals_the_twin():
    g, c = ST.body_setup(DEV), ST.body_setup("cpu")
    for key in c:
        for k in ("recs", "flags", "clip", "dropped", "ground", "tile_counts"):
            assert np.array_equal(g[key][k].view(np.uint8), c[key][k].view(np.uint8)), (key, k)


@pytest.mark.parametrize("width", [48, 40])
@pytest.mark.parametrize("name", ST.CASES)
def test_every_stage_equals_the_twin(name, width):
    _, gl, gc, gi = ST.draw(name, width, DEV)
    _, cl, cc, ci = ST.draw(name, width, "cpu")
    assert_views_identical(gl, cl, name + " light")
    assert_views_identical(gc, cc, name + " camera")
    assert np.array_equal(gi, ci), name + ": image"
    s = torch.from_numpy(ci)
    assert np.array_equal(raster.resolve(s.to(DEV), 2).cpu().numpy(), raster.resolve(s, 2).numpy())


@pytest.mark.parametrize("name", ["noise16", "torus16", "two_spheres16"])
def test_stages_against_the_reference_on_the_device(name):
    ST.body_case(name, 48, DEV)


def test_covering_sets_on_the_device():
    ST.check_single_triangles("quad", 48, DEV, True, ST.CAMERA_VP)
    ST.check_single_triangles("sliver", 40, DEV, True, ST.CAMERA_VP)
    ST.check_single_triangles("offscreen", ST.SHADOW, DEV, False, ST.LIGHT_VP)


def mixed_grids(n, R=32):
    g = torch.Generator().manual_seed(11)
    grids = []
    for i in range(n):
        kind = i % 4
        if kind == 0:
            grids.append(E2E.sphere_grid(R, 0.3 + 0.02 * i))
        elif kind == 1:
            grids.append(torch.rand((R, R, R), generator=g) * 2 - 1)
        elif kind == 2:
            grids.append(torch.ones(R, R, R))                     # no sign change: an empty shape
        else:
            grids.append(E2E.sphere_grid(R, 0.5) + 0.2 * (torch.rand((R, R, R), generator=g) - 0.5))
    return torch.stack(grids)


def test_batch_of_twenty_twice():
    grids = mixed_grids(20).to(DEV)
    v = MeshRenderer(size=96, ssaa=2, shadow_size=128)
    a = v.render_voxels(grids, return_tensor=True).clone()
    b = v.render_voxels(grids, return_tensor=True)
    assert a.shape == (20, 96, 96, 3) and a.dtype == torch.uint8 and a.is_cuda
    assert torch.equal(a, b)
    assert bool((a[2] == a[6]).all()) and bool((a[0] != a[4]).any())          # the empty shapes draw alike, the spheres differ


def test_generator_output_on_the_device_equals_the_twin():
    from shapegan_amd.model.gan import Generator
    torch.manual_seed(3)
    gen = Generator().to(DEV)
    with torch.no_grad():
        sample = gen(torch.randn(2, 128, device=DEV)).squeeze(1)
    assert sample.is_cuda and sample.shape == (2, 32, 32, 32)
    v = MeshRenderer(size=64, ssaa=2, shadow_size=128)
    got = v.render_voxels(sample, return_tensor=True)
    want = v.render_voxels(sample.cpu(), return_tensor=True)
    assert got.is_cuda and not want.is_cuda and torch.equal(got.cpu(), want)
    v.set_voxels(sample[0])
    on_device = v.get_image()
    v.set_voxels(sample[0].cpu())
    assert np.array_equal(on_device, v.get_image())
