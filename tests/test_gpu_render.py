"""Sphere-traced renders on the GPU (csrc/raymarch.hip): against the C++ twin, the reference golden, themselves and batches."""
import os

import numpy as np
import pytest
import torch

from shapegan_amd.model.sdf_net import SDFNet
from shapegan_amd.rendering import raymarching as rm
from shapegan_amd.util import crop_image

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SETTINGS = dict(radius=1.6, sdf_offset=-0.045, vertical_cutoff=1)
COLOR = (0.8, 0.1, 0.1)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "raymarch_chairs.npz"))


@pytest.fixture(scope="module")
def nets(chairs_state):
    g = SDFNet(device="cuda")
    g.load_state_dict(chairs_state)
    c = SDFNet(device="cpu")
    c.load_state_dict(chairs_state)
    return g, c


def render(net, z, res, ssaa, **kw):
    args = dict(threshold=0.0005, sdf_offset=0.0, iterations=1000, radius=1.0, vertical_cutoff=None)
    args.update(kw)
    return rm._render(net, z, res, args["threshold"], args["sdf_offset"], args["iterations"], ssaa, args["radius"], COLOR,
                      args["vertical_cutoff"])


def test_gpu_matches_twin(nets, golden):
    g, c = nets
    z = torch.from_numpy(golden["latents"])
    _, sg = render(g, z.cuda(), 32, 2, **SETTINGS)
    _, sc = render(c, z, 32, 2, **SETTINGS)
    mg, mc = sg["status"].cpu().bool(), sc["status"].bool()
    assert (mg == mc).float().mean().item() >= 0.999
    both = mg & mc
    err = (sg["pos"].cpu()[both] - sc["pos"][both]).abs().max().item()
    assert err <= 1e-4, err


@pytest.mark.parametrize("ssaa", [1, 2])
def test_gpu_matches_reference(nets, golden, ssaa):
    g, _ = nets
    for i in range(2):
        img = rm.render_image(g, torch.from_numpy(golden["latents"][i]).cuda(), resolution=32, ssaa=ssaa, **SETTINGS)
        d = np.abs(np.asarray(img).astype(np.int32) - golden["image_ssaa%d_%d" % (ssaa, i)].astype(np.int32))
        assert (d.max(axis=-1) > 8).mean() <= 0.01 and d.mean() <= 1.5, ((d.max(axis=-1) > 8).mean(), d.mean())
    img = rm.render_image(g, torch.from_numpy(golden["latents"][0]).cuda(), resolution=32)
    d = np.abs(np.asarray(img).astype(np.int32) - golden["image_default_0"].astype(np.int32))
    assert (d.max(axis=-1) > 8).mean() <= 0.01 and d.mean() <= 1.5


def test_gpu_deterministic(nets, golden):
    g, _ = nets
    z = torch.from_numpy(golden["latents"]).cuda()
    a_img, a = render(g, z, 64, 2, **SETTINGS)
    b_img, b = render(g, z, 64, 2, **SETTINGS)
    assert torch.equal(a_img, b_img)
    assert torch.equal(a["hit_pos"], b["hit_pos"]) and torch.equal(a["shadows"], b["shadows"])
    assert (a["iterations"], a["shadow_iterations"], a["evaluations"]) == (b["iterations"], b["shadow_iterations"], b["evaluations"])


def test_gpu_batch_equals_singles(nets, golden):
    g, _ = nets
    z = (torch.randn(5, 128, generator=torch.Generator().manual_seed(41)) * 0.5).cuda()
    z[4] = torch.from_numpy(golden["latents"][0]).cuda()
    kw = dict(resolution=48, ssaa=1, return_tensor=True, **SETTINGS)
    batch, sb = render(g, z, 48, 1, **SETTINGS)
    for i in range(5):
        single, ss = render(g, z[i:i + 1], 48, 1, **SETTINGS)
        assert torch.equal(batch[i], single[0]), i
        o = sb["hit_offsets"]
        assert torch.equal(sb["hit_pos"][o[i]:o[i + 1]], ss["hit_pos"]), i
    assert torch.equal(rm.render_images(g, z, **kw), batch)
    # a tight iteration cap leaves rays of every image active: the "< 2 rays" rule and the cap apply image by image
    capped, _ = render(g, z, 48, 1, iterations=20, **SETTINGS)
    for i in range(5):
        assert torch.equal(capped[i], render(g, z[i:i + 1], 48, 1, iterations=20, **SETTINGS)[0][0]), i


def test_gpu_options(nets, golden):
    g, _ = nets
    z = torch.from_numpy(golden["latents"][0]).cuda()
    plain, sp = render(g, z, 32, 1)
    offset, so = render(g, z, 32, 1, sdf_offset=-0.045)
    assert so["hits"] > sp["hits"]            # a negative offset grows the shape
    cut, sc = render(g, z, 32, 1, vertical_cutoff=0.2)
    assert sc["hits"] < sp["hits"]
    assert (sc["hit_pos"][:, 1].abs() <= 0.2).all()
    empty, se = render(g, z, 16, 1, sdf_offset=1.0)
    assert se["hits"] == 0 and bool((empty == 255).all())


def test_gpu_full_resolution(nets, golden):
    g, _ = nets
    z = torch.from_numpy(golden["latents"][0]).cuda()
    image, stats = render(g, z, 800, 2, **SETTINGS)
    assert image.shape == (1, 1600, 1600, 3) and stats["hits"] > 0
    img = rm.render_image(g, z, **SETTINGS, crop=True)
    assert img.size == (800, 800)
    assert crop_image(image[0].cpu().numpy(), background=255).shape[0] < 1600   # the crop applies at this size
