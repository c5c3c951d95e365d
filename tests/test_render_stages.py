"""The stages of the sphere-tracing renderer on the C++ twin, each against the float64 references of tests/geometry_reference.py
(written from include/shapegan_hip.h); tests/test_gpu_render_stages.py runs the same bodies on the MI355X."""
import os

import numpy as np
import pytest
import torch

import geometry_reference as R
from shapegan_amd.model.sdf_net import SDFNet
from shapegan_amd.rendering import raymarching as rm

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DEVICE = "cpu"


@pytest.fixture(scope="module")
def golden_latents():
    return np.load(os.path.join(GOLDEN, "raymarch_chairs.npz"))["latents"]


@pytest.fixture(scope="module")
def net(chairs_state):
    n = SDFNet(device=DEVICE)
    n.load_state_dict(chairs_state)
    return n


# ---- 1. march steps -----------------------------------------------------------------------------------------------------
def body_camera_lockstep(net, state, latents):
    m = R.camera_march(net, latents)
    out = R.lockstep(m, state, 80)
    print("camera lockstep:", out)
    assert out["ray_steps"] > 50000 and out["steps"] == 80
    return out


def body_shadow_lockstep(net, state, latents):
    m = R.shadow_march(net, latents)
    sizes = R.shadow_segment_sizes()
    assert set(R.SHADOW_SIZES) <= set(sizes.tolist()) and sizes.max() > 500 and m.nseg == 256 and m.nshapes == 128
    # (six steps: a ray that oversteps the surface creeps back to it from below with an SDF value that tends to 0, so the fragile
    # share of a shadow march grows with every further step)
    out = R.lockstep(m, state, 6)
    print("shadow lockstep:", out)
    st = R.npy(m.status)
    assert out["lone_segments"] > 0          # segments left with exactly one ray were seen (and checked) on the way
    assert 0 < st.sum() < len(st)            # hits, and rays that left or still march
    assert sum(len(l) for l in m.lists()) > 0
    return out


def body_chunking(net, latents, repeat):
    for make in (R.camera_march, R.shadow_march):
        start = make(net, latents)
        end = R.check_chunking(start, repeat=repeat)
        # (d) the cap: rays remain after 16 steps, and sg_raymarch_finish marks exactly those
        listed, marked = R.check_finish(end)
        assert marked == listed > 0
        early = make(net, latents)
        early.steps(3)
        R.check_finish(early)


def body_get_shadows(net, state, latents):
    z = torch.from_numpy(latents[0]).to(net.device)
    light = np.asarray(rm.light_position, dtype=np.float64)
    assert rm.get_shadows(net, np.zeros((0, 3)), light, z).shape == (0,)
    seen = set()
    # one point: marched at iteration 0 whatever the count; it is lit only if that one step takes it above the radius
    for pts in ([[0.0, 0.0, 0.0]], [[0.05, 0.93, 0.1]], [[0.0, 0.0, 0.0], [0.05, 0.93, 0.1]], [[0.3, -0.4, 0.2], [-0.2, 0.1, 0.4]],
                [[0.1, 0.95, 0.0], [-0.1, 0.96, 0.05]]):
        pts = np.array(pts, dtype=np.float64)
        ref, fragile = R.shadows_reference(state, z, pts.copy(), light, 0.001, -0.045, 1.0)
        assert not fragile, "choose other points: the float64 march passes within rounding of a decision"
        got = rm.get_shadows(net, pts.copy(), light, z, sdf_offset=-0.045)
        assert got.dtype == np.float32 and np.array_equal(got, ref), (pts, got, ref)
        seen |= {(len(pts), float(v)) for v in got}
    assert {(1, 0.0), (1, 1.0)} <= seen and (2, 1.0) in seen
    rng = np.random.RandomState(2)
    pts = rng.uniform(-0.9, 0.9, size=(1000, 3))
    got = rm.get_shadows(net, pts, light, z, sdf_offset=-0.045)
    assert got.shape == (1000,) and got.dtype == np.float32 and set(np.unique(got)) == {0.0, 1.0}


def test_camera_march_lockstep(net, chairs_state, golden_latents):
    body_camera_lockstep(net, chairs_state, golden_latents)


def test_shadow_march_lockstep(net, chairs_state, golden_latents):
    body_shadow_lockstep(net, chairs_state, golden_latents)


def test_march_chunking_and_cap(net, golden_latents):
    body_chunking(net, golden_latents, repeat=False)


def test_get_shadows_small_counts(net, chairs_state, golden_latents):
    body_get_shadows(net, chairs_state, golden_latents)


# ---- 2. camera rays -----------------------------------------------------------------------------------------------------
def body_rays(dev):
    fragile = 0
    for radius, focal_radius in R.RAY_RADII:
        for W, S in R.RAY_CASES:
            out = R.check_rays(dev, W, S, radius, focal_radius)
            fragile += out["fragile"]
            if (radius, focal_radius) == (0.5, 1.6) and W >= 16:
                assert 0 < out["entering"] < W * W // 4      # corner rays (most rays) miss the small sphere
            if (radius, focal_radius) == (1.6, 0.7):
                assert out["entering"] == W * W
    return fragile


def body_too_many_codes(net):
    with pytest.raises(ValueError):
        rm.render_images(net, torch.zeros((129, 128), device=net.device), resolution=4, ssaa=1)


def test_camera_rays():
    body_rays(DEVICE)


def test_render_images_code_limit(net):
    body_too_many_codes(net)


# ---- 3. / 4. hits, ground plane, shadow-ray setup, shading ---------------------------------------------------------------
SCENES = [(1000, 6, True), (1000, 6, False), (50001, 6, True), (255, 1, False), (257, 128, True)]


def body_scene_and_shade(dev, M, S, use_cutoff):
    scene = R.check_scene(dev, M, S, use_cutoff)
    print("scene", M, S, use_cutoff, {k: scene[k] for k in ("H", "G", "fragile", "dir_err", "pos_err")})
    if S >= 5:
        assert scene["H"] > 0 and scene["G"] > 0
    shade = R.check_shade(dev, scene, M, S)
    print("shade", shade)
    return scene, shade


def body_no_hit_ground_is_inf(net, latents):
    # an offset of +1 keeps the SDF positive everywhere: no hit, so the ground plane is the minimum over nothing
    _, stats = rm._render(net, torch.from_numpy(latents[:2]).to(net.device), 8, 0.0005, 1.0, 1000, 1, 1.0, (0.8, 0.1, 0.1), None)
    g = stats["ground"].cpu().numpy()
    assert stats["hits"] == 0 and np.isposinf(g).all(), g


@pytest.mark.parametrize("M,S,use_cutoff", SCENES)
def test_classify_emit_shade(M, S, use_cutoff):
    body_scene_and_shade(DEVICE, M, S, use_cutoff)


def test_ground_without_hits_is_inf(net, golden_latents):
    body_no_hit_ground_is_inf(net, golden_latents)
