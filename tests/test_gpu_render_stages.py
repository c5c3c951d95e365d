"""The stages of csrc/raymarch.hip on the MI355X, each entry point on its own, against the float64 references of
tests/geometry_reference.py: the bodies of tests/test_render_stages.py on GPU tensors."""
import numpy as np
import pytest

import test_render_stages as T
from shapegan_amd.model.sdf_net import SDFNet

pytestmark = pytest.mark.gpu

golden_latents = T.golden_latents


@pytest.fixture(scope="module")
def net(chairs_state):
    n = SDFNet(device="cuda")
    n.load_state_dict(chairs_state)
    return n


def test_gpu_camera_march_lockstep(net, chairs_state, golden_latents):
    T.body_camera_lockstep(net, chairs_state, golden_latents)


def test_gpu_shadow_march_lockstep(net, chairs_state, golden_latents):
    T.body_shadow_lockstep(net, chairs_state, golden_latents)


def test_gpu_march_chunking_and_cap(net, golden_latents):
    T.body_chunking(net, golden_latents, repeat=True)


def test_gpu_get_shadows_small_counts(net, chairs_state, golden_latents):
    T.body_get_shadows(net, chairs_state, golden_latents)


def test_gpu_camera_rays():
    T.body_rays("cuda")


def test_gpu_render_images_code_limit(net):
    T.body_too_many_codes(net)


@pytest.mark.parametrize("M,S,use_cutoff", T.SCENES)
def test_gpu_classify_emit_shade(M, S, use_cutoff):
    T.body_scene_and_shade("cuda", M, S, use_cutoff)


def test_gpu_ground_without_hits_is_inf(net, golden_latents):
    T.body_no_hit_ground_is_inf(net, golden_latents)
