"""Meshes to SDF training data on the MI355X (csrc/meshsdf.hip): the bodies of test_prepare.py on the device against the float64
reference, and every output against the C++ twin bit for bit, in every calling form of the distance kernel."""
import numpy as np
import pytest
import torch

from shapegan_amd import prepare as P
import prepare_reference as R
import test_prepare as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(R.MESHES))
def test_distance_matches_float64(name):
    T.check_distance(name, "cuda")


@pytest.mark.parametrize("name", sorted(R.MESHES))
def test_distance_equals_twin_bit_for_bit(name):
    tris, queries, _ = R.distance_case(name)
    T.assert_same_bits(T.run_distance([tris], queries[None], "cuda")[:3], T.run_distance([tris], queries[None], "cpu")[:3], name)


# ---- forms ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", T.FORM_Q)
def test_forms_query_counts(Q):
    T.check_form("cuda", Q, 300)


@pytest.mark.parametrize("T_", T.FORM_T)
def test_forms_triangle_counts(T_):
    T.check_form("cuda", 200, T_)


def test_few_queries_against_many_triangles_split_the_triangles():
    """Q = 5 against T = 3000: 12 LDS chunks.  The host's own choice cuts them into 12 runs; forced factors give the same bits."""
    chunks = (3000 + P.CHUNK - 1) // P.CHUNK
    assert T.check_form("cuda", 5, 3000) == chunks
    for split in (1, 2, 5, 1000):
        assert T.check_form("cuda", 5, 3000, split=split) == min(split, chunks)
    # many queries: no split is needed to fill the device, and none is made
    tris, _ = T.form_case(5, 3000)
    points = np.random.RandomState(1).uniform(-1, 1, (1, 1 << 20, 3)).astype(np.float32)
    assert T.run_distance([tris], points, "cuda", want_closest=False)[3] == 1


def test_empty_middle_shape():
    T.check_empty_middle_shape("cuda")


def test_optional_outputs():
    T.check_optional_outputs("cuda")


def test_points_on_the_triangle():
    T.check_on_the_triangle("cuda")


def test_non_finite_inputs_stay_in_range():
    T.check_non_finite("cuda")


def test_sizes_out_of_range_are_refused():
    T.check_sizes_refused("cuda")


# ---- the sign ------------------------------------------------------------------------------------------------------------------------------
def test_sign_k20_n128():
    T.check_sign("cuda", 20, 128, 0.15)


def test_sign_k50_n256():
    T.check_sign("cuda", 50, 256, 0.10)


def test_sign_equals_twin_bit_for_bit():
    gpu, cpu = T.mesh_scans("cuda", 20, 128), T.mesh_scans("cpu", 20, 128)
    assert torch.equal(gpu.depth.cpu(), cpu.depth)
    points = np.stack([R.sign_case(n)[0] for n in sorted(R.MESHES)])
    a, b = gpu.get_sdf(points), cpu.get_sdf(points)
    assert torch.equal(a.cpu().view(torch.int32), b.view(torch.int32))
    assert torch.equal(gpu.is_outside(points).cpu(), cpu.is_outside(points))


def test_sign_rule_on_a_hand_made_map():
    T.check_sign_rule("cuda")


def test_perspective_view_is_refused():
    T.check_perspective_is_refused("cuda")


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------------
def test_voxels_pass_check_and_axes_are_in_order():
    T.check_voxels("cuda")


def test_near_surface_sampling():
    T.check_near_surface("cuda")


def test_uniform_and_surface_points_and_the_bad_mesh():
    T.check_uniform_and_surface("cuda")


def test_pipeline_equals_twin_bit_for_bit():
    """One seed, one set of query points, the same files' worth of numbers on either device."""
    out = {}
    for dev in ("cuda", "cpu"):
        scans = P.SurfaceScans([R.mesh("torus"), R.mesh("box")], 1.0, T.PIPE_K, T.PIPE_N, device=dev)
        g = torch.Generator().manual_seed(3)
        out[dev] = [t.cpu() for t in scans.sample_sdf_near_surface(1000, generator=g) + scans.get_uniform_and_surface_points(1500, generator=g)]
        out[dev].append(scans.get_voxels(16).cpu())
    for a, b in zip(out["cuda"], out["cpu"]):
        assert a.dtype == b.dtype and torch.equal(a, b)
