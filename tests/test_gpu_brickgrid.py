"""The narrow-band voxel grid on the MI355X (bodies: tests/brickgrid_forms.py; the rule restated: tests/brickgrid_reference.py)."""
import pytest

import brickgrid_forms as F
import brickgrid_net_forms as N

DEV = "cuda"
pytestmark = pytest.mark.gpu
ROD = [(32, 8), (32, 4), (24, 4), (16, 4)]


@pytest.mark.parametrize("R,B,S", F.combos())
@pytest.mark.parametrize("name", ["sphere", "torus", "no_crossing"])
def test_field_matches_restatement_and_dense_mesh(name, R, B, S):
    F.check_field(name, DEV, R, B, S)


@pytest.mark.parametrize("R,B,S", F.combos(min_bricks_per_axis=4))
def test_two_spheres_in_non_adjacent_bricks(R, B, S):
    res, _ = F.check_field("two_spheres", DEV, R, B, S)
    assert res.stats["evaluated_points"][0] < R ** 3


@pytest.mark.parametrize("pad", [True, False])
@pytest.mark.parametrize("R,B,S", F.combos())
def test_slab_crossing_the_border(R, B, S, pad):
    F.check_field("slab", DEV, R, B, S, pad=pad)


@pytest.mark.parametrize("R,B,S", F.combos())
def test_mask_makes_the_crossing(R, B, S):
    _, mesh = F.check_field("big_sphere", DEV, R, B, S, masked=True)
    assert mesh.faces.shape[0] > 0


@pytest.mark.parametrize("level", [0.04, -0.1])
@pytest.mark.parametrize("R,B,S", F.combos())
def test_level_other_than_zero(R, B, S, level):
    F.check_field("sphere", DEV, R, B, S, level=level)


@pytest.mark.parametrize("R,B,S", [(16, 4, 3), (32, 8, 1)])
def test_band_zero(R, B, S):
    F.check_field("torus", DEV, R, B, S, band=0.0)


@pytest.mark.parametrize("R,B", ROD)
def test_rod_is_followed_by_continuation(R, B):
    F.check_rod(DEV, R, B)


def test_floater_is_the_allowed_difference():
    F.check_floater(DEV)


def test_refusals_before_any_launch():
    F.check_refusals(DEV)


def test_bit_identical_repeats():
    F.check_determinism(DEV)


# ---- with the network ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,B,sphere_only,level", N.CASES)
def test_network_grid_and_mesh_equal_dense(R, B, sphere_only, level):
    N.check_case(DEV, R, B, sphere_only, level)


def test_get_mesh_narrow_band_equals_dense_with_fewer_points():
    N.check_get_mesh(DEV)


def test_sample_point_clouds_narrow_band_equals_dense_with_fewer_points():
    N.check_sample_point_clouds(DEV)


def test_traversal_frames_narrow_band_equal_dense_with_fewer_points():
    N.check_traversal_frames(DEV)


def test_reconstruct_meshes_narrow_band_equals_dense_with_fewer_points():
    N.check_reconstruct_meshes(DEV)


def test_a_point_has_the_same_bits_wherever_it_stands_in_a_launch():
    N.check_position_independence(DEV)
