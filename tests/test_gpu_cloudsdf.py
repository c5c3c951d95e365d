"""GPU tier of the point-cloud SDF (K19): the kernels of csrc/cloud.hip equal the twin bit for bit on every case, and pass the float64
checks of tests/cloud_cases.py themselves; the Python layer again on the GPU."""
import pytest

import cloud_cases as K

pytestmark = pytest.mark.gpu


def test_knn_equals_the_twin_bit_for_bit():
    K.check_bitwise_equal(K.knn_outputs("cuda"), K.knn_outputs("cpu"))


def test_knn_non_finite_equals_the_twin():
    K.check_bitwise_equal(K.run_nonfinite("cuda"), K.run_nonfinite("cpu"))


def test_normals_equal_the_twin_bit_for_bit():
    K.check_bitwise_equal(K.normal_outputs("cuda"), K.normal_outputs("cpu"))


def test_sdf_equals_the_twin_bit_for_bit():
    K.check_bitwise_equal(K.sdf_outputs("cuda"), K.sdf_outputs("cpu"))


@pytest.mark.parametrize("self_query", [False, True])
@pytest.mark.parametrize("k", K.KS)
def test_knn_lattice_is_the_float64_order_exactly(k, self_query):
    K.check_lattice_exact("cuda", k, self_query)


@pytest.mark.parametrize("self_query", [False, True])
@pytest.mark.parametrize("k", K.KS)
def test_knn_random_against_float64(k, self_query):
    K.check_random_against_float64("cuda", k, self_query)


@pytest.mark.parametrize("k", [8, 17])
def test_a_shape_does_not_depend_on_its_batch(k):
    K.check_batch_independence("cuda", k)


def test_argument_errors():
    K.check_argument_errors("cuda")


@pytest.mark.parametrize("k", [3, 8, 16, 32])
def test_normals_against_float64_eigh(k):
    K.check_normals_against_float64("cuda", k)


def test_normal_views():
    K.check_normal_views("cuda")


def test_degenerate_neighbourhoods():
    K.check_degenerate_normals("cuda")


def test_normal_tie_rules():
    K.check_tie_rules("cuda")


def test_normals_are_translation_invariant():
    K.check_translation_invariance("cuda")


@pytest.mark.parametrize("k", K.KS)
def test_sdf_is_the_composition_on_the_lattice(k):
    K.check_sdf_lattice_composition("cuda", k)


def test_sdf_tied_vote_and_short_lists():
    K.check_tied_vote("cuda")


def test_sdf_sphere_geometry():
    K.check_sphere_geometry("cuda")


def test_knn_and_estimate_normals_forms():
    K.check_public_functions("cuda")


def test_voxels_equal_sdf_on_the_grid():
    K.check_voxels_equal_sdf_on_the_grid("cuda")


def test_sample_sdf_near_surface():
    K.check_sample_sdf_near_surface("cuda")


def test_from_scans_of_a_cube():
    K.check_from_scans_cube("cuda")


def test_view_is_in_the_files_frame(tmp_path):
    K.check_view_is_in_the_files_frame("cuda", tmp_path)


def test_command_line(tmp_path, chairs_state, capsys):
    K.check_command_line("cuda", tmp_path, chairs_state)
    capsys.readouterr()
