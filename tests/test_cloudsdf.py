"""CPU tier of the point-cloud SDF (K19): the twin against the float64 references of tests/cloud_reference.py, and the Python layer
(shapegan_amd/cloudsdf.py, the cloud options of shapegan_amd.reconstruct) on the twin.  The bodies are tests/cloud_cases.py, which
tests/test_gpu_cloudsdf.py runs on the GPU."""
import pytest

import cloud_cases as K


# ---- k nearest neighbours ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("self_query", [False, True])
@pytest.mark.parametrize("k", K.KS)
def test_knn_lattice_is_the_float64_order_exactly(k, self_query):
    K.check_lattice_exact("cpu", k, self_query)


@pytest.mark.parametrize("self_query", [False, True])
@pytest.mark.parametrize("k", K.KS)
def test_random_reference_alone_has_the_gaps(k, self_query):
    K.check_random_reference_has_gaps(k, self_query)


@pytest.mark.parametrize("self_query", [False, True])
@pytest.mark.parametrize("k", K.KS)
def test_knn_random_against_float64(k, self_query):
    K.check_random_against_float64("cpu", k, self_query)


@pytest.mark.parametrize("k", [8, 17])
def test_a_shape_does_not_depend_on_its_batch(k):
    K.check_batch_independence("cpu", k)


def test_non_finite_coordinates():
    K.run_nonfinite("cpu")


def test_argument_errors():
    K.check_argument_errors("cpu")


def test_constants_come_from_the_header():
    assert (K.MAX_K, K.TILE, K.STAGE) == (32, 256, 1024)


# ---- normals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 8, 16, 32])
def test_normals_against_float64_eigh(k):
    K.check_normals_against_float64("cpu", k)


def test_normal_views():
    K.check_normal_views("cpu")


def test_degenerate_neighbourhoods():
    K.check_degenerate_normals("cpu")


def test_normal_tie_rules():
    K.check_tie_rules("cpu")


def test_normals_are_translation_invariant():
    K.check_translation_invariance("cpu")


# ---- sg_cloud_sdf ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", K.KS)
def test_sdf_is_the_composition_on_the_lattice(k):
    K.check_sdf_lattice_composition("cpu", k)


def test_sdf_tied_vote_and_short_lists():
    K.check_tied_vote("cpu")


def test_sdf_sphere_geometry():
    K.check_sphere_geometry("cpu")


# ---- the Python layer ----------------------------------------------------------------------------------------------------------------------
def test_knn_and_estimate_normals_forms():
    K.check_public_functions("cpu")


def test_voxels_equal_sdf_on_the_grid():
    K.check_voxels_equal_sdf_on_the_grid("cpu")


def test_sample_sdf_near_surface():
    K.check_sample_sdf_near_surface("cpu")


def test_from_scans_of_a_cube():
    K.check_from_scans_cube("cpu")


def test_load_cloud_round_trips(tmp_path):
    K.check_load_cloud_round_trips(tmp_path)


def test_view_is_in_the_files_frame(tmp_path):
    K.check_view_is_in_the_files_frame("cpu", tmp_path)


def test_command_line(tmp_path, chairs_state, capsys):
    K.check_command_line("cpu", tmp_path, chairs_state)
    capsys.readouterr()
