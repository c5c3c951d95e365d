"""GPU tier of the distance transforms (K21): the kernels of csrc/edt.hip equal the twin bit for bit on every case — squared distances,
nearest sites, closest crossings, finished distances, in both kernel forms —, and pass the float64 checks of tests/edt_cases.py
themselves; the Python layer again on the GPU."""
import pytest

import edt_cases as K

pytestmark = pytest.mark.gpu


def test_every_output_equals_the_twin_bit_for_bit():
    K.check_bitwise_equal("cuda")


@pytest.mark.parametrize("name", K.CASES)
def test_against_float64(name):
    K.check_against_float64("cuda", name)


def test_distance_transform_equals_the_scipy_golden():
    K.check_distance_transform_equals_golden("cuda")


def test_what_the_cases_were_built_for():
    K.check_case_properties("cuda")


def test_a_grid_does_not_depend_on_its_batch():
    K.check_batch_independence("cuda")


def test_crossings_are_the_mesh_vertices():
    K.check_crossings_are_the_mesh_vertices("cuda")


def test_redistance_recovers_a_sphere():
    K.check_redistance_recovers_a_sphere("cuda")


def test_offset_moves_a_sphere():
    K.check_offset_moves_a_sphere("cuda")


def test_occupancy_to_sdf():
    K.check_occupancy_to_sdf("cuda")


def test_hooks_off_change_nothing(monkeypatch):
    K.check_hooks_off_change_nothing("cuda", monkeypatch)


def test_sample_from_voxels_redistance(monkeypatch):
    K.check_sample_from_voxels_redistance("cuda", monkeypatch)


def test_voxel_dataset_occupancy(tmp_path):
    K.check_voxel_dataset_occupancy("cuda", tmp_path)


def test_input_forms():
    K.check_input_forms("cuda")


def test_empty_calls():
    K.check_empty("cuda")


def test_argument_errors():
    K.check_argument_errors("cuda")


def test_a_short_workspace_is_refused():
    K.check_short_workspace("cuda")
