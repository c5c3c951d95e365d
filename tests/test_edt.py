"""Twin tier of the distance transforms (K21): the definition is scipy's (golden file; live scipy when it imports), the C++ twin against
the float64 brute force of tests/edt_reference.py on every case of tests/edt_cases.py, the properties, and the Python layer on CPU
tensors."""
import pytest

import edt_cases as K


def test_reference_equals_the_scipy_golden():
    K.check_reference_equals_golden()


def test_reference_equals_live_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    K.check_reference_equals_live_scipy(ndimage)


def test_distance_transform_equals_the_scipy_golden():
    K.check_distance_transform_equals_golden("cpu")


@pytest.mark.parametrize("name", K.CASES)
def test_against_float64(name):
    K.check_against_float64("cpu", name)


def test_every_form_has_a_case():
    assert set(K.FORMS.values()) == {K.FORM_LDS, K.FORM_GLOBAL} and set(K.FORMS) <= set(K.CASES)
    small, large = K.threshold_shapes()
    assert small[0] + 1 == large[0] and small[1:] == large[1:]


def test_what_the_cases_were_built_for():
    K.check_case_properties("cpu")


def test_a_grid_does_not_depend_on_its_batch():
    K.check_batch_independence("cpu")


def test_crossings_are_the_mesh_vertices():
    K.check_crossings_are_the_mesh_vertices("cpu")


def test_the_sphere_site_error_is_the_recorded_one():
    K.check_sphere_site_error_is_the_recorded_one()


def test_redistance_recovers_a_sphere():
    K.check_redistance_recovers_a_sphere("cpu")


def test_offset_moves_a_sphere():
    K.check_offset_moves_a_sphere("cpu")


def test_occupancy_to_sdf():
    K.check_occupancy_to_sdf("cpu")


def test_hooks_off_change_nothing(monkeypatch):
    K.check_hooks_off_change_nothing("cpu", monkeypatch)


def test_sample_from_voxels_redistance(monkeypatch):
    K.check_sample_from_voxels_redistance("cpu", monkeypatch)


def test_voxel_dataset_occupancy(tmp_path):
    K.check_voxel_dataset_occupancy("cpu", tmp_path)


def test_binvox_round_trip(tmp_path):
    K.check_binvox_round_trip(tmp_path)


def test_input_forms():
    K.check_input_forms("cpu")


def test_empty_calls():
    K.check_empty("cpu")


def test_argument_errors():
    K.check_argument_errors("cpu")


def test_a_short_workspace_is_refused():
    K.check_short_workspace("cpu")
