"""Twin tier of the voxel zoom (K20): the definition is scipy's (golden file; live scipy when it imports), the C++ twin against the
float64 restatement of tests/zoom_reference.py on every case of tests/zoom_cases.py, the properties, and the Python layer on CPU tensors."""
import pytest

import zoom_cases as K


def test_reference_equals_the_scipy_golden():
    K.check_reference_equals_golden()


def test_reference_equals_live_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    K.check_reference_equals_live_scipy(ndimage)


def test_the_tolerance_is_the_measured_one():
    """zoom_reference in float32 against itself in float64 stays within the constants the tolerance is made of."""
    value, sample_value, gradient = K.measure_float32_reference()
    print("float32 reference: zoom %.3g, sample value %.3g, sample gradient %.3g" % (value, sample_value, gradient))
    assert max(value, sample_value) <= K.F32_VALUE_ERROR and gradient <= K.F32_GRADIENT_ERROR
    assert max(value, sample_value) >= K.F32_VALUE_ERROR / 2 and gradient >= K.F32_GRADIENT_ERROR / 2      # and they are not loose


@pytest.mark.parametrize("shape,size", K.ZOOM_CASES)
def test_zoom_against_float64(shape, size):
    K.check_zoom_against_float64("cpu", shape, size)


def test_every_form_has_a_case():
    forms = set(K.FORMS.values())
    assert {f[0] for f in forms} == {K.FORM_LDS, K.FORM_GLOBAL} and {f[1] for f in forms} == {K.FORM_LDS, K.FORM_GLOBAL}
    assert set(K.FORMS) <= set(K.ZOOM_CASES)


@pytest.mark.parametrize("shape", K.SAMPLE_CASES)
def test_sample_against_float64(shape):
    K.check_sample_against_float64("cpu", shape)


def test_interpolation_at_the_nodes():
    K.check_interpolation("cpu")


def test_constant_grids_stay_constant():
    K.check_constant("cpu")


def test_gradient_is_the_derivative_of_the_values():
    K.check_gradient_is_the_derivative("cpu")


def test_faces_are_inside_and_beyond_is_outside():
    K.check_faces_and_outside("cpu")


def test_a_grid_does_not_depend_on_its_batch():
    K.check_batch_independence("cpu")


def test_empty_calls():
    K.check_empty("cpu")


def test_argument_errors():
    K.check_argument_errors("cpu")


def test_input_forms():
    K.check_input_forms("cpu")


def test_marching_cubes_upscale():
    K.check_marching_cubes_upscale("cpu")


def test_render_voxels_upscale():
    K.check_render_voxels_upscale("cpu")


def test_sample_from_voxels_upscale(monkeypatch):
    K.check_sample_from_voxels_upscale("cpu", monkeypatch)
