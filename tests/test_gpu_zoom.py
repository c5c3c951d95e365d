"""GPU tier of the voxel zoom (K20): the kernels of csrc/spline.hip equal the twin bit for bit on every case — coefficients, zoom
outputs of both orders, sample values and gradients, in every kernel form —, and pass the float64 checks of tests/zoom_cases.py
themselves; the Python layer again on the GPU."""
import pytest

import zoom_cases as K

pytestmark = pytest.mark.gpu


def test_prefilter_and_zoom_equal_the_twin_bit_for_bit():
    K.check_bitwise_equal(K.zoom_outputs("cuda"), K.zoom_outputs("cpu"))


def test_sample_equals_the_twin_bit_for_bit():
    K.check_bitwise_equal(K.sample_outputs("cuda"), K.sample_outputs("cpu"))


@pytest.mark.parametrize("shape,size", K.ZOOM_CASES)
def test_zoom_against_float64(shape, size):
    K.check_zoom_against_float64("cuda", shape, size)


@pytest.mark.parametrize("shape", K.SAMPLE_CASES)
def test_sample_against_float64(shape):
    K.check_sample_against_float64("cuda", shape)


def test_interpolation_at_the_nodes():
    K.check_interpolation("cuda")


def test_constant_grids_stay_constant():
    K.check_constant("cuda")


def test_gradient_is_the_derivative_of_the_values():
    K.check_gradient_is_the_derivative("cuda")


def test_faces_are_inside_and_beyond_is_outside():
    K.check_faces_and_outside("cuda")


def test_a_grid_does_not_depend_on_its_batch():
    K.check_batch_independence("cuda")


def test_empty_calls():
    K.check_empty("cuda")


def test_argument_errors():
    K.check_argument_errors("cuda")


def test_input_forms():
    K.check_input_forms("cuda")


def test_marching_cubes_upscale():
    K.check_marching_cubes_upscale("cuda")


def test_render_voxels_upscale():
    K.check_render_voxels_upscale("cuda")


def test_sample_from_voxels_upscale(monkeypatch):
    K.check_sample_from_voxels_upscale("cuda", monkeypatch)
