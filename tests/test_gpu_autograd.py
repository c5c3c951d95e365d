"""GPU tier of the autograd-layer table (tests/autograd_cases.py): every Function of shapegan_amd/ops.py whose backward chooses
between kernels, for every subset of differentiable inputs, in first order (stock engine and lib.backward into the flat gradient
slices), second order and three layouts of the incoming gradient, against float64 autograd; with the expected raw entries asserted
from the host side.  tests/test_cpu_twin.py runs the same bodies on the twin."""
import pytest

import autograd_cases as AG

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,order,layout", AG.PARAMS)
def test_autograd_table(name, order, layout, monkeypatch):
    AG.body(name, order, layout, monkeypatch)


def test_sample_packed_converts_float64_vertices_and_strided_faces():
    AG.body_sample_packed_inputs()


def test_once_differentiable_losses_raise_at_second_order():
    AG.body_once_differentiable_losses_raise()
