"""GPU tier: the fused optimizers and the elementwise kernels in every calling form against float64 (bodies, case tables, bounds:
tests/optim_forms.py; the float64 formulas themselves are held against torch.optim by tests/test_optim_forms_host.py)."""
import pytest

import optim_forms as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", O.ALL_N)
def test_adam_forms(n):
    O.body_adam(n)


@pytest.mark.parametrize("n", O.ALL_N)
def test_rmsprop_forms(n):
    O.body_rmsprop(n)


@pytest.mark.parametrize("kind", O.NONFINITE)
def test_optimizers_nan_inf_and_overflowing_gradients(kind):
    O.body_nonfinite(kind)


@pytest.mark.parametrize("preset", O.COUNTER_PRESETS)
def test_adam_device_counter(preset):
    O.body_dev_counter(preset)


@pytest.mark.parametrize("case_id", sorted(O.MULTI))
def test_adam_multi_forms(case_id):
    O.body_multi(case_id)


def test_adam_multi_refusals_write_nothing():
    O.body_multi_refusals()


def test_adam_guard_word():
    O.body_guard()


@pytest.mark.parametrize("n", O.CLAMP_N)
def test_clamp_forms(n):
    O.body_clamp(n)


@pytest.mark.parametrize("ntensors", O.CLAMP_MULTI)
def test_clamp_multi_forms(ntensors):
    O.body_clamp_multi(ntensors)


def test_clip_keeps_a_nan_weight():
    O.body_clip_nan()


@pytest.mark.parametrize("n", O.REDUCE_N)
def test_reduce_sum_forms(n):
    O.body_reduce(n)


@pytest.mark.parametrize("n", O.ACT_N)
def test_activation_forms(n):
    O.body_act(n)


@pytest.mark.parametrize("S", O.ROWSUM_S)
def test_activation_backward_rowsum_forms(S):
    O.body_act_rowsum(S)


@pytest.mark.parametrize("L", O.ROWS_L)
def test_gather_scatter_rows_forms(L):
    O.body_rows(L)


@pytest.mark.parametrize("n", O.AXPBY_N)
def test_axpby_forms(n):
    O.body_axpby(n)
