"""The projection kernel under poison (tests/project_poison_bodies.py, the pattern of tests/test_gpu_unwritten.py): every output written in
full, ragged last tiles included, nothing stale read, two runs bit-identical, a small call after a large one."""
import pytest

import project_poison_bodies as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("iterations,rule", B.FORMS)
def test_outputs_written_and_repeatable(iterations, rule):
    B.check_outputs_and_repeat("cuda", iterations, rule)


def test_small_call_after_a_large_one():
    B.check_small_after_large("cuda")


def test_surface_writes_everything():
    B.check_surface_under_poison("cuda")
