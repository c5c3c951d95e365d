"""The projection entry point of the twin under poison (tests/project_poison_bodies.py): every output written in full, nothing stale read."""
import pytest

import project_poison_bodies as B


@pytest.mark.parametrize("iterations,rule", B.FORMS)
def test_outputs_written_and_repeatable(iterations, rule):
    B.check_outputs_and_repeat("cpu", iterations, rule)


def test_small_call_after_a_large_one():
    B.check_small_after_large("cpu")


def test_surface_writes_everything():
    B.check_surface_under_poison("cpu")
