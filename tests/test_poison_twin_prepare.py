"""The mesh-to-SDF entry points of the twin under poison (tests/prepare_poison_bodies.py): every output written in full, nothing stale read."""
import pytest

import prepare_poison_bodies as B


@pytest.mark.parametrize("Q,T", B.FORMS)
def test_outputs_written_and_repeatable(Q, T):
    B.check_outputs_and_repeat("cpu", Q, T)


def test_small_call_after_a_large_one():
    B.check_small_after_large("cpu")


def test_pipeline_writes_everything():
    B.check_pipeline_under_poison("cpu")
