"""The topology entry points of the twin under poison (tests/topology_poison_bodies.py): every output written in full, nothing stale read."""
import pytest

import topology_poison_bodies as B


@pytest.mark.parametrize("name", B.CASES)
def test_outputs_written_and_repeatable(name):
    B.check_outputs_and_repeat("cpu", name)


def test_emit_respects_its_capacities():
    B.check_capacities("cpu")


def test_small_call_after_a_large_one():
    B.check_small_after_large("cpu")
