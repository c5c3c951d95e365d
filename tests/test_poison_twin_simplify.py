"""The simplification entry points of the twin under poison (tests/simplify_poison_bodies.py): every output written in full, nothing stale
read."""
import pytest

import simplify_poison_bodies as B


@pytest.mark.parametrize("case", sorted(B.CASES))
def test_outputs_written_and_repeatable(case):
    B.check_outputs_and_repeat("cpu", case)


def test_every_stage_is_written():
    B.check_every_stage_is_written("cpu")


def test_emit_respects_its_capacities():
    B.check_capacities("cpu")


def test_small_call_after_a_large_one():
    B.check_small_after_large("cpu")
