"""The distance-transform entry points of the twin under poison (tests/edt_poison_bodies.py): every output written in full, no canary
changed, a repeat bit-identical."""
import pytest

import edt_poison_bodies as B


@pytest.mark.parametrize("case", sorted(B.CASES))
def test_outputs_written_and_repeatable(case):
    B.check_outputs_and_repeat("cpu", case)


def test_small_call_after_a_large_one():
    B.check_small_after_large("cpu")
