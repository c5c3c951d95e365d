"""The earth mover's distance of the twin under poison (tests/emd_poison_bodies.py): every output written in full, nothing stale read."""
import pytest

import emd_poison_bodies as B


@pytest.mark.parametrize("P", B.FORMS)
def test_outputs_written_and_repeatable(P):
    B.check_outputs_and_repeat("cpu", P)


def test_optional_outputs_are_written():
    B.check_raw_outputs("cpu")


def test_second_pair_sees_no_state_of_the_first():
    B.check_second_pair_sees_no_state("cpu")
