"""The auction kernel under poison (tests/emd_poison_bodies.py, the pattern of tests/test_gpu_unwritten.py): every output written in
full, the matching in range, nothing stale read from memory or left in LDS, two runs bit-identical."""
import pytest

import emd_poison_bodies as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("P", B.FORMS)
def test_outputs_written_and_repeatable(P):
    B.check_outputs_and_repeat("cuda", P)


def test_optional_outputs_are_written():
    B.check_raw_outputs("cuda")


def test_second_pair_sees_no_state_of_the_first():
    B.check_second_pair_sees_no_state("cuda")
