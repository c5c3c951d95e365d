"""The point-cloud SDF kernels under poison (tests/cloud_poison_bodies.py, the pattern of tests/test_gpu_unwritten.py): every output
written in full — short lists, empty shapes, a NULL `nearest`, ragged last tiles —, no canary changed, a repeat bit-identical."""
import pytest

import cloud_poison_bodies as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sorted(B.CASES))
def test_outputs_written_and_repeatable(case):
    B.check_outputs_and_repeat("cuda", case)


def test_small_call_after_a_large_one():
    B.check_small_after_large("cuda")
