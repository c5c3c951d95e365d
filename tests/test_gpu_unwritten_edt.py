"""The distance-transform kernels under poison (tests/edt_poison_bodies.py, the pattern of tests/test_gpu_unwritten.py): every output
written in full — odd widths, single voxels, a grid without sites, NULL optional outputs, both kernel forms —, no canary changed, no
stale workspace read, a repeat bit-identical."""
import pytest

import edt_poison_bodies as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sorted(B.CASES))
def test_outputs_written_and_repeatable(case):
    B.check_outputs_and_repeat("cuda", case)


def test_small_call_after_a_large_one():
    B.check_small_after_large("cuda")
