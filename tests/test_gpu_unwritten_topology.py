"""The topology kernels under poison (tests/topology_poison_bodies.py, the pattern of tests/test_gpu_unwritten.py): every output written in
full, ragged and empty shapes included, nothing stale read, capacities respected, two runs bit-identical, a small call after a large one."""
import pytest

import topology_poison_bodies as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", B.CASES)
def test_outputs_written_and_repeatable(name):
    B.check_outputs_and_repeat("cuda", name)


def test_emit_respects_its_capacities():
    B.check_capacities("cuda")


def test_small_call_after_a_large_one():
    B.check_small_after_large("cuda")
