"""The simplification kernels under poison (tests/simplify_poison_bodies.py, the pattern of tests/test_gpu_unwritten.py): every output and
every offset written in full, ragged last tiles and empty shapes included, nothing stale read, capacities respected, two runs
bit-identical, a small call after a large one."""
import pytest

import simplify_poison_bodies as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sorted(B.CASES))
def test_outputs_written_and_repeatable(case):
    B.check_outputs_and_repeat("cuda", case)


def test_every_stage_is_written():
    B.check_every_stage_is_written("cuda")


def test_emit_respects_its_capacities():
    B.check_capacities("cuda")


def test_small_call_after_a_large_one():
    B.check_small_after_large("cuda")
