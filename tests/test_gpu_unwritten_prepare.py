"""The mesh-to-SDF kernels under poison (tests/prepare_poison_bodies.py, the pattern of tests/test_gpu_unwritten.py): every output written
in full, indices in range, nothing stale read from the workspace, two runs bit-identical."""
import pytest

import prepare_poison_bodies as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("Q,T", B.FORMS)
def test_outputs_written_and_repeatable(Q, T):
    B.check_outputs_and_repeat("cuda", Q, T)


def test_small_call_after_a_large_one():
    B.check_small_after_large("cuda")


def test_pipeline_writes_everything():
    B.check_pipeline_under_poison("cuda")
