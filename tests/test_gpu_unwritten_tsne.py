"""The t-SNE kernels under poison (tests/tsne_poison_bodies.py, the pattern of tests/test_gpu_unwritten.py): P written in full, diagonal
included, grad, kl, beta and plogp written, nothing stale read, two runs bit-identical, a small call after a large one."""
import pytest

import tsne_poison_bodies as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", B.SIZES)
def test_outputs_written_and_repeatable(n):
    B.check_outputs_and_repeat("cuda", n)


def test_small_call_after_a_large_one():
    B.check_small_after_large("cuda")


def test_tsne_writes_everything():
    B.check_tsne_under_poison("cuda")
