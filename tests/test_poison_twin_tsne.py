"""The t-SNE entry points of the twin under poison (tests/tsne_poison_bodies.py): every output written in full, nothing stale read."""
import pytest

import tsne_poison_bodies as B


@pytest.mark.parametrize("n", B.SIZES)
def test_outputs_written_and_repeatable(n):
    B.check_outputs_and_repeat("cpu", n)


def test_small_call_after_a_large_one():
    B.check_small_after_large("cpu")


def test_tsne_writes_everything():
    B.check_tsne_under_poison("cpu")
