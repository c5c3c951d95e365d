"""The pose-fit entry points of the twin under poison (tests/latent_pose_poison_bodies.py): every output written in full, nothing stale read."""
import pytest

import latent_pose_poison_bodies as B


@pytest.mark.parametrize("window,sigma", B.FORMS)
def test_outputs_written_and_repeatable(window, sigma):
    B.check_outputs_and_repeat("cpu", window, sigma)


def test_every_row_written_in_full():
    B.check_raw_rows("cpu")


def test_small_call_after_a_large_one():
    B.check_small_after_large("cpu")


def test_fit_writes_everything():
    B.check_fit_under_poison("cpu")
