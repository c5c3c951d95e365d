"""The pose-fit kernels under poison (tests/latent_pose_poison_bodies.py, the pattern of tests/test_gpu_unwritten.py): every output written
in full, ragged last tiles and table rows that name nothing included, nothing stale read, two runs bit-identical, a small call after a
large one."""
import pytest

import latent_pose_poison_bodies as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("window,sigma", B.FORMS)
def test_outputs_written_and_repeatable(window, sigma):
    B.check_outputs_and_repeat("cuda", window, sigma)


def test_every_row_written_in_full():
    B.check_raw_rows("cuda")


def test_small_call_after_a_large_one():
    B.check_small_after_large("cuda")


def test_fit_writes_everything():
    B.check_fit_under_poison("cuda")
