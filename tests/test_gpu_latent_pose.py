"""The pose fit on the GPU: csrc/latent_fit.hip (bodies: tests/latent_pose_forms.py; the same bodies on the twin: tests/test_latent_pose.py)."""
import pytest

import latent_pose_forms as F

DEV = "cuda"
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", F.POSES)
@pytest.mark.parametrize("sigma", [0.0, 0.01])
@pytest.mark.parametrize("weights", ["seeded", "chairs"])
def test_positions(weights, sigma, kind):
    F.body_positions(DEV, weights, sigma, kind)


@pytest.mark.parametrize("sigma", [0.0, 0.01])
@pytest.mark.parametrize("latent", [1, 29, 128])
def test_latent_sizes(latent, sigma):
    F.body_latent_sizes(DEV, latent, sigma)


@pytest.mark.parametrize("window", [(0, 0), (190, 64)])
def test_identity_pose_is_the_latent_fit(window):
    F.body_identity_bits(DEV, window)


def test_independence():
    F.body_independence(DEV)


@pytest.mark.parametrize("window", F.WINDOWS)
def test_windows(window):
    F.body_windows(DEV, window)


def test_chunking(monkeypatch):
    F.body_chunking(DEV, monkeypatch)


def test_exact_zero():
    F.body_exact_zero(DEV)


def test_entry_point_refusals():
    F.body_entry_refusals(DEV)


def test_python_refusals(monkeypatch):
    F.body_python_refusals(DEV, monkeypatch)


def test_fit():
    F.body_fit(DEV)


@pytest.mark.parametrize("pose", ["translation", "translation+scale", "rigid", "similarity"])
def test_frozen_groups(pose):
    F.body_frozen_groups(DEV, pose)


def test_recovery():
    F.body_recovery(DEV)


def test_rotation_starts():
    F.body_rotation_starts(DEV)


def test_meshes():
    F.body_meshes(DEV)


def test_cli(tmp_path, capsys):
    F.body_cli(tmp_path, capsys)
