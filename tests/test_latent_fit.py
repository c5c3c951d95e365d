"""The latent fit on the C++ twin (bodies: tests/latent_fit_forms.py; the same bodies on the GPU: tests/test_gpu_latent_fit.py)."""
import pytest

import latent_fit_forms as F

DEV = "cpu"


@pytest.mark.parametrize("sigma", [0.0, 0.01])
@pytest.mark.parametrize("weights", ["seeded", "chairs"])
def test_positions(weights, sigma):
    F.body_positions(DEV, weights, sigma)


@pytest.mark.parametrize("latent", [1, 29, 30, 128])
def test_latent_sizes(latent):
    F.body_latent_sizes(DEV, latent)


def test_independence():
    F.body_independence(DEV)


@pytest.mark.parametrize("window", F.WINDOWS)
def test_windows(window):
    F.body_windows(DEV, window)


def test_exact_zero():
    F.body_exact_zero(DEV)


def test_composed_path():
    F.body_composed(DEV)


def test_chunking(monkeypatch):
    F.body_chunking(DEV, monkeypatch)


def test_refusals(monkeypatch):
    F.body_refusals(DEV, monkeypatch)


def test_fit():
    F.body_fit(DEV)


def test_fit_composed():
    F.body_fit(DEV, fused=False)


def test_fit_windows():
    F.body_fit_windows(DEV)


def test_meshes():
    F.body_meshes(DEV)


def test_cli(tmp_path, capsys):
    F.body_cli(tmp_path, capsys)
