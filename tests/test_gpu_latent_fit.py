"""The latent fit on the GPU: csrc/latent_fit.hip through SDFNet.latent_loss_and_grad and shapegan_amd/reconstruct.py (bodies:
tests/latent_fit_forms.py; the same bodies on the twin: tests/test_latent_fit.py)."""
import pytest

import latent_fit_forms as F

DEV = "cuda"
pytestmark = pytest.mark.gpu


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


def test_voxel_grid_cache_follows_the_device():
    """SDFNet keeps one sample grid per resolution: a network on the CPU asking after one on the GPU (the command line with --device
    cpu next to GPU work) gets a grid on its own device, and both give get_mesh's values."""
    import torch
    sd = F.chairs_state()
    z = torch.zeros(1, 128)
    on_gpu = F.net_on("cuda", 5, 128, sd).voxel_grids(z.cuda(), 12)
    on_cpu = F.net_on("cpu", 5, 128, sd).voxel_grids(z, 12)
    again = F.net_on("cuda", 5, 128, sd).voxel_grids(z.cuda(), 12)
    assert on_gpu.is_cuda and not on_cpu.is_cuda and again.is_cuda
    assert torch.equal(on_gpu, again)
    torch.testing.assert_close(on_gpu.cpu(), on_cpu, rtol=1e-4, atol=2e-6)
