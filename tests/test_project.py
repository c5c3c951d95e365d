"""The level-set projection on the C++ twin (bodies: tests/project_forms.py; the same bodies on the GPU: tests/test_gpu_project.py)."""
import pytest

import project_forms as F

DEV = "cpu"


@pytest.mark.parametrize("level", [0.0, 0.02])
@pytest.mark.parametrize("rule", F.RULES)
@pytest.mark.parametrize("weights", ["seeded", "chairs"])
def test_positions(weights, rule, level):
    F.body_positions(DEV, weights, rule, level)


@pytest.mark.parametrize("latent", [1, 29, 128])
def test_latent_sizes(latent):
    F.body_latent_sizes(DEV, latent)


def test_value_is_the_forward():
    F.body_value_is_the_forward(DEV)


def test_independence(monkeypatch):
    F.body_independence(DEV, monkeypatch)


def test_in_place():
    F.body_in_place(DEV)


def test_clipped_steps():
    F.body_clipped_steps(DEV)


def test_zero_gradient():
    F.body_zero_gradient(DEV)


def test_no_side_effects():
    F.body_no_side_effects(DEV)


def test_refusals(monkeypatch):
    F.body_refusals(DEV, monkeypatch)


def test_convergence():
    F.body_convergence(DEV)


def test_refine_meshes():
    F.body_refine_meshes(DEV)


def test_refine_entry_points(tmp_path):
    F.body_refine_entry_points(DEV, tmp_path)


def test_oriented_clouds():
    F.body_oriented_clouds(DEV)


def test_fused_render():
    F.body_fused_render(DEV)
