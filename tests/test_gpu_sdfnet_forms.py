"""GPU tier: the fused SDFNet MLP (csrc/sdfnet.hip, csrc/sdfnet_tile.h, ops.SDFNetPoints / ops.SDFNetShapes) in every calling
form against float64 — which inputs require grad, ragged segments by position, more shapes than the one-launch fold takes, the
three ways the fold is made, the ABI arguments no shell passes, latent sizes at the padding edges, one grid shared by several
shapes.  Bodies, references and the criterion: tests/sdfnet_forms.py (re-run on the twin by tests/test_cpu_twin.py)."""
import pytest

import sdfnet_forms as FORMS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("need_p,need_z,need_w", FORMS.SUBSETS)
@pytest.mark.parametrize("mode", FORMS.MODES)
def test_which_grads(mode, need_p, need_z, need_w):
    FORMS.body_which_grads(mode, need_p, need_z, need_w)


@pytest.mark.parametrize("with_reg", [True, False])
def test_segments_by_position(with_reg):
    FORMS.body_segments_dense(with_reg)


@pytest.mark.parametrize("where", sorted(FORMS.ONE_HOT_POSITIONS))
def test_segments_one_hot(where):
    FORMS.body_segments_one_hot(where)


@pytest.mark.parametrize("kind", sorted(FORMS.DEGENERATE))
def test_segments_degenerate_tables(kind):
    FORMS.body_segments_degenerate(kind)


@pytest.mark.parametrize("S,reg,z_only", FORMS.FOLD_CASES)
def test_beyond_the_one_launch_fold(S, reg, z_only):
    FORMS.body_beyond_fold(S, reg, z_only)


def test_fold_forms():
    FORMS.body_fold_forms()


@pytest.mark.parametrize("train", [False, True])
def test_raw_abi_latent_idx_and_points_period(train):
    FORMS.body_raw_abi(train)


@pytest.mark.parametrize("latent", FORMS.EDGE_LATENTS)
@pytest.mark.parametrize("mode", ["points", "ragged"])
def test_latent_sizes_at_the_padding_edges(mode, latent):
    FORMS.body_latent_size(mode, latent)


@pytest.mark.parametrize("R", sorted(FORMS.SPHERE_POINTS))
def test_voxel_grids_of_several_shapes(R):
    FORMS.body_sphere_grids(R)


def test_grid_values_of_several_shapes():
    FORMS.body_grid_values()


def test_points_per_shape_refusal():
    FORMS.body_points_per_shape_refusal()
