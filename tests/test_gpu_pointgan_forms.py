"""GPU tier: the point-GAN kernels in every calling form against float64 — the LayerNorm form of the fused MLP (csrc/sdfnet.hip,
csrc/sdfnet_tile.h, ops.SDFGenFused, SDFGenerator: shapes on both sides of the 32-point forward tiles, one-hot upstream gradients,
which inputs require grad, positions that require grad, offset rows, eps, the C ABI with ldn > N) and the fused PointNet selection
pass (csrc/pointnet.hip, ops.pointnet_select, every branch of PointNet.forward, the gradient penalty).  Bodies, references and the
criterion: tests/pointgan_forms.py (re-run on the twin by tests/test_cpu_twin.py)."""
import pytest

import pointgan_forms as PG

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("S,pps,sid", PG.SHAPES)
def test_generator_shapes(S, pps, sid):
    PG.body_shapes(S, pps, sid)


@pytest.mark.parametrize("where", sorted(PG.ONE_HOT_POSITIONS))
def test_generator_one_hot(where):
    PG.body_one_hot(where)


@pytest.mark.parametrize("need_z,need_lins,need_norms", PG.SUBSETS)
def test_generator_which_grads(need_z, need_lins, need_norms):
    PG.body_which_grads(need_z, need_lins, need_norms)


def test_generator_forward_without_grad():
    PG.body_no_grad_forward()


def test_generator_positions_require_grad():
    PG.body_positions_require_grad()


def test_generator_offset_rows():
    PG.body_offset_rows()


def test_generator_eps():
    PG.body_eps(1e-3)


def test_generator_raw_abi_ldn():
    PG.body_raw_abi_ldn()


@pytest.mark.parametrize("B,P,twin_rows", PG.SELECT_CASES)
def test_pointnet_select(B, P, twin_rows):
    PG.body_select(B, P, twin_rows)


@pytest.mark.parametrize("P", PG.FORWARD_POINTS)
def test_pointnet_forward_forms(P):
    PG.body_forward_forms(P)


@pytest.mark.parametrize("P", PG.PENALTY_POINTS)
def test_pointnet_gradient_penalty(P):
    PG.body_gradient_penalty(P)
