"""GPU tier: BatchNorm in every dispatch form against float64 (bodies, case table, bounds: tests/batchnorm_forms.py; the plan each shape
claims is asserted without a GPU by tests/test_batchnorm_plan_host.py)."""
import pytest

import batchnorm_forms as B

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape_id", [s.id for s in B.SHAPES])
def test_batchnorm_forms(shape_id):
    B.body_shape(shape_id)


@pytest.mark.parametrize("gid", B.GROUPED_IDS)
def test_batchnorm_grouped_forms(gid):
    B.body_grouped(gid)


def test_batchnorm_refusals_touch_no_output():
    B.body_refusals()
