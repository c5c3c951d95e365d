"""GPU tier: the GEMM family in every dispatch form against float64 (bodies, case tables and checks: tests/gemm_forms.py; which kernel
each case reaches is asserted without a GPU by tests/test_gemm_dispatch.py and again, on the call's own pointers, inside the bodies)."""
import pytest

import gemm_forms as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case_id", [c.id for c in G.GEMM_CASES])
def test_gemm(case_id):
    G.body_gemm(case_id)


@pytest.mark.parametrize("case_id", G.NONFINITE_IDS)
def test_gemm_nan_and_inf_stay_where_the_reference_has_them(case_id):
    G.body_gemm_nonfinite(case_id)


@pytest.mark.parametrize("case_id", [c.id for c in G.NT_CASES])
def test_gemm_nt(case_id):
    G.body_gemm_nt(case_id)


def test_gemm_nt_nan_and_inf_stay_where_the_reference_has_them():
    G.body_gemm_nt_nonfinite()


@pytest.mark.parametrize("case_id", ["nt-b1-70x128x515", "batched-b2-70x129x100", "batched-b8-70x260x1003", "lnrelu-b2-129x260x1003"])
def test_gemm_nt_workspace_one_byte_short_is_refused(case_id):
    G.body_gemm_nt_short_workspace(case_id)


@pytest.mark.parametrize("rows,length", G.ROWSUM_CASES)
def test_rowsum(rows, length):
    G.body_rowsum(rows, length)


@pytest.mark.parametrize("ndst,rows_per_dst,length,strided", G.ROWSUM_MULTI_CASES)
def test_rowsum_multi(ndst, rows_per_dst, length, strided):
    G.body_rowsum_multi(ndst, rows_per_dst, length, strided)


@pytest.mark.parametrize("rows,nseg,lengths", G.SEGSUM_CASES)
def test_segsum(rows, nseg, lengths):
    G.body_segsum(rows, nseg, lengths)


@pytest.mark.parametrize("rows,cols", G.COLSUM_CASES)
def test_colsum(rows, cols):
    G.body_colsum(rows, cols)
