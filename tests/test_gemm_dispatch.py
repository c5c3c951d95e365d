"""Which kernel sg_gemm and the sg_gemm_nt entries launch (host logic of libshapegan_hip.so, no GPU): sg_gemm_plan / sg_gemm_nt_plan
return the value the launchers themselves launch from.  Every case of tests/gemm_forms.py must plan what it claims to reach, and the
boundaries of the dispatch are pinned one case on each side."""
import pytest

import gemm_forms as G
from gemm_forms import FIN_DEEP, FIN_FLAT, FIN_NONE, GEMM128, GEMM128_SPLIT, PERSISTENT, SKELETON


@pytest.mark.parametrize("case_id", sorted(G.GEMM_BY_ID))
def test_gemm_case_reaches_the_kernel_it_claims(case_id):
    case = G.GEMM_BY_ID[case_id]
    plan = case.query()
    assert plan["key"] == case.plan, plan
    assert plan["layout"] == 2 * (case.la == "k") + (case.lb == "k")
    if plan["kind"] != SKELETON:
        assert (case.la, case.lb) != ("r", "k") and case.aligned
    if plan["nsplit"] > 1:      # the partials fit the workspace handed over, and every split owns a part of K
        assert plan["nsplit"] * case.M * case.N * 4 <= case.ws_bytes()
        assert (plan["nsplit"] - 1) * plan["kchunk"] < case.K <= plan["nsplit"] * plan["kchunk"] or plan["kind"] == SKELETON
    assert (plan["finalize"] == FIN_NONE) == (plan["nsplit"] == 1)


def test_the_table_covers_every_branch():
    """layouts x tile plans x epilogue of the skeleton, the gemm128 family by layout and finalize, the flat finalize's split counts"""
    seen = {(c.la + c.lb,) + c.plan for c in G.GEMM_CASES}
    for layout in ("kk", "kr", "rk", "rr"):
        for tm, tn in ((1, 1), (1, 2), (2, 1), (2, 2)):
            fins = {k[5] for k in seen if k[:4] == (layout, SKELETON, tm, tn)}
            assert fins == {FIN_NONE, FIN_FLAT, FIN_DEEP}, (layout, tm, tn, fins)
    for layout in ("kk", "kr", "rr"):
        for kind, fin in ((GEMM128, FIN_NONE), (GEMM128_SPLIT, FIN_FLAT), (GEMM128_SPLIT, FIN_DEEP), (PERSISTENT, FIN_NONE)):
            assert any(k[0] == layout and k[1] == kind and k[5] == fin for k in seen), (layout, kind, fin)
    flat_splits = {c.plan[3] for c in G.GEMM_CASES if c.plan[4] == FIN_FLAT and c.N % 4 == 0}
    assert {2, 3, 4, 5, 6, 7, 8, 16} <= flat_splits            # groups of four partials with remainders 0, 1, 2 and 3
    assert any(c.plan[4] == FIN_FLAT and c.N % 4 for c in G.GEMM_CASES)
    assert set(G.NONFINITE_IDS + G.POISON_IDS + G.POISON_TWIN_IDS + G.GEMM_TWIN_IDS) <= set(G.GEMM_BY_ID)
    assert sorted(G.GEMM_BY_ID[i].plan[0] for i in G.NONFINITE_IDS) == [SKELETON, GEMM128, GEMM128_SPLIT, PERSISTENT]
    assert sorted(G.GEMM_BY_ID[i].plan[0] for i in G.POISON_IDS) == [SKELETON, GEMM128, GEMM128_SPLIT, PERSISTENT]


@pytest.mark.parametrize("case_id", sorted(G.NT_BY_ID))
def test_gemm_nt_case_plans_what_it_claims(case_id):
    case = G.NT_BY_ID[case_id]
    plan = G.query_nt_plan(case.batch, case.M, case.N, case.K)
    assert (plan["direct"], plan["nsplit"]) == case.plan, plan
    tiles = -(-case.M // 128) * -(-case.N // 128)
    assert plan["grid"] == -(-case.batch * plan["nsplit"] // 8) * 8 * tiles
    assert plan["ws_bytes"] == (0 if plan["direct"] else case.batch * plan["nsplit"] * case.M * case.N * 4)
    assert (plan["nsplit"] - 1) * plan["kchunk"] < case.K <= plan["nsplit"] * plan["kchunk"] and plan["kchunk"] % 32 == 0
    lib = G._lib()
    if case.batch == 1:
        assert lib.sg_gemm_nt_workspace_bytes(case.M, case.N, case.K) == plan["ws_bytes"]
    assert lib.sg_gemm_nt_batched_workspace_bytes(case.batch, case.M, case.N, case.K) == case.batch * plan["nsplit"] * case.M * case.N * 4


def test_gemm_nt_table_covers_the_issue():
    plans = {(c.entry != "nt", c.batch) + c.plan for c in G.NT_CASES}
    assert {c.plan[1] for c in G.NT_CASES} >= {1, 2, 3, 256}
    for batch in (1, 2, 8):
        assert any(p[1] == batch and p[3] == 1 for p in plans) and any(p[1] == batch and p[3] > 1 for p in plans)
    assert {c.M for c in G.NT_CASES} >= {1, 70, 128, 129, 256, 260} and {c.N for c in G.NT_CASES} >= {1, 70, 128, 129, 256, 260}


# ---- boundaries, one case on each side -------------------------------------------------------------------------------------------------
A0, B0, W0 = 0x10000, 0x20000, 0x30000       # 16-byte aligned addresses


def plan(M, N, K, la="k", lb="k", lda=None, ldb=None, a=A0, b=B0, ws=W0, ws_bytes=None, sci=None, scj=1, bias_i=False):
    lda = lda or ((K if la == "k" else M) + 3) // 4 * 4 + 4
    ldb = ldb or ((K if lb == "k" else N) + 3) // 4 * 4 + 4
    sai, sak = (lda, 1) if la == "k" else (1, lda)
    sbk, sbj = (1, ldb) if lb == "k" else (ldb, 1)
    if ws_bytes is None:
        ws_bytes = min(128 * M * N * 4, G.WS_CAP)
    return G.query_plan(a, sai, sak, b, sbk, sbj, N + 5 if sci is None else sci, scj, bias_i, M, N, K, ws, ws_bytes)


def test_m_and_n_127_128():
    assert plan(127, 16384, 64)["kind"] == SKELETON and plan(128, 16384, 64)["key"] == (GEMM128, 0, 0, 1, FIN_NONE)
    assert plan(16384, 127, 64)["kind"] == SKELETON and plan(16384, 128, 64)["key"] == (GEMM128, 0, 0, 1, FIN_NONE)


def test_k_63_64():
    assert plan(1000, 2000, 63)["kind"] == SKELETON and plan(1000, 2000, 64)["kind"] == GEMM128


def test_m_times_n_below_and_at_2_to_16():
    assert 255 * 257 == 2 ** 16 - 1
    assert plan(255, 257, 16384)["kind"] == SKELETON
    assert plan(256, 256, 16384)["key"] == (GEMM128_SPLIT, 0, 0, 64, FIN_DEEP)


def test_workgroups_127_128():
    assert plan(127 * 128, 128, 64)["kind"] == SKELETON                      # 127 tiles, no split at K = 64
    assert plan(128 * 128, 128, 64)["key"] == (GEMM128, 0, 0, 1, FIN_NONE)
    assert plan(128 * 128, 128, 64)["grid"] == 128
    # tiles x s: 32 tiles with 3 / 4 partials
    assert plan(129, 2000, 1024, ws_bytes=3 * 129 * 2000 * 4)["kind"] == SKELETON
    assert plan(129, 2000, 1024, ws_bytes=4 * 129 * 2000 * 4)["key"] == (GEMM128_SPLIT, 0, 0, 4, FIN_FLAT)


@pytest.mark.parametrize("K,even", [(64, True), (96, False), (128, True), (160, False)])
def test_tiles_512_513_and_the_stage_count(K, even):
    at = plan(4096, 2048, K)                                                 # 32 x 16 tiles
    over = plan(3456, 2432, K)                                               # 27 x 19 tiles
    assert at["key"] == (GEMM128, 0, 0, 1, FIN_NONE) and at["grid"] == 512
    assert over["key"] == (PERSISTENT if even else GEMM128, 0, 0, 1, FIN_NONE) and over["grid"] == (512 if even else 513)


def test_leading_dimension_and_base_alignment():
    assert plan(1000, 2000, 64, lda=68)["kind"] == GEMM128
    for lda in (69, 70, 71):
        assert plan(1000, 2000, 64, lda=lda)["kind"] == SKELETON
    assert plan(1000, 2000, 64, ldb=70)["kind"] == SKELETON
    assert plan(1000, 2000, 64, a=A0 + 4)["kind"] == SKELETON and plan(1000, 2000, 64, b=B0 + 4)["kind"] == SKELETON
    assert plan(1000, 2000, 64, a=A0 + 16, b=B0 + 32)["kind"] == GEMM128


def test_row_major_operands_need_whole_pieces():
    assert plan(1000, 2000, 64, la="r", lb="r")["kind"] == GEMM128
    assert plan(1002, 2000, 64, la="r", lb="r")["kind"] == SKELETON          # M & 3 with a row-major A
    assert plan(1000, 2002, 64, la="k", lb="r")["kind"] == SKELETON          # N & 3 with a row-major B
    assert plan(1002, 2002, 64)["kind"] == GEMM128                           # k-major operands do not care
    assert plan(1000, 2000, 64, la="r", lb="k")["kind"] == SKELETON          # the layout gemm128 does not have


def test_deep_flat_finalize_fork():
    """>= 32 partials of at most 2^18 elements go to the deep finalize.  A product of more than 2^18 elements has more than 16 tiles of
    128 x 128 and the planners then ask for at most ceil(512 / 17) = 31 partials: through sg_gemm the fork is decided by the split
    count alone, and 2^18 + 4 = 4 x 65537 elements cannot be split at all (a 4 x 65537 product has 513 column tiles)."""
    assert plan(512, 512, 31 * 256)["key"] == (GEMM128_SPLIT, 0, 0, 31, FIN_FLAT)
    assert plan(512, 512, 32 * 256)["key"] == (GEMM128_SPLIT, 0, 0, 32, FIN_DEEP)
    assert plan(512, 512, 64 * 256)["key"] == (GEMM128_SPLIT, 0, 0, 32, FIN_DEEP)
    over = plan(516, 512, 64 * 256)                                          # 2^18 + 2048 elements: 20 tiles
    assert over["kind"] == GEMM128_SPLIT and over["nsplit"] <= 31 and over["finalize"] == FIN_FLAT
    tall = plan(4, 65537, 64 * 256, lda=64 * 256 + 1)                        # 2^18 + 4 elements
    assert tall["key"] == (SKELETON, 1, 2, 1, FIN_NONE)
    # the skeleton's own fork, through a capped workspace
    assert plan(1, 64, 4096, lda=4097)["key"] == (SKELETON, 1, 1, 32, FIN_DEEP)
    assert plan(1, 64, 4096, lda=4097, ws_bytes=31 * 64 * 4)["key"] == (SKELETON, 1, 1, 31, FIN_FLAT)


def test_workspace_short_and_null():
    P = 1000 * 2000 * 4
    assert plan(1000, 2000, 1024, ws_bytes=4 * P)["key"] == (GEMM128_SPLIT, 0, 0, 4, FIN_FLAT)
    assert plan(1000, 2000, 1024, ws_bytes=4 * P - 1)["key"] == (GEMM128_SPLIT, 0, 0, 3, FIN_FLAT)
    assert plan(1000, 2000, 1024, ws_bytes=2 * P - 1)["key"] == (GEMM128, 0, 0, 1, FIN_NONE)
    assert plan(1000, 2000, 1024, ws_bytes=0)["key"] == (GEMM128, 0, 0, 1, FIN_NONE)
    assert plan(1000, 2000, 1024, ws=None, ws_bytes=4 * P)["key"] == (GEMM128, 0, 0, 1, FIN_NONE)
    # the skeleton: one byte short of S partials plans S - 1, a null workspace none
    assert plan(1, 64, 4096, lda=4097, ws_bytes=7 * 64 * 4)["nsplit"] == 7
    assert plan(1, 64, 4096, lda=4097, ws_bytes=7 * 64 * 4 - 1)["nsplit"] == 6
    assert plan(1, 64, 4096, lda=4097, ws=None)["key"] == (SKELETON, 1, 1, 1, FIN_NONE)


def test_epilogues_that_switch_the_persistent_form_off():
    assert plan(2000, 4100, 64)["key"] == (PERSISTENT, 0, 0, 1, FIN_NONE)
    assert plan(2000, 4100, 64, sci=4100)["kind"] == PERSISTENT              # sci == N: rows touch, they do not overlap
    assert plan(2000, 4100, 64, sci=4099)["key"] == (GEMM128, 0, 0, 1, FIN_NONE)
    assert plan(2000, 4100, 64, sci=1, scj=2003)["key"] == (GEMM128, 0, 0, 1, FIN_NONE)
    assert plan(2000, 4100, 64, sci=8200, scj=2)["key"] == (GEMM128, 0, 0, 1, FIN_NONE)
    assert plan(2000, 4100, 64, bias_i=True)["key"] == (GEMM128, 0, 0, 1, FIN_NONE)
    assert plan(2000, 4100, 64, bias_i=True)["grid"] == 528


def test_grid_and_kchunk_of_the_skeleton():
    p = plan(129, 2000, 2050, lda=2051)
    assert p["key"] == (SKELETON, 2, 2, 16, FIN_FLAT) and p["grid"] == 16 * 2 * 16 and p["kchunk"] == 144
    p = plan(5, 7, 40, lda=41)
    assert p["key"] == (SKELETON, 1, 1, 1, FIN_NONE) and p["grid"] == 1 and p["kchunk"] == 40


# The plans the older GEMM tests reached at the commit before the plan query existed, recorded there from the launcher's arithmetic
# (gemm128_try, plan_tiles, gemm_nt_plan) for the calls those tests make through ops.gemm_raw / ops.gemm_nt_raw: exact leading
# dimensions, contiguous C, the workspace min(128 M N 4, 256 MiB).  (kind, tm, tn, nsplit, finalize, grid) with kind 0 skeleton,
# 1 gemm128, 2 gemm128 with a K split, 3 persistent and finalize 0 none, 1 flat, 2 deep.
# test_linear_fwd_bwd (M rows, N out, K in): forward M x N x K kk, input gradient M x K x N kr, weight gradient N x K x M rr
EXISTING_LINEAR = [
    ((64, 128, 256), (0, 1, 1, 2, 1, 4), (0, 1, 1, 1, 0, 4), (0, 1, 1, 1, 0, 8)),
    ((4, 128, 256), (0, 1, 1, 2, 1, 4), (0, 1, 1, 1, 0, 4), (0, 1, 1, 1, 0, 8)),
    ((16, 128, 16384), (0, 1, 1, 128, 2, 256), (0, 1, 1, 1, 0, 256), (0, 1, 1, 1, 0, 512)),
    ((64, 1, 16384), (0, 1, 1, 128, 2, 128), (0, 1, 1, 1, 0, 256), (0, 1, 1, 1, 0, 256)),
    ((5, 7, 3), (0, 1, 1, 1, 0, 1), (0, 1, 1, 1, 0, 1), (0, 1, 1, 1, 0, 1)),
    ((200, 300, 130), (0, 1, 1, 1, 0, 20), (0, 1, 1, 2, 1, 24), (0, 1, 1, 1, 0, 15)),
    ((64, 16384, 128), (0, 1, 1, 1, 0, 256), (0, 1, 1, 128, 2, 256), (1, 0, 0, 1, 0, 128)),
    ((20000, 256, 256), (1, 0, 0, 1, 0, 314), (1, 0, 0, 1, 0, 314), (2, 0, 0, 70, 2, 288)),
    ((16388, 384, 320), (1, 0, 0, 1, 0, 387), (1, 0, 0, 1, 0, 387), (2, 0, 0, 57, 2, 576)),
    ((40004, 128, 100), (1, 0, 0, 1, 0, 313), (0, 2, 1, 1, 0, 626), (0, 1, 1, 128, 2, 512)),
    ((70004, 256, 128), (3, 0, 0, 1, 0, 512), (3, 0, 0, 1, 0, 512), (0, 2, 1, 128, 2, 512)),
]
# test_gemm128_persistent_all_layouts and test_gpu_unwritten.py::test_gemm_forms: M x N x K as kk, kr and rr
EXISTING_LAYOUTS = [
    ((70004, 256, 128), (3, 0, 0, 1, 0, 512), (3, 0, 0, 1, 0, 512), (3, 0, 0, 1, 0, 512)),
    ((66000, 384, 64), (3, 0, 0, 1, 0, 512), (3, 0, 0, 1, 0, 512), (3, 0, 0, 1, 0, 512)),
    ((131072, 128, 320), (3, 0, 0, 1, 0, 512), (3, 0, 0, 1, 0, 512), (3, 0, 0, 1, 0, 512)),
    ((70004, 256, 100), (3, 0, 0, 1, 0, 512), (3, 0, 0, 1, 0, 512), (3, 0, 0, 1, 0, 512)),
    ((200, 300, 130), (0, 1, 1, 1, 0, 20), (0, 1, 1, 1, 0, 20), (0, 1, 1, 1, 0, 20)),
    ((16388, 384, 320), (1, 0, 0, 1, 0, 387), (1, 0, 0, 1, 0, 387), (1, 0, 0, 1, 0, 387)),
    ((40004, 128, 100), (1, 0, 0, 1, 0, 313), (1, 0, 0, 1, 0, 313), (1, 0, 0, 1, 0, 313)),
]
# test_gemm_nt_bigk and test_gemm_nt_lnrelu_matches_torch: (batch, M, N, K) -> (direct, nsplit, kchunk, grid, workspace bytes)
EXISTING_NT = [
    ((1, 256, 256, 20000), (0, 70, 288, 288, 18350080)),
    ((1, 256, 256, 4099), (0, 15, 288, 64, 3932160)),
    ((1, 70, 130, 1000), (0, 3, 352, 16, 109200)),
    ((1, 256, 256, 31), (1, 1, 32, 32, 0)),
    ((1, 32, 256, 262144), (0, 256, 1024, 512, 8388608)),
    ((1, 256, 256, 33), (1, 1, 64, 32, 0)),
    ((2, 256, 256, 4133), (0, 15, 288, 128, 7864320)),
]


def _raw(M, N, K, la, lb):
    p = plan(M, N, K, la=la, lb=lb, lda=K if la == "k" else M, ldb=K if lb == "k" else N, sci=N)
    return p["key"] + (p["grid"],)


@pytest.mark.parametrize("shape,fwd,dgrad,wgrad", EXISTING_LINEAR)
def test_existing_linear_shapes_keep_their_plans(shape, fwd, dgrad, wgrad):
    M, N, K = shape
    assert (_raw(M, N, K, "k", "k"), _raw(M, K, N, "k", "r"), _raw(N, K, M, "r", "r")) == (fwd, dgrad, wgrad)


@pytest.mark.parametrize("shape,kk,kr,rr", EXISTING_LAYOUTS)
def test_existing_layout_shapes_keep_their_plans(shape, kk, kr, rr):
    assert (_raw(*shape, "k", "k"), _raw(*shape, "k", "r"), _raw(*shape, "r", "r")) == (kk, kr, rr)


@pytest.mark.parametrize("shape,want", EXISTING_NT)
def test_existing_gemm_nt_shapes_keep_their_plans(shape, want):
    p = G.query_nt_plan(*shape)
    assert (int(p["direct"]), p["nsplit"], p["kchunk"], p["grid"], p["ws_bytes"]) == want
