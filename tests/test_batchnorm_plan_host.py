"""Which slices the BatchNorm launchers cut a channel into (host logic of libshapegan_hip.so, no GPU): ops.bn_plan returns what
sg_bn_plan reports, the functions of csrc/batchnorm_core.h the launchers themselves launch from.  Every shape of
tests/batchnorm_forms.py must get the plan it claims, and the table as a whole must contain every path the kernels have."""
import ctypes

import pytest

import batchnorm_forms as B
from shapegan_amd import lib as L
from shapegan_amd import ops


@pytest.mark.parametrize("shape_id", sorted(B.BY_ID))
def test_shape_gets_the_plan_it_claims(shape_id):
    s = B.BY_ID[shape_id]
    assert ops.bn_plan(s.N, s.C, s.S) == s.plan
    assert s.vector == (s.S % 4 == 0)
    lengths, chunk = s.slice_lengths()
    assert chunk % 4 == 0 and sum(lengths) == s.N * s.S and min(lengths) > 0
    assert (lengths[0] % 2048, lengths[-1] % 2048) == s.slices
    nsplit, napply = s.plan
    assert 1 <= nsplit <= 64 and nsplit <= napply and 64 * 2 * 8 * s.C == L._load_hip().sg_bn_workspace_bytes(s.C)


def test_the_twin_reports_the_same_plan():
    twin = L.load_cpu()
    for s in B.SHAPES:
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        assert twin.sg_bn_plan_cpu(s.N, s.C, s.S, ctypes.addressof(a), ctypes.addressof(b)) == 0
        assert (a.value, b.value) == s.plan
    assert twin.sg_bn_plan_cpu(0, 1, 1, ctypes.addressof(a), ctypes.addressof(b)) != 0
    assert L._load_hip().sg_bn_plan(1, 1, 0, ctypes.addressof(a), ctypes.addressof(b)) != 0
    assert L._load_hip().sg_bn_plan(1, 1, 1, None, ctypes.addressof(b)) != 0


@pytest.mark.parametrize("gid", B.GROUPED_IDS)
def test_grouped_case_gets_the_split_it_claims(gid):
    groups, per, C, S, nsplit = B.GROUPED_BY_ID[gid]
    assert ops.bn_plan(per, C, S)[0] == nsplit and 1 <= groups <= 64


def _mid_sample(s, count):
    """whether a slice of the `count`-way split starts inside a sample"""
    total = s.N * s.S
    chunk = ((total + count - 1) // count + 3) & ~3
    return any((i * chunk) % s.S for i in range(1, count) if i * chunk < total)


def test_the_table_covers_every_path():
    S = B.SHAPES
    multi = [s for s in S if s.plan[0] > 1]
    # the scalar form with more than one slice; the float4 form starting inside a sample with steps beyond, of and below a sample
    assert any(not s.vector for s in multi) and any(not s.vector and _mid_sample(s, s.plan[0]) for s in multi)
    vec_mid = [s for s in multi if s.vector and _mid_sample(s, s.plan[0])]
    assert any(s.S < 1024 for s in vec_mid) and any(s.S == 1024 for s in vec_mid) and any(s.S > 1024 for s in vec_mid)
    assert any(s.vector and not _mid_sample(s, s.plan[0]) for s in multi)
    # napply != nsplit: more apply slices, the 64 cap (a full wave of partials), one statistics slice with two apply slices at C > 512
    assert any(s.plan[0] == 64 and s.plan[1] > 64 for s in S) and any(s.plan[0] == 63 for s in S)
    assert any(s.C > 512 and s.plan == (1, 2) for s in S)
    assert any(s.plan[0] == 64 and s.slice_lengths()[0][0] != s.slice_lengths()[0][-1] for s in S)      # ... with a ragged last slice
    # both exits of the two-groups-in-flight loop with a non-empty single-group tail, and no tail at all
    rem = {r for s in multi if s.vector for r in s.slices}
    assert any(0 < r <= 1024 for r in rem) and any(1024 < r < 2048 for r in rem) and 0 in rem
    # the small ends, BatchNorm1d, one value per channel
    assert any(s.N * s.S == 1 for s in S) and any(s.N * s.S == 2 for s in S) and any(s.S == 1 and s.plan[0] > 1 for s in S)
    # all five activations at a float4 shape, a scalar shape and the 64 cap; the hard numerics at a float4 and a scalar shape
    full = [s for s in S if len({a for a, _ in s.acts}) == 5]
    assert any(s.vector and s.plan[0] == 2 for s in full) and any(not s.vector and s.plan[0] == 2 for s in full)
    assert any(s.plan[0] == 64 for s in full)
    assert {s.vector for s in S if s.hard} == {True, False} and len(B.HARD_KINDS) == 10
    for s in S:
        if s.hard:       # four rotations of the ten kinds reach every kind at every hard shape
            assert {B.HARD_KINDS[(c + 3 * r) % 10] for c in range(s.C) for r in range(4)} == set(B.HARD_KINDS)
        vs = B.variants(s)
        assert {v["training"] for v in vs} == {True, False} and {v["grads"] for v in vs} == {"all", "x"}
        assert {v["momentum"] for v in vs} == {0.1, 1.0} and {v["eps"] for v in vs} == {1e-5, 1e-3} and any(not v["running"] for v in vs)
        assert {(v["training"], v["grads"]) for v in vs} == {(True, "all"), (True, "x"), (False, "all"), (False, "x")}
    assert {v["slope"] for s in S for v in B.variants(s) if v["act"] == B.LEAKY} == {0.2, 0.01}
    assert {g[0] for g in B.GROUPED} == {1, 2, 5, 64} and {g[1:4] for g in B.GROUPED if g[0] == 64} == {(2, 3, 8), (130, 2, 64)}
    assert set(B.TWIN_IDS) <= set(B.BY_ID) and len(B.TWIN_IDS) >= len(S) - 1
