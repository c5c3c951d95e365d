"""Earth mover's distance (shapegan_amd/evaluation.py, include/shapegan_hip.h K15) on the C++ twin against the float64 statement in
emd_reference.py: scipy's exact assignment on the float64 distances.

The bodies take the device, so that test_gpu_emd.py runs the same checks on the MI355X.  The bound is the header's guarantee and
nothing else: with s = 4 * 2^-24 * emd* for the float32 rounding of the distances (emd_reference.S_REL),

    emd* - s <= emd <= emd* + eps + s        for every pair, none left out.
"""
import numpy as np
import pytest
import torch

from shapegan_amd import evaluation as E
from shapegan_amd import lib as L
import emd_reference as X
from test_evaluation import all_pairs

ROUND_CAP = 1 << 20               # SG_EMD_ROUND_CAP


def tensor(x, dev):
    """A copy on `dev`: the references of emd_reference are shared between tests and read-only."""
    return torch.from_numpy(np.array(x)).to(dev)


def raw_match(a, b, eps, dev):
    """sg_emd_match on its own: (emd [S], match [S, P], rounds [S], status [S]) as numpy."""
    a, b = tensor(a, dev), tensor(b, dev)
    S, P = a.shape[0], a.shape[1]
    emd = torch.empty(S, dtype=torch.float64, device=dev)
    match = torch.empty((S, P), dtype=torch.int32, device=dev)
    rounds = torch.empty(S, dtype=torch.int32, device=dev)
    status = torch.empty(S, dtype=torch.int32, device=dev)
    try:
        L.check(L.load().sg_emd_match(L.ptr(a), L.ptr(b), S, P, float(eps), L.ptr(match), L.ptr(emd), L.ptr(rounds), L.ptr(status),
                                      L.stream()), "emd_match")
    finally:
        L.reset_call_state()
    return tuple(t.cpu().numpy() for t in (emd, match, rounds, status))


def assert_bound(got, want, eps, what):
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    s = X.S_REL * want
    print("%s: eps %g, excess over the optimum: largest %.3g, smallest %.3g (s up to %.3g)" % (
        what, eps, float((got - want).max()), float((got - want).min()), float(s.max())))
    assert (got >= want - s).all() and (got <= want + eps + s).all(), what


def assert_answer(a, b, emd, match, what):
    """match is a permutation and emd the mean of its distances."""
    for s in range(len(a)):
        assert np.array_equal(np.sort(match[s]), np.arange(a.shape[1])), "%s: pair %d: no permutation" % (what, s)
        mean = X.matching_mean(a[s], b[s], match[s])
        assert abs(emd[s] - mean) <= X.S_REL * mean, (what, s, emd[s], mean)


def check_bound(P, eps, dev):
    A, B, want = X.case(P)
    pa, pb = all_pairs(A, B)
    emd, match = E.earth_movers_distance(tensor(pa, dev), tensor(pb, dev), eps=eps, return_matching=True)
    assert emd.dtype == torch.float64 and emd.shape == (len(pa),) and emd.device.type == dev
    assert match.dtype == torch.int32 and match.shape == pa.shape[:2]
    emd, match = emd.cpu().numpy(), match.cpu().numpy()
    assert_bound(emd, want, eps, "P = %d" % P)
    assert_answer(pa, pb, emd, match, "P = %d" % P)
    # the matrix is the matched batch, bit for bit; rows in chunks too; float64 input is accepted
    m = E.emd_matrix(tensor(A, dev), tensor(B, dev), eps=eps)
    assert m.dtype == torch.float64 and m.shape == want.shape and m.device.type == dev
    np.testing.assert_array_equal(m.cpu().numpy().reshape(-1), emd)
    m2 = E.emd_matrix(tensor(A.astype(np.float64), dev), np.array(B), eps=eps, chunk=3)
    np.testing.assert_array_equal(m2.cpu().numpy(), m.cpu().numpy())
    assert E.earth_movers_distance(tensor(A[0], dev), np.array(B[0]), eps=eps).shape == (1,)          # single clouds [P, 3]


def check_symmetric(P, eps, dev):
    A, _, _ = X.case(P)
    a = tensor(A, dev)
    full = E.emd_matrix(a, a, eps=eps).cpu().numpy()
    sym = E.emd_matrix(a, a, eps=eps, symmetric=True).cpu().numpy()
    np.testing.assert_array_equal(sym, sym.T)
    assert not np.diag(sym).any()
    upper = np.triu_indices(len(A), 1)
    np.testing.assert_array_equal(sym[upper], full[upper])
    np.testing.assert_array_equal(E.emd_matrix(a, a, eps=eps, symmetric=True, chunk=3).cpu().numpy(), sym)
    assert (np.diag(full) <= eps).all()         # a cloud against itself: the optimum is 0


def check_large_pair(eps, dev):
    a, b, want = X.one_large_pair()
    emd, match, rounds, status = raw_match(a, b, eps, dev)
    assert not status.any() and (rounds < ROUND_CAP).all()
    print("P = 2048, eps %g: %d rounds" % (eps, rounds[0]))
    assert_bound(emd, want, eps, "P = 2048")
    assert_answer(a, b, emd, match, "P = 2048")


def check_degenerate(kind, eps, dev):
    a, b = X.degenerate(kind)
    emd, match, rounds, status = raw_match(a, b, eps, dev)
    assert not status.any() and (rounds < ROUND_CAP).all(), (kind, rounds)
    print("%s, eps %g: %d rounds" % (kind, eps, rounds[0]))
    want = np.array([X.exact(a[0], b[0])])
    assert_bound(emd, want, eps, kind)
    assert_answer(a, b, emd, match, kind)
    if kind == "identical":
        assert emd[0] == 0.0
    if kind == "shuffled":
        assert want[0] == 0.0 and emd[0] <= eps


def check_non_finite(dev):
    a, b = (x.copy() for x in X.case(64)[:2])
    a[0, 5, 1] = np.nan
    b[0, 9, 2] = np.inf
    emd, match = E.earth_movers_distance(tensor(a[:2], dev), tensor(b[:2], dev), eps=1e-3, return_matching=True)
    match = match.cpu().numpy()
    for s in range(2):
        assert np.array_equal(np.sort(match[s]), np.arange(64))
    # the pair without a non-finite coordinate is the pair it was
    want = E.earth_movers_distance(tensor(a[1:2], dev), tensor(b[1:2], dev), eps=1e-3)
    assert float(emd[1]) == float(want[0])
    m = E.emd_matrix(tensor(a[:3], dev), tensor(b[:3], dev), eps=1e-3).cpu().numpy()
    assert np.isfinite(m[1:, 1:]).all()


def check_set_scores(name, dev):
    G, D, exact, want, gap = X.score_case(name)
    eps = X.SCORE_EPS
    s = X.S_REL * max(m.max() for m in exact.values())
    assert gap > 2 * (eps + s), "the input does not decide its arg-minima by more than 2 eps: %g" % gap
    got = E.evaluate(tensor(G, dev), tensor(D, dev), emd=True, emd_eps=eps)
    assert set(got) == {"mmd_cd", "cov_cd", "one_nna_cd", "jsd", "mmd_emd", "cov_emd", "one_nna_emd"}
    print("%s: %s (exact %s), smallest gap %.3g" % (name, {k: got[k] for k in want}, want, gap))
    assert want["mmd_emd"] - s <= got["mmd_emd"] <= want["mmd_emd"] + eps + s
    assert got["cov_emd"] == want["cov_emd"] and got["one_nna_emd"] == want["one_nna_emd"]
    plain = E.evaluate(tensor(G, dev), tensor(D, dev))
    assert set(plain) == {"mmd_cd", "cov_cd", "one_nna_cd", "jsd"}
    assert all(plain[k] == got[k] for k in plain)


def check_input_errors(dev):
    A, B, _ = X.case(64)
    a, b = tensor(A, dev), tensor(B, dev)
    big = torch.zeros(1, 2049, 3, device=dev)
    for call in (E.earth_movers_distance, E.emd_matrix):
        with pytest.raises(ValueError, match="same point count"):
            call(a[:2], b[:2, :63])
        with pytest.raises(ValueError, match="at most 2048"):
            call(big, big)
        for eps in (0.0, -1e-3, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="eps"):
                call(a[:2], b[:2], eps=eps)
        with pytest.raises(ValueError, match="smallest eps accepted is"):
            call(a[:2], b[:2], eps=1e-7)
        with pytest.raises(ValueError, match="smallest eps accepted is"):
            call(a[:2] * 1e6, b[:2] * 1e6, eps=1e-4)
    with pytest.raises(ValueError):
        E.evaluate(a, b[:, :63], emd=True)
    with pytest.raises(ValueError, match="same number of clouds"):
        E.earth_movers_distance(a[:2], b[:3])
    # eps = 1e-5 is accepted for clouds anywhere inside the unit cube
    corners = torch.tensor([[[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]], device=dev)
    assert float(E.earth_movers_distance(corners, corners.flip(1), eps=1e-5)) == 0.0
    # the library refuses what the Python layer refuses, by return code
    lib, out = L.load(), torch.empty(4, dtype=torch.float64, device=dev)
    status = torch.empty(4, dtype=torch.int32, device=dev)
    for P, eps in ((2049, 1e-4), (0, 1e-4), (64, 0.0), (64, -1.0), (64, float("nan"))):
        try:
            rc = lib.sg_emd_match(L.ptr(big), L.ptr(big), 1, P, eps, None, L.ptr(out), None, L.ptr(status), L.stream())
        finally:
            L.reset_call_state()
        assert rc == -1, (P, eps, rc)
    # and reports an eps below what its integers support for the pair in the pair's status: no result, no fault
    emd, match, rounds, status = raw_match(A[:2] * 100, B[:2] * 100, 1e-6, dev)
    assert (status == 2).all() and np.isnan(emd).all() and (match == np.arange(64)).all() and not rounds.any()


# ---- the twin ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", X.EPS)
@pytest.mark.parametrize("P", X.POINT_COUNTS)
def test_emd_is_within_eps_of_the_exact_optimum(P, eps):
    check_bound(P, eps, "cpu")


@pytest.mark.parametrize("P", [2, 65, 257])
def test_symmetric_matrix(P):
    check_symmetric(P, 1e-3, "cpu")


@pytest.mark.parametrize("eps", X.EPS)
def test_one_pair_of_2048_points(eps):
    check_large_pair(eps, "cpu")


@pytest.mark.parametrize("eps", X.EPS)
@pytest.mark.parametrize("kind", X.DEGENERATE)
def test_degenerate_clouds(kind, eps):
    check_degenerate(kind, eps, "cpu")


def test_non_finite_points_give_a_permutation():
    check_non_finite("cpu")


@pytest.mark.parametrize("name", sorted(X.SCORE_SETS))
def test_set_scores_match_the_exact_ones(name):
    check_set_scores(name, "cpu")


def test_input_checks():
    check_input_errors("cpu")
