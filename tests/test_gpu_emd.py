"""Earth mover's distance on the MI355X (csrc/emd.hip): the bodies of test_emd.py on the device against the exact optimum, and the
kernel against the C++ twin bit for bit: value, matching and number of rounds."""
import numpy as np
import pytest
import torch

from shapegan_amd import evaluation as E
from shapegan_amd import lib as L
import emd_reference as X
import evaluation_reference as R
import test_emd as T
from test_evaluation import all_pairs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("eps", X.EPS)
@pytest.mark.parametrize("P", X.POINT_COUNTS)
def test_emd_is_within_eps_of_the_exact_optimum(P, eps):
    T.check_bound(P, eps, "cuda")


@pytest.mark.parametrize("P", [2, 65, 257])
def test_symmetric_matrix(P):
    T.check_symmetric(P, 1e-3, "cuda")


@pytest.mark.parametrize("eps", X.EPS)
def test_one_pair_of_2048_points(eps):
    T.check_large_pair(eps, "cuda")


@pytest.mark.parametrize("eps", X.EPS)
@pytest.mark.parametrize("kind", X.DEGENERATE)
def test_degenerate_clouds(kind, eps):
    T.check_degenerate(kind, eps, "cuda")


def test_non_finite_points_give_a_permutation():
    T.check_non_finite("cuda")


@pytest.mark.parametrize("name", sorted(X.SCORE_SETS))
def test_set_scores_match_the_exact_ones(name):
    T.check_set_scores(name, "cuda")


def test_input_checks():
    T.check_input_errors("cuda")
    A, B, _ = X.case(64)
    for call in (E.earth_movers_distance, E.emd_matrix):
        with pytest.raises(ValueError, match="different devices"):
            call(T.tensor(A, "cuda"), T.tensor(B, "cpu"))


# ---- GPU against twin: the same bits ---------------------------------------------------------------------------------------------
def assert_same_as_twin(a, b, eps):
    gpu, cpu = T.raw_match(a, b, eps, "cuda"), T.raw_match(a, b, eps, "cpu")
    for got, want, what in zip(gpu, cpu, ("emd", "match", "rounds", "status")):
        np.testing.assert_array_equal(got, want, err_msg=what)
    return gpu


@pytest.mark.parametrize("eps", X.EPS)
@pytest.mark.parametrize("P", X.POINT_COUNTS + (2048,))
def test_gpu_equals_twin_bit_for_bit(P, eps):
    if P == 2048:
        a, b, _ = X.one_large_pair()
    else:
        A, B, _ = X.case(P)
        a, b = all_pairs(A, B)
    emd, match, rounds, status = assert_same_as_twin(a, b, eps)
    print("P = %d, eps %g: rounds median %d, max %d" % (P, eps, np.median(rounds), rounds.max()))
    assert not status.any()


@pytest.mark.parametrize("kind", X.DEGENERATE)
def test_gpu_equals_twin_on_degenerate_clouds(kind):
    assert_same_as_twin(*X.degenerate(kind), 1e-5)


@pytest.mark.parametrize("wave_scan_at,block_scan_at", [(0, 0), (256, 0), (64, 1), (1, 16), (256, 16)])
def test_every_form_of_a_round_gives_the_same_bits(wave_scan_at, block_scan_at):
    """One lane per bidder only (0, 0), a wave per bidder up to the most the kernel takes (256), the whole workgroup per bidder up
    to the most it takes (16), and switches in between, against the defaults."""
    A, B, _ = X.case(512)
    a, b = T.tensor(A, "cuda"), T.tensor(B, "cuda")
    want = T.raw_match(A, B, 1e-4, "cuda")
    S, P = a.shape[:2]
    emd = torch.empty(S, dtype=torch.float64, device="cuda")
    match = torch.empty((S, P), dtype=torch.int32, device="cuda")
    rounds, status = (torch.empty(S, dtype=torch.int32, device="cuda") for _ in range(2))
    L.check(L.load().sg_emd_match_impl(L.ptr(a), L.ptr(b), S, P, 1e-4, L.ptr(match), L.ptr(emd), L.ptr(rounds), L.ptr(status),
                                       wave_scan_at, block_scan_at, L.stream()), "emd_match_impl")
    L.reset_call_state()
    for got, ref in zip((emd, match, rounds, status), want):
        np.testing.assert_array_equal(got.cpu().numpy(), ref)


def test_matrix_of_many_large_clouds_matches_twin_on_a_sub_block():
    """40 x 40 clouds of 2048 points, eps = 1e-3: a 5 x 5 sub-block of sampled rows and columns against the twin on those clouds
    alone catches the grid indexing; the symmetric form against the full one on its upper triangle."""
    a, b = R.make_set(40, 2048, 41), R.make_set(40, 2048, 42, first_kind=2)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    m = E.emd_matrix(ta, tb, eps=1e-3).cpu().numpy()
    rng = np.random.default_rng(43)
    rows, cols = np.sort(rng.choice(40, 5, replace=False)), np.sort(rng.choice(40, 5, replace=False))
    want = E.emd_matrix(torch.from_numpy(a[rows]), torch.from_numpy(b[cols]), eps=1e-3).numpy()
    np.testing.assert_array_equal(m[np.ix_(rows, cols)], want)
    sym = E.emd_matrix(ta[:12], ta[:12], eps=1e-3, symmetric=True).cpu().numpy()
    full = E.emd_matrix(ta[:12], ta[:12], eps=1e-3).cpu().numpy()
    upper = np.triu_indices(12, 1)
    np.testing.assert_array_equal(sym[upper], full[upper])
    np.testing.assert_array_equal(sym, sym.T)
    assert not np.diag(sym).any()
