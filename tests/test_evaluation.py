"""Point-cloud evaluation (shapegan_amd/evaluation.py) on the C++ twin against the float64 statement in evaluation_reference.py.

The bodies take the device, so that test_gpu_evaluation.py runs the same checks on the MI355X.  Bounds (evaluation_reference):
distances within 6 * 2^-24 of the float64 minimum (the float32 formula of a pair is off by at most 5 * 2^-24, relative), means
within the same bound of their own value, indices exact outside the fragile points (runner-up within 12 * 2^-24; an exact tie is
NOT fragile and must give the lowest index), histogram counts exact outside the points within 4 * 2^-24 * R cells of a boundary;
at most 1e-3 of the points may be fragile.
"""
import numpy as np
import pytest
import torch

from shapegan_amd import evaluation as E
import evaluation_reference as R


def all_pairs(a, b):
    """Matched batches that pair every cloud of a with every cloud of b: pair i * Sb + j is (a[i], b[j])."""
    return np.repeat(a, len(b), axis=0), np.tile(b, (len(a), 1, 1))


def assert_rel(got, want, rtol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    worst = float((err / np.where(want > 0, want, 1.0)).max())
    print("%s: worst relative error %.3g x 2^-24 (bound %.3g)" % (what, worst / R.U, rtol / R.U))
    assert (err <= rtol * want).all(), (what, worst)


def check_matrix(name, dev):
    a, b = R.case_sets(name)
    ab, ba = E.chamfer_matrix(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
    assert ab.dtype == ba.dtype == torch.float64 and ab.shape == ba.shape == (len(a), len(b)) and ab.device.type == dev
    want_ab, want_ba = R.chamfer_matrix(a, b)
    assert_rel(ab.cpu().numpy(), want_ab, R.DIST_RTOL, name + " ab")
    assert_rel(ba.cpu().numpy(), want_ba, R.DIST_RTOL, name + " ba")
    # rows in chunks give the same bits, and float64 input is accepted
    ab2, ba2 = E.chamfer_matrix(torch.from_numpy(a.astype(np.float64)).to(dev), torch.from_numpy(b).to(dev), chunk=3)
    assert torch.equal(ab, ab2) and torch.equal(ba, ba2)


def check_nearest(name, dev):
    a, b = R.case_sets(name)
    pa, pb = all_pairs(a, b)
    da, ia, db, ib = (t.cpu().numpy() for t in E.nearest_neighbours(torch.from_numpy(pa).to(dev), torch.from_numpy(pb).to(dev)))
    assert da.dtype == db.dtype == np.float32 and ia.dtype == ib.dtype == np.int32
    assert da.shape == ia.shape == pa.shape[:2] and db.shape == ib.shape == pb.shape[:2]
    fragile = total = 0
    for s in range(len(pa)):
        ra, ja, fa, rb, jb, fb = R.nearest(pa[s], pb[s])
        for got_d, got_i, want_d, want_i, frag, limit in ((da[s], ia[s], ra, ja, fa, pb.shape[1]), (db[s], ib[s], rb, jb, fb, pa.shape[1])):
            assert (np.abs(got_d - want_d) <= R.DIST_RTOL * want_d).all(), (name, s)
            assert (got_i >= 0).all() and (got_i < limit).all()
            assert np.array_equal(got_i[~frag], want_i[~frag]), (name, s)
            fragile += int(frag.sum())
            total += frag.size
    print("%s: %d fragile points of %d" % (name, fragile, total))
    assert fragile <= R.FRAGILE_CAP * total
    # the matched-batch distance is the diagonal of the matrix sums
    d = E.chamfer_distance(torch.from_numpy(pa).to(dev), torch.from_numpy(pb).to(dev))
    want = np.array([sum(x.mean() for x in (R.nearest(pa[s], pb[s])[0], R.nearest(pa[s], pb[s])[3])) for s in range(min(len(pa), 3))])
    assert_rel(d.cpu().numpy()[:len(want)], want, R.DIST_RTOL, name + " chamfer_distance")


def check_ties(dev):
    a, b = R.duplicate_clouds()
    A = torch.from_numpy(np.stack([a])).to(dev)
    da, ia, db, ib = (t.cpu().numpy()[0] for t in E.nearest_neighbours(A, A))
    first = np.arange(300)
    first[100:150] -= 100                        # the duplicates answer with the lower index of their pair
    assert not da.any() and not db.any()
    assert np.array_equal(ia, first) and np.array_equal(ib, first)
    d, ja, jb = E.chamfer_distance(A, torch.from_numpy(np.stack([b])).to(dev), return_indices=True)
    ra, wa, fa, rb, wb, fb = R.nearest(a, b)
    assert not fa.any() and not fb.any()         # the exact ties are not fragile
    assert np.array_equal(ja.cpu().numpy()[0], wa) and np.array_equal(jb.cpu().numpy()[0], wb)
    assert (wa[60:70] == np.arange(10)).all() and (wb[150:200] == wb[20:70]).all()
    assert_rel(d.cpu().numpy(), [ra.mean() + rb.mean()], R.DIST_RTOL, "duplicates")
    ab, ba = E.chamfer_matrix(A, A)
    assert float(ab) == 0.0 and float(ba) == 0.0


def check_non_finite(dev):
    """Unspecified values, but every index in range and the untouched clouds unharmed."""
    a, b = R.case_sets("64x33")
    a, b = a.copy(), b.copy()
    a[1, 5] = np.nan
    a[1, 6, 0] = np.inf
    b[2, 0] = -np.inf
    b[3] = np.nan
    _, ia, _, ib = E.nearest_neighbours(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
    assert int(ia.min()) >= 0 and int(ia.max()) < 33 and int(ib.min()) >= 0 and int(ib.max()) < 64
    ab, _ = E.chamfer_matrix(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))
    want, _ = R.chamfer_matrix(a[:1], b[:2])
    assert_rel(ab.cpu().numpy()[:1, :2], want, R.DIST_RTOL, "finite rows beside non-finite ones")
    h = E.occupancy_histogram(torch.from_numpy(a).to(dev), 8)
    assert int(h.sum()) == a.shape[0] * a.shape[1] and int(h.min()) >= 0


def check_histogram(name, res, dev):
    a, b = R.case_sets(name)
    ha = E.occupancy_histogram(torch.from_numpy(a).to(dev), res)
    hb = E.occupancy_histogram(torch.from_numpy(b).to(dev), res)
    assert ha.dtype == torch.int64 and ha.shape == (res, res, res)
    fragile_points = []
    for h, clouds in ((ha, a), (hb, b)):
        want, fragile, n = R.occupancy(clouds, res)
        assert int(h.sum()) == clouds.shape[0] * clouds.shape[1]
        assert n <= R.FRAGILE_CAP * clouds.shape[0] * clouds.shape[1]
        assert (np.abs(h.cpu().numpy() - want) <= R.neighbourhood_sum(fragile)).all()
        fragile_points.append(n)
    print("%s R=%d: %s fragile points" % (name, res, fragile_points))
    got = E.jsd(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), resolution=res)
    assert abs(got - R.jsd(ha.cpu().numpy(), hb.cpu().numpy())) <= 1e-12
    # 1e-12 when no point is fragile, otherwise what the fragile points can move it by
    bound = R.jsd_bound(fragile_points[0], a.shape[0] * a.shape[1], fragile_points[1], b.shape[0] * b.shape[1], res ** 3)
    assert abs(got - R.jsd(R.occupancy(a, res)[0], R.occupancy(b, res)[0])) <= bound
    assert 0.0 <= got <= 1.0 + 1e-12
    assert abs(E.jsd(torch.from_numpy(a).to(dev), torch.from_numpy(a).to(dev), resolution=res)) <= 1e-12


def check_set_scores(name, dev):
    g, r = R.case_sets(name)
    tg, tr = torch.from_numpy(g).to(dev), torch.from_numpy(r).to(dev)
    ab, ba = E.chamfer_matrix(tg, tr)
    self_ab, self_ba = E.chamfer_matrix(tg, tg)
    assert torch.equal(self_ba, self_ab.t())     # the formula of a pair is symmetric bit for bit
    gg, rr = self_ab + self_ba, sum(E.chamfer_matrix(tr, tr))
    want_gr, want_gg, want_rr = sum(R.chamfer_matrix(g, r)), sum(R.chamfer_matrix(g, g)), sum(R.chamfer_matrix(r, r))
    # no arg-minimum is in doubt: the two best entries of every row are much further apart than the rounding
    union = np.block([[want_gg + np.diag([np.inf] * len(g)), want_gr], [want_gr.T, want_rr + np.diag([np.inf] * len(r))]])
    gap = min(R.row_gap(want_gr), R.row_gap(union))
    print("%s: smallest relative gap between a row's two best entries %.3g" % (name, gap))
    assert gap > 100 * R.DIST_RTOL
    mmd, cov = E.mmd_cov(ab, ba)
    want_mmd, want_cov = R.mmd_cov(want_gr)
    assert abs(mmd - want_mmd) <= R.DIST_RTOL * want_mmd and cov == want_cov
    assert E.one_nn_accuracy(gg, ab + ba, rr) == R.one_nn_accuracy(want_gg, want_gr, want_rr)
    # numpy matrices are accepted too
    mmd_np, cov_np = E.mmd_cov(ab.cpu().numpy(), ba.cpu().numpy())
    assert abs(mmd_np - mmd) <= 1e-15 * mmd and cov_np == cov
    scores = E.evaluate(tg, tr)
    assert scores["mmd_cd"] == mmd and scores["cov_cd"] == cov
    assert scores["one_nna_cd"] == R.one_nn_accuracy(want_gg, want_gr, want_rr)
    assert abs(scores["jsd"] - E.jsd(tg, tr)) <= 1e-15


def assert_scores_match(scores, g, r, resolution=28):
    """`scores` of float32 clouds g against r equal the float64 reference's: MMD within the distance bound, COV and 1-NNA
    exactly, JSD at 1e-12 when no histogram point is fragile and within R.jsd_bound of the fragile counts otherwise."""
    want = R.evaluate(g, r, resolution)
    fragile = R.occupancy(g, resolution)[2], R.occupancy(r, resolution)[2]
    jsd_bound = R.jsd_bound(fragile[0], g.shape[0] * g.shape[1], fragile[1], r.shape[0] * r.shape[1], resolution ** 3)
    print("scores", scores, "reference", want, "fragile histogram points", fragile, "jsd bound %.3g" % jsd_bound)
    assert set(scores) == {"mmd_cd", "cov_cd", "one_nna_cd", "jsd"}
    assert abs(scores["mmd_cd"] - want["mmd_cd"]) <= R.DIST_RTOL * want["mmd_cd"]
    assert scores["cov_cd"] == want["cov_cd"] and scores["one_nna_cd"] == want["one_nna_cd"]
    assert abs(scores["jsd"] - want["jsd"]) <= jsd_bound


# ---- the CPU tier ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_chamfer_matrix_matches_float64(name):
    check_matrix(name, "cpu")


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_nearest_matches_float64(name):
    check_nearest(name, "cpu")


def test_exact_ties_take_the_lowest_index():
    check_ties("cpu")


def test_non_finite_points_stay_in_range():
    check_non_finite("cpu")


@pytest.mark.parametrize("name,res", [("2048x2048", 28), ("513x700", 28), ("64x33", 5), ("1x1", 2)])
def test_histogram_and_jsd_match_float64(name, res):
    check_histogram(name, res, "cpu")


@pytest.mark.parametrize("name", ["513x700", "64x33"])
def test_set_scores_match_float64(name):
    check_set_scores(name, "cpu")


def test_mmd_cov_known_answers():
    d = np.array([[1.0, 5.0, 3.0], [2.0, 0.5, 4.0]])
    mmd, cov = E.mmd_cov(d / 4, 3 * d / 4)
    assert mmd == (1.0 + 0.5 + 3.0) / 3 and cov == 2 / 3
    mmd, cov = E.mmd_cov(torch.tensor([[4.0, 1.0], [5.0, 2.0], [6.0, 3.0]]), torch.zeros(3, 2))
    assert mmd == 2.5 and cov == 0.5         # every generated cloud picks dataset cloud 1
    assert E.mmd_cov(np.eye(4) * -1 + 1, np.zeros((4, 4))) == (0.0, 1.0)


def test_one_nn_accuracy_known_answers():
    unit = np.array([[0.0, 1.0], [1.0, 0.0]])
    assert E.one_nn_accuracy(unit, np.array([[5.0, 6.0], [7.0, 8.0]]), unit) == 1.0       # two far-apart clusters
    assert E.one_nn_accuracy(unit, np.array([[0.1, 6.0], [7.0, 8.0]]), unit) == 0.5       # g0 and r0 find each other
    assert E.one_nn_accuracy(unit * 9, np.full((2, 2), 0.5), unit * 9) == 0.0             # always the other set
    # the diagonal (a cloud against itself) never counts, whatever it holds
    assert E.one_nn_accuracy(unit - 5 * np.eye(2), np.array([[5.0, 6.0], [7.0, 8.0]]), unit) == 1.0
    assert R.one_nn_accuracy(unit, np.array([[0.1, 6.0], [7.0, 8.0]]), unit) == 0.5
    with pytest.raises(ValueError):
        E.one_nn_accuracy(unit, np.zeros((2, 3)), unit)


def test_jsd_known_answers():
    assert E.jsd_of_histograms([1, 0, 0, 0], [0, 0, 0, 7]) == 1.0                          # disjoint supports: one bit
    assert E.jsd_of_histograms([3, 1], [6, 2]) == 0.0
    corner = np.array([[[-0.5, -0.5, -0.5], [0.5, 0.5, 0.5], [9.0, -9.0, 0.0]]], dtype=np.float32)
    h = E.occupancy_histogram(torch.from_numpy(corner), 3).numpy()
    assert h[0, 0, 0] == 1 and h[2, 2, 2] == 1 and h[2, 0, 1] == 1 and h.sum() == 3        # outside points go to the border cell


def test_inputs_are_checked():
    a = torch.zeros((2, 5, 3))
    with pytest.raises(ValueError):
        E.chamfer_matrix(torch.zeros((2, 5, 2)), a)
    with pytest.raises(ValueError):
        E.nearest_neighbours(a, torch.zeros((3, 5, 3)))
    with pytest.raises(ValueError):
        E.chamfer_matrix(torch.zeros((0, 5, 3)), a)
    # a single cloud [P, 3] is a batch of one; a numpy array goes to the device of the tensor it is paired with
    ab, ba = E.chamfer_matrix(a[0], np.zeros((2, 5, 3)))
    assert ab.shape == (1, 2) and ab.device.type == "cpu"


def test_evaluate_matches_float64_end_to_end():
    g, r = R.make_set(7, 300, 31), R.make_set(9, 257, 32, first_kind=2)
    assert_scores_match(E.evaluate(torch.from_numpy(g), torch.from_numpy(r)), g, r)
