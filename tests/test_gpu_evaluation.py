"""Point-cloud evaluation on the MI355X (csrc/pointcloud.hip): the bodies of test_evaluation.py on the device against the float64
reference, the kernels against the C++ twin bit for bit, and `evaluate` end to end on clouds sampled from voxel grids."""
import numpy as np
import pytest
import torch

from shapegan_amd import evaluation as E
from shapegan_amd import metrics
import evaluation_reference as R
import test_evaluation as T
from test_mesh import sphere_grid, torus_grid

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_chamfer_matrix_matches_float64(name):
    T.check_matrix(name, "cuda")


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_nearest_matches_float64(name):
    T.check_nearest(name, "cuda")


def test_exact_ties_take_the_lowest_index():
    T.check_ties("cuda")


def test_non_finite_points_stay_in_range():
    T.check_non_finite("cuda")


@pytest.mark.parametrize("name,res", [("2048x2048", 28), ("513x700", 28), ("64x33", 5), ("1x1", 2)])
def test_histogram_and_jsd_match_float64(name, res):
    T.check_histogram(name, res, "cuda")


@pytest.mark.parametrize("name", ["513x700", "64x33"])
def test_set_scores_match_float64(name):
    T.check_set_scores(name, "cuda")


# ---- GPU against twin: the same bits ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_gpu_equals_twin_bit_for_bit(name):
    a, b = R.case_sets(name)
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    # include/shapegan_hip.h: one summation order for both, so the float64 means are equal too
    for gpu, cpu in zip(E.chamfer_matrix(ta.cuda(), tb.cuda()), E.chamfer_matrix(ta, tb)):
        np.testing.assert_array_equal(gpu.cpu().numpy(), cpu.numpy())
    pa, pb = (torch.from_numpy(x) for x in T.all_pairs(a, b))
    for gpu, cpu in zip(E.nearest_neighbours(pa.cuda(), pb.cuda()), E.nearest_neighbours(pa, pb)):
        np.testing.assert_array_equal(gpu.cpu().numpy(), cpu.numpy())
    for res in (28, 7):
        np.testing.assert_array_equal(E.occupancy_histogram(ta.cuda(), res).cpu().numpy(), E.occupancy_histogram(ta, res).numpy())


def test_gpu_equals_twin_on_ties():
    a, b = (torch.from_numpy(np.stack([x])) for x in R.duplicate_clouds())
    for x, y in ((a, a), (a, b), (b, a)):
        for gpu, cpu in zip(E.nearest_neighbours(x.cuda(), y.cuda()), E.nearest_neighbours(x, y)):
            np.testing.assert_array_equal(gpu.cpu().numpy(), cpu.numpy())


def sub_block_equals_twin(a, b, seed, n=5):
    """chamfer_matrix of all of a against all of b on the device; an n x n sub-block of sampled rows and columns is compared bit
    for bit with the twin run on those clouds alone.  Returns the device matrices."""
    ab, ba = E.chamfer_matrix(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    rng = np.random.default_rng(seed)
    rows, cols = np.sort(rng.choice(len(a), n, replace=False)), np.sort(rng.choice(len(b), n, replace=False))
    want_ab, want_ba = E.chamfer_matrix(torch.from_numpy(a[rows]), torch.from_numpy(b[cols]))
    np.testing.assert_array_equal(ab.cpu().numpy()[np.ix_(rows, cols)], want_ab.numpy())
    np.testing.assert_array_equal(ba.cpu().numpy()[np.ix_(rows, cols)], want_ba.numpy())
    return ab, ba


def test_many_clouds_per_row_match_twin_on_a_sub_block():
    """40 x 40 clouds of 2048 points: B does not fit the LDS stage at once, every row is split along B into 40 workgroups of one
    cloud each.  Compared with the twin on a sampled 5 x 5 sub-block (the twin takes a second per entry of this size)."""
    a, b = R.make_set(40, 2048, 41), R.make_set(40, 2048, 42, first_kind=2)
    ab, ba = sub_block_equals_twin(a, b, 43)
    # the rows computed in three calls are the rows computed in one
    ab3, ba3 = E.chamfer_matrix(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), chunk=17)
    assert torch.equal(ab, ab3) and torch.equal(ba, ba3)


# The walk of ONE workgroup over SEVERAL clouds of B (the loop the 1000 x 1000 numbers come from: the LDS stage refilled after the
# barrier, the running minima reset, the float64 tree reused, one partial sum stored per cloud).  chamfer_sweep gives a row
# ceil(4096 / (rows x tiles)) workgroups, at most one per cloud of B, so it takes rows x tiles x clouds of B well above 4096; the
# shares of a row are [z Sb / split, (z + 1) Sb / split).  Both sweeps (ab, and ba with the roles exchanged) are listed.
@pytest.mark.parametrize("Sa,Sb,P,Q,shares", [
    (100, 100, 2048, 2048, "41 shares of 2 or 3 clouds, both sweeps"),
    (40, 200, 2048, 2048, "ab: 103 shares of 1 or 2 of 200; ba: 21 shares of 1 or 2 of 40"),
    (300, 260, 700, 513, "ab: 14 shares of 18 or 19 of 260; ba: 16 shares of 18 or 19 of 300; stages that end inside a group of 4"),
])
def test_workgroups_that_walk_several_clouds_match_twin_on_a_sub_block(Sa, Sb, P, Q, shares):
    for rows, cols in ((Sa, Sb), (Sb, Sa)):
        split = min(-(-4096 // rows), cols)          # one tile per cloud here
        assert split < cols and cols % split, "the case is meant to have uneven shares of several clouds"
    a, b = R.make_set(Sa, P, 61 + Sa), R.make_set(Sb, Q, 62 + Sb, first_kind=1)
    ab, ba = sub_block_equals_twin(a, b, 63 + Sa)
    ab3, ba3 = E.chamfer_matrix(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), chunk=Sa // 3 + 1)
    assert torch.equal(ab, ab3) and torch.equal(ba, ba3)     # other shares (fewer rows per call), the same bits


def test_one_workgroup_walks_a_whole_row():
    """More than 4096 rows: no split, every workgroup of the ab sweep walks all 7 clouds of B; the full matrices against the twin."""
    a, b = R.make_set(4200, 64, 71), R.make_set(7, 33, 72, first_kind=3)
    for gpu, cpu in zip(E.chamfer_matrix(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()),
                        E.chamfer_matrix(torch.from_numpy(a), torch.from_numpy(b))):
        np.testing.assert_array_equal(gpu.cpu().numpy(), cpu.numpy())


def test_clouds_longer_than_one_tile_match_twin():
    """P and Q beyond 2048: several register tiles of A per cloud and several LDS stages per cloud of B."""
    a, b = R.make_set(3, 5000, 51), R.make_set(2, 4100, 52, first_kind=1)
    for gpu, cpu in zip(E.chamfer_matrix(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()),
                        E.chamfer_matrix(torch.from_numpy(a), torch.from_numpy(b))):
        np.testing.assert_array_equal(gpu.cpu().numpy(), cpu.numpy())
    for gpu, cpu in zip(E.nearest_neighbours(torch.from_numpy(a[:2]).cuda(), torch.from_numpy(b).cuda()),
                        E.nearest_neighbours(torch.from_numpy(a[:2]), torch.from_numpy(b))):
        np.testing.assert_array_equal(gpu.cpu().numpy(), cpu.numpy())


# ---- end to end --------------------------------------------------------------------------------------------------------------
def test_evaluate_on_sampled_voxel_grids_matches_float64():
    """metrics.sample_from_voxels -> evaluate: 16 sphere clouds against 16 torus clouds of 1024 points, float64 numpy in,
    scores equal to the float64 reference on the same clouds."""
    torch.manual_seed(5)
    spheres = np.stack([sphere_grid(32, 0.45 + 0.02 * i) for i in range(16)])
    tori = np.stack([torus_grid(32, 0.5, 0.12 + 0.01 * i) for i in range(16)])
    g = metrics.sample_from_voxels(spheres, 1024)
    r = metrics.sample_from_voxels(tori, 1024)
    assert g.dtype == np.float64 and g.shape == (16, 1024, 3)
    scores = E.evaluate(g, r)
    g32, r32 = g.astype(np.float32), r.astype(np.float32)        # the cast evaluate makes: the reference sees the same points
    T.assert_scores_match(scores, g32, r32)
    assert scores["one_nna_cd"] == 1.0 and scores["jsd"] > 0.1      # spheres and tori are told apart
