"""Float64 numpy statement of the point-cloud evaluation quantities (include/shapegan_hip.h, K13; shapegan_amd/evaluation.py).

Written from the header's text, brute force: every pair's squared distance in float64, minima and arg-minima over the full
[P, Q] table, the histogram by the nearest grid centre.  Shares no code with the package.  Also the seeded inputs of the tests
and the `fragile` sets: the points whose answer the float32 rounding of the kernels may legitimately change.
"""
import numpy as np

U = 2.0 ** -24                    # unit roundoff of float32
DIST_RTOL = 6 * U                 # |fl(d2) - d2| <= 5 u d2 (three differences, one product, two fused steps); a minimum keeps it
INDEX_FRAGILE_RTOL = 12 * U       # best and runner-up closer than twice that: either may win in float32
HIST_FRAGILE = 4 * U              # x R: distance (in cells) from a cell boundary below which float32 may pick the other cell
FRAGILE_CAP = 1e-3                # share of points that may be left out of an exact comparison


# ---- seeded inputs --------------------------------------------------------------------------------------------------------
def make_cloud(kind, n, rng):
    """float32 [n, 3]: 0 sphere surface of radius 0.2-0.5, 1 torus, 2 box volume, 3 Gaussian blob; shifted by about 0.02."""
    kind = kind % 4
    if kind == 0:
        v = rng.normal(size=(n, 3))
        p = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.2, 0.5)
    elif kind == 1:
        u, w = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
        R, r = rng.uniform(0.25, 0.35), rng.uniform(0.05, 0.12)
        p = np.stack([(R + r * np.cos(w)) * np.cos(u), r * np.sin(w), (R + r * np.cos(w)) * np.sin(u)], axis=1)
    elif kind == 2:
        p = rng.uniform(-1, 1, size=(n, 3)) * rng.uniform(0.15, 0.45, size=3)
    else:
        p = rng.normal(size=(n, 3)) * rng.uniform(0.08, 0.2)
    return (p + rng.normal(size=3) * 0.02).astype(np.float32)


def make_set(count, n, seed, first_kind=0):
    rng = np.random.default_rng(seed)
    return np.stack([make_cloud(first_kind + s, n, rng) for s in range(count)])


CASES = {"2048x2048": (2048, 2048, 4, 4), "513x700": (513, 700, 6, 5), "64x33": (64, 33, 8, 8), "1x1": (1, 1, 1, 1)}


def case_sets(name):
    P, Q, Sa, Sb = CASES[name]
    seed = sorted(CASES).index(name)
    return make_set(Sa, P, 100 + seed), make_set(Sb, Q, 200 + seed, first_kind=1)


def duplicate_clouds():
    """a: 300 points of which [100, 150) repeat [0, 50) exactly; b: 200 points, [150, 200) repeat [20, 70) and [0, 10) are
    points of a: comparing them (and a with itself) has zero distances and exact index ties."""
    rng = np.random.default_rng(7)
    a = make_cloud(2, 300, rng)
    a[100:150] = a[0:50]
    b = make_cloud(3, 200, rng)
    b[0:10] = a[60:70]
    b[150:200] = b[20:70]
    return a, b


# ---- Chamfer --------------------------------------------------------------------------------------------------------------
def pair_table(a, b):
    """[P, Q] float64 squared distances."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.zeros((a.shape[0], b.shape[0]))
    for c in range(3):
        d += (a[:, c, None] - b[None, :, c]) ** 2
    return d


def nearest_rows(d):
    """Per row of the table: minimum, lowest arg-minimum, fragile flag (a strictly larger entry within INDEX_FRAGILE_RTOL of it)."""
    best = d.min(axis=1)
    arg = d.argmin(axis=1)                                        # the first occurrence: the lowest index of a tie
    above = np.where(d > best[:, None], d, np.inf).min(axis=1)      # the smallest entry that is not a tie
    fragile = np.isfinite(above) & ((above - best) <= INDEX_FRAGILE_RTOL * np.where(np.isfinite(above), above, 0.0))
    return best, arg, fragile


def nearest(a, b):
    """(dist_a, idx_a, fragile_a, dist_b, idx_b, fragile_b) for one pair of clouds."""
    d = pair_table(a, b)
    return nearest_rows(d) + nearest_rows(d.T.copy())


def chamfer_matrix(A, B):
    ab = np.zeros((len(A), len(B)))
    ba = np.zeros((len(A), len(B)))
    for i in range(len(A)):
        for j in range(len(B)):
            d = pair_table(A[i], B[j])
            ab[i, j] = d.min(axis=1).mean()
            ba[i, j] = d.min(axis=0).mean()
    return ab, ba


# ---- set scores -----------------------------------------------------------------------------------------------------------
def mmd_cov(d):
    """d [G, R]: rows generated, columns dataset."""
    G, R = d.shape
    mmd = sum(min(d[g, r] for g in range(G)) for r in range(R)) / R
    matched = set()
    for g in range(G):
        matched.add(min(range(R), key=lambda r: d[g, r]))
    return mmd, len(matched) / R


def one_nn_accuracy(d_gg, d_gr, d_rr):
    G, R = d_gr.shape
    right = 0
    for g in range(G):
        same = min(d_gg[g, o] for o in range(G) if o != g) if G > 1 else np.inf
        other = min(d_gr[g, r] for r in range(R))
        right += same <= other        # an exact tie goes to the generated set, listed first in the union
    for r in range(R):
        same = min(d_rr[r, o] for o in range(R) if o != r) if R > 1 else np.inf
        other = min(d_gr[g, r] for g in range(G))
        right += same < other
    return right / (G + R)


def row_gap(d):
    """Smallest relative gap between the two best entries of a row (inf for one column): how safe the arg-minima are."""
    if d.shape[1] < 2:
        return np.inf
    s = np.sort(d, axis=1)
    return float(((s[:, 1] - s[:, 0]) / s[:, 1]).min())


# ---- occupancy histogram and JSD ------------------------------------------------------------------------------------------
def occupancy(clouds, R):
    """(hist [R,R,R] int64 by nearest centre, fragile [R,R,R] int64: per cell the points within HIST_FRAGILE * R cells of a
    boundary between two cells of the grid, number of fragile points)."""
    pts = np.asarray(clouds, dtype=np.float64).reshape(-1, 3)
    centres = -0.5 + np.arange(R) / (R - 1)
    idx = np.abs(pts[:, :, None] - centres[None, None, :]).argmin(axis=2)              # [n, 3]
    t = (pts + 0.5) * (R - 1) + 0.5                                                   # boundaries at the integers 1 .. R-1
    k = np.rint(t)
    near = (np.abs(t - k) <= HIST_FRAGILE * R) & (k >= 1) & (k <= R - 1)
    frag = near.any(axis=1)
    hist = np.zeros((R, R, R), dtype=np.int64)
    np.add.at(hist, (idx[:, 0], idx[:, 1], idx[:, 2]), 1)
    fragile = np.zeros((R, R, R), dtype=np.int64)
    np.add.at(fragile, (idx[frag, 0], idx[frag, 1], idx[frag, 2]), 1)
    return hist, fragile, int(frag.sum())


def neighbourhood_sum(x):
    """Per cell the sum over the cell and its 26 neighbours."""
    p = np.pad(x, 1)
    out = np.zeros_like(x)
    n = x.shape[0]
    for a in range(3):
        for b in range(3):
            for c in range(3):
                out += p[a:a + n, b:b + n, c:c + n]
    return out


def jsd(ha, hb):
    p = np.asarray(ha, dtype=np.float64).ravel()
    q = np.asarray(hb, dtype=np.float64).ravel()
    p, q = p / p.sum(), q / q.sum()
    m = (p + q) / 2

    def kl(x, y):
        keep = x > 0
        return float((x[keep] * np.log2(x[keep] / y[keep])).sum())

    return (kl(p, m) + kl(q, m)) / 2


def _entropy_shift(t, cells):
    """Most the base-2 entropy of a distribution over `cells` cells can change when it moves by the total variation t <= 1/2:
    t log2(cells - 1) + h(t), h the binary entropy (the sharp form of Fannes' inequality: Audenaert 2007, Zhang 2007)."""
    if t <= 0:
        return 0.0
    t = min(t, 0.5)
    return t * np.log2(max(cells - 1, 2)) + (-t * np.log2(t) - (1 - t) * np.log2(1 - t))


def jsd_bound(fragile_a, points_a, fragile_b, points_b, cells):
    """How far the JSD of two histograms may be from the reference's when `fragile_a` of the `points_a` points of the first and
    `fragile_b` of the `points_b` of the second may each sit in a neighbouring cell.  1e-12 (float64 rounding of the sums) when
    no point is fragile.  Otherwise: k moved points shift a histogram's distribution p by a total variation of at most k / n,
    the mixture m = (p + q) / 2 by at most the mean of the two, and JSD = H(m) - (H(p) + H(q)) / 2 by the entropy shifts."""
    ta, tb = fragile_a / points_a, fragile_b / points_b
    return 1e-12 + _entropy_shift((ta + tb) / 2, cells) + (_entropy_shift(ta, cells) + _entropy_shift(tb, cells)) / 2


def evaluate(G, R, resolution=28):
    ab, ba = chamfer_matrix(G, R)
    gg = sum(chamfer_matrix(G, G))
    rr = sum(chamfer_matrix(R, R))
    mmd, cov = mmd_cov(ab + ba)
    return {"mmd_cd": mmd, "cov_cd": cov, "one_nna_cd": one_nn_accuracy(gg, ab + ba, rr),
            "jsd": jsd(occupancy(G, resolution)[0], occupancy(R, resolution)[0])}
