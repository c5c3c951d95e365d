"""Float64 statement of what shapegan_amd/prepare.py computes, and the procedural meshes its tests use.

Meshes (closed, consistently oriented, outward): icosphere (2 subdivisions, 320 triangles, r = 0.8), torus (R = 0.55, r = 0.2, 32 x 16
quads), box (half extents 0.5, 0.3, 0.4).  All lie inside the unit sphere.
Reference: the brute-force closest point of every (point, triangle) pair in float64, on the float32 coordinates the kernels see; for
the sign of these meshes the generalised winding number (Van Oosterom & Strackee's solid angle per triangle).

Bound of the distance tests: |sqrtf(dist2) - reference| <= 16 * 2^-24 ABSOLUTE on coordinates inside [-1, 1]^3: two float32
formulations of the closest point were measured at 1.0 - 1.6 x 2^-24 on exactly these inputs, the factor of ten covers another order of
operations and the fused steps.
"""
import functools

import numpy as np

U = 2.0 ** -24
DIST_ATOL = 16 * U


# ---- meshes ----------------------------------------------------------------------------------------------------------------------------
def icosphere(subdivisions=2, radius=0.8):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        cache, out = {}, []

        def mid(i, j):
            key = (min(i, j), max(i, j))
            if key not in cache:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]

        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.asarray(v) * radius, np.asarray(f, dtype=np.int64)


def torus(R=0.55, r=0.2, nu=32, nv=16):
    a = np.arange(nu) * (2 * np.pi / nu)
    b = np.arange(nv) * (2 * np.pi / nv)
    A, B = np.meshgrid(a, b, indexing="ij")
    v = np.stack([(R + r * np.cos(B)) * np.cos(A), r * np.sin(B), (R + r * np.cos(B)) * np.sin(A)], axis=-1).reshape(-1, 3)
    f = []
    for i in range(nu):
        for j in range(nv):
            p00, p10, p01, p11 = i * nv + j, ((i + 1) % nu) * nv + j, i * nv + (j + 1) % nv, ((i + 1) % nu) * nv + (j + 1) % nv
            f += [(p00, p01, p11), (p00, p11, p10)]
    return v, np.asarray(f, dtype=np.int64)


def box(half=(0.5, 0.3, 0.4)):
    v = np.asarray([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64) * np.asarray(half)
    f = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)]
    return v, np.asarray(f, dtype=np.int64)


MESHES = {"icosphere": icosphere, "torus": torus, "box": box}


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(vertices [V, 3] float64 holding float32 values, faces [F, 3]); outward orientation is asserted through the signed volume."""
    v, f = MESHES[name]()
    v = v.astype(np.float32).astype(np.float64)
    t = v[f]
    assert np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() > 0, name
    return v, f


def soup(name):
    v, f = mesh(name)
    return v[f].astype(np.float32)


def single_triangle():
    """One slender triangle (area 0.18 inside the unit sphere)."""
    return np.asarray([[-0.9, 0.0, 0.0], [0.9, 0.05, 0.0], [0.0, 0.2, 0.1]], dtype=np.float64), np.asarray([[0, 1, 2]], dtype=np.int64)


def with_degenerates(tris, seed):
    """tris [T, 3, 3] float32 plus four slivers (the third corner on the first edge, plus 1e-7) and two triangles whose corners are equal."""
    rng = np.random.RandomState(seed)
    extra = []
    for _ in range(4):
        a, b = rng.uniform(-0.7, 0.7, 3), rng.uniform(-0.7, 0.7, 3)
        extra.append([a, b, a + rng.uniform(0.2, 0.8) * (b - a) + 1e-7])
    for _ in range(2):
        p = rng.uniform(-0.7, 0.7, 3)
        extra.append([p, p, p])
    return np.concatenate([tris, np.asarray(extra, dtype=np.float32)]).astype(np.float32)


def random_soup(T, seed):
    """T small random triangles inside the unit cube, float32 [T, 3, 3]."""
    rng = np.random.RandomState(seed)
    centre = rng.uniform(-0.8, 0.8, (T, 1, 3))
    return (centre + rng.uniform(-0.1, 0.1, (T, 3, 3))).astype(np.float32)


def surface_samples(tris, count, rng):
    """`count` points on random triangles (by area) of tris [T, 3, 3], float64."""
    t = tris.astype(np.float64)
    area = np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1)
    pick = rng.choice(len(t), count, p=area / area.sum())
    u, w = rng.uniform(size=count), rng.uniform(size=count)
    flip = u + w > 1
    u, w = np.where(flip, 1 - u, u), np.where(flip, 1 - w, w)
    return t[pick, 0] + u[:, None] * (t[pick, 1] - t[pick, 0]) + w[:, None] * (t[pick, 2] - t[pick, 0])


def distance_queries(name, seed=0):
    """The query set of the distance tests: 1 500 uniform in [-1, 1]^3, 1 500 at N(0, 0.00025^2) from random surface points, 50 mesh
    vertices; float32 [3050, 3]."""
    rng = np.random.RandomState(seed)
    v, _ = mesh(name)
    near = surface_samples(soup(name), 1500, rng) + rng.normal(scale=0.00025, size=(1500, 3))
    return np.concatenate([rng.uniform(-1, 1, (1500, 3)), near, v[rng.choice(len(v), 50)]]).astype(np.float32)


# ---- float64 reference --------------------------------------------------------------------------------------------------------------
def _segment(p, o, e):
    """Closest points of the segments o + t e to the points p: p [Q, 1, 3], o, e [1, T, 3] -> [Q, T, 3]."""
    ee = (e * e).sum(-1)
    t = np.where(ee > 0, (((p - o) * e).sum(-1)) / np.where(ee > 0, ee, 1.0), 0.0)
    return o + np.clip(t, 0.0, 1.0)[..., None] * e


def closest_points(points, tris):
    """(distance [Q, T], closest [Q, T, 3]) of every pair in float64: the projection onto the plane where it falls inside the triangle,
    else the nearest of the three edges; triangles without area have edges only."""
    p = np.asarray(points, dtype=np.float64)[:, None, :]
    t = np.asarray(tris, dtype=np.float64)[None]
    a, b, c = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    best, best_d = None, None
    for o, e in ((a, b - a), (b, c - b), (c, a - c)):
        cand = _segment(p, o, e)
        d = np.linalg.norm(p - cand, axis=-1)
        if best is None:
            best, best_d = cand, d
        else:
            take = d < best_d
            best, best_d = np.where(take[..., None], cand, best), np.where(take, d, best_d)
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    ok = nn > 1e-24 * np.maximum(((b - a) ** 2).sum(-1) * ((c - a) ** 2).sum(-1), 1e-300)
    safe = np.where(ok, nn, 1.0)
    ap = p - a
    v = (np.cross(ap, c - a) * n).sum(-1) / safe
    w = (np.cross(b - a, ap) * n).sum(-1) / safe
    inside = ok & (v >= 0) & (w >= 0) & (v + w <= 1)
    cand = a + v[..., None] * (b - a) + w[..., None] * (c - a)
    d = np.linalg.norm(p - cand, axis=-1)
    take = inside & (d < best_d)
    return np.where(take, d, best_d), np.where(take[..., None], cand, best)


def winding_number(points, tris):
    """Generalised winding number [Q] of the points with respect to the oriented triangles (1 inside a closed outward mesh, 0 outside)."""
    p = np.asarray(points, dtype=np.float64)[:, None, :]
    t = np.asarray(tris, dtype=np.float64)[None]
    a, b, c = t[:, :, 0] - p, t[:, :, 1] - p, t[:, :, 2] - p
    la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
    num = (a * np.cross(b, c)).sum(-1)
    den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
    return (2.0 * np.arctan2(num, den)).sum(-1) / (4.0 * np.pi)


@functools.lru_cache(maxsize=None)
def distance_case(name):
    """(triangles with degenerates [T, 3, 3] f32, queries [Q, 3] f32, reference distance per pair [Q, T] f64): computed once, read-only."""
    tris = with_degenerates(soup(name), seed=7)
    queries = distance_queries(name)
    dist, _ = closest_points(queries, tris)
    for x in (tris, queries, dist):
        x.setflags(write=False)
    return tris, queries, dist


@functools.lru_cache(maxsize=None)
def sign_case(name):
    """(queries [4096, 3] f32 uniform in the unit sphere, float64 distance [4096], inside [4096] bool by the winding number)."""
    rng = np.random.RandomState(11)
    p = rng.uniform(-1, 1, (16384, 3))
    p = p[np.linalg.norm(p, axis=1) < 1][:4096].astype(np.float32)
    tris = soup(name)
    dist = np.concatenate([closest_points(p[i:i + 512], tris)[0].min(axis=1) for i in range(0, len(p), 512)])
    wn = np.concatenate([winding_number(p[i:i + 512], tris) for i in range(0, len(p), 512)])
    inside = wn > 0.5
    assert (np.abs(wn - inside) < 1e-6).all(), name       # closed and consistently oriented: the number is 0 or 1
    for x in (p, dist, inside):
        x.setflags(write=False)
    return p, dist, inside


# ---- the sign rule in numpy float32 (include/shapegan_hip.h, K16) ---------------------------------------------------------------------
def _fma(a, b, c):
    """fmaf of float32 values: the product of two float32 is exact in float64; the cases of the rule test have sums that are too."""
    with np.errstate(invalid="ignore"):
        return (np.float64(np.float32(a)) * np.float64(np.float32(b)) + np.float64(np.float32(c))).astype(np.float32)


def visible_rule(points, depth, vp, bias):
    """visible [Q] of one scan by the written formula: points [Q, 3] f32, depth [N, N] f32, vp [4, 4] float64."""
    M = np.asarray(vp, dtype=np.float64).astype(np.float32)
    x, y, z = (np.asarray(points, dtype=np.float32)[:, i] for i in range(3))
    c = [_fma(M[j, 2], z, _fma(M[j, 1], y, _fma(M[j, 0], x, np.broadcast_to(M[j, 3], x.shape)))) for j in range(3)]
    N = depth.shape[0]
    h = np.float32(0.5) * np.float32(N)
    with np.errstate(invalid="ignore"):
        fx, fy = _fma(c[0], h, h), _fma(c[1], -h, h)
        in_window = (fx >= 0) & (fx < N) & (fy >= 0) & (fy < N)
        ix, iy = np.where(in_window, fx, 0).astype(np.int64), np.where(in_window, fy, 0).astype(np.int64)
        t = depth[iy, ix]
        return ~in_window | (t == np.float32(1.0)) | (c[2] < (t - np.float32(bias)).astype(np.float32))
