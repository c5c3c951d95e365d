"""Float64 brute-force references of K19 (signed distances from oriented point clouds), written from the contract of
include/shapegan_hip.h alone: numpy only, nothing of the package.

Clouds and queries are ragged: points [N, 3] with offsets [S + 1].  Every function takes float32 or float64 arrays and computes in float64."""
import numpy as np


def pair_d2(queries, cloud):
    """[Q, P] float64 squared distances; a non-finite one is +inf (never a neighbour)."""
    q, p = np.asarray(queries, dtype=np.float64), np.asarray(cloud, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = ((q[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
    d[~np.isfinite(d)] = np.inf
    return d


def knn(points, cloud_offsets, queries, query_offsets, K, exclude_self=False, extra=0):
    """(idx [M, K + extra] int64, d2 [M, K + extra] float64): per query the first points of its shape's cloud in the order (d2, index);
    -1 / +inf beyond the neighbours there are.  extra: further columns of the same order (the gap behind the K-th)."""
    S, M, W = len(cloud_offsets) - 1, len(queries), K + extra
    idx, d2 = np.full((M, W), -1, dtype=np.int64), np.full((M, W), np.inf)
    for s in range(S):
        c0, c1, q0, q1 = (int(v) for v in (cloud_offsets[s], cloud_offsets[s + 1], query_offsets[s], query_offsets[s + 1]))
        if q1 == q0 or c1 == c0:
            continue
        d = pair_d2(queries[q0:q1], points[c0:c1])
        if exclude_self:
            assert q1 - q0 == c1 - c0
            d[np.arange(q1 - q0), np.arange(c1 - c0)] = np.inf
        order = np.argsort(d, axis=1, kind="stable")[:, :W]      # stable: equal distances stay in index order
        best = np.take_along_axis(d, order, axis=1)
        w = order.shape[1]
        idx[q0:q1, :w] = np.where(np.isfinite(best), order, -1)
        d2[q0:q1, :w] = best
    return idx, d2


def neighbourhoods(points, cloud_offsets, idx):
    """Per point the float64 covariance sums [N, 3, 3] of its samples (itself and its valid neighbours, relative to the point, about their
    centroid) and the number of samples [N]."""
    p = np.asarray(points, dtype=np.float64)
    N = len(p)
    cov, count = np.zeros((N, 3, 3)), np.zeros(N, dtype=np.int64)
    for s in range(len(cloud_offsets) - 1):
        c0, c1 = int(cloud_offsets[s]), int(cloud_offsets[s + 1])
        for i in range(c0, c1):
            nb = idx[i][(idx[i] >= 0) & (idx[i] < c1 - c0)]
            q = np.concatenate([np.zeros((1, 3)), p[c0 + nb] - p[i]])
            e = q - q.mean(axis=0)
            cov[i], count[i] = e.T @ e, len(q)
    return cov, count


def normals(points, cloud_offsets, idx):
    """(normal [N, 3] — the unit eigenvector of the smallest eigenvalue, sign free —, eigenvalues [N, 3] ascending, samples [N])."""
    cov, count = neighbourhoods(points, cloud_offsets, idx)
    w, v = np.linalg.eigh(cov)
    return v[:, :, 0], w, count


def orient(normal, points, view):
    """The contract's orientation of float64 unit normals: view [N, 4] per point, or None (largest component positive, lowest axis on a tie)."""
    n = np.array(normal, dtype=np.float64)
    if view is None:
        big = np.argmax(np.abs(n), axis=1)
        flip = n[np.arange(len(n)), big] < 0
    else:
        v = np.asarray(view, dtype=np.float64)
        flip = (n * (v[:, :3] - v[:, 3:4] * np.asarray(points, dtype=np.float64))).sum(axis=1) < 0
    n[flip] *= -1
    return n


def sdf(points, point_normals, cloud_offsets, queries, query_offsets, K):
    """(sdf [M] float64, nearest [M] int64): knn -> gather -> vote."""
    idx, d2 = knn(points, cloud_offsets, queries, query_offsets, K)
    p, n, q = (np.asarray(a, dtype=np.float64) for a in (points, point_normals, queries))
    out, nearest = np.full(len(q), np.inf), np.full(len(q), -1, dtype=np.int64)
    for s in range(len(cloud_offsets) - 1):
        c0, q0, q1 = int(cloud_offsets[s]), int(query_offsets[s]), int(query_offsets[s + 1])
        for i in range(q0, q1):
            nb = idx[i][idx[i] >= 0]
            if not len(nb):
                continue
            t = ((q[i] - p[c0 + nb]) * n[c0 + nb]).sum(axis=1)
            inside = 2 * int((t < 0).sum()) > len(nb)
            out[i], nearest[i] = (-1 if inside else 1) * np.sqrt(d2[i, 0]), idx[i, 0]
    return out, nearest


def fibonacci_sphere(count, radius=0.5):
    i = np.arange(count, dtype=np.float64)
    y = 1.0 - (2.0 * i + 1.0) / count
    r = np.sqrt(1.0 - y * y)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), y, r * np.sin(phi)], axis=1) * radius
