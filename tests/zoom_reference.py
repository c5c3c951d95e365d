"""Cubic B-spline zoom and sampling in numpy (K20 of include/shapegan_hip.h), restated from the definition and from nothing else: no
scipy, no code of the package.  float64 by default; `dtype=np.float32` runs the same steps in single precision, which is how the
tolerance of tests/zoom_cases.py was measured.

The definition is scipy.ndimage.zoom / map_coordinates at their defaults (tests/golden/zoom_scipy.npz pins that, test_zoom.py)."""
import numpy as np


def prefilter_axis(c, axis, dtype):
    """The line filter along one axis of an array, every line at once."""
    c = np.moveaxis(c, axis, 0).astype(dtype).copy()
    n = c.shape[0]
    if n == 1:
        return np.moveaxis(c, 0, axis)
    z = dtype(np.sqrt(3.0) - 2.0)
    c *= dtype(6)
    zn = dtype(z ** (n - 1))
    c0 = c[0] + zn * c[n - 1]
    zi = z
    for i in range(1, n - 1):
        c0 = c0 + zi * (c[i] + zn * c[n - 1 - i])
        zi = dtype(zi * z)
    c[0] = c0 / (dtype(1) - zn * zn)
    for i in range(1, n):
        c[i] += z * c[i - 1]
    c[n - 1] = (z * c[n - 2] + c[n - 1]) * (z / (z * z - dtype(1)))
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return np.moveaxis(c, 0, axis)


def prefilter(grids, dtype=np.float64):
    """Coefficients of grids [..., D, H, W]: along W, then H, then D."""
    c = np.asarray(grids).astype(dtype)
    for axis in (-1, -2, -3):
        c = prefilter_axis(c, axis, dtype)
    return c


def mirror(i, n):
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def weights(t, order, dtype):
    t = t.astype(dtype)
    one, six = dtype(1), dtype(6)
    if order == 1:
        return np.stack([np.zeros_like(t), one - t, t, np.zeros_like(t)])
    return np.stack([(one - t) ** 3 / six, (3 * t ** 3 - 6 * t ** 2 + 4) / six, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / six, t ** 3 / six]).astype(dtype)


def dweights(t, dtype):
    t = t.astype(dtype)
    return np.stack([-(1 - t) ** 2 / 2, (9 * t ** 2 - 12 * t) / 6, (-9 * t ** 2 + 6 * t + 3) / 6, t ** 2 / 2]).astype(dtype)


def zoom_coordinates(n, N, dtype):
    """(f [N] int, t [N]) of the output indices of an axis: o (n - 1) / (N - 1) in integers."""
    if N == 1:
        return np.zeros(1, np.int64), np.zeros(1, dtype)
    num = np.arange(N, dtype=np.int64) * (n - 1)
    return num // (N - 1), (num % (N - 1)).astype(dtype) / dtype(N - 1)


def axis_matrix(n, f, w, dtype):
    """[len(f), n]: row o holds the weights w[:, o] at the mirror-folded taps f[o] - 1 .. f[o] + 2 (taps that fold onto one index add)."""
    m = np.zeros((len(f), n), dtype)
    for k in range(4):
        np.add.at(m, (np.arange(len(f)), mirror(f - 1 + k, n)), w[k])
    return m


def zoom(grid, size, order=3, dtype=np.float64):
    """One grid [D, H, W] -> [D', H', W']."""
    grid = np.asarray(grid)
    c = prefilter(grid, dtype) if order == 3 else grid.astype(dtype)
    out = c
    for axis, (n, N) in enumerate(zip(grid.shape, size)):
        f, t = zoom_coordinates(n, N, dtype)
        m = axis_matrix(n, f, weights(t, order, dtype), dtype)
        out = np.moveaxis(np.tensordot(m, out, axes=([1], [axis])), 0, axis)
    return out.astype(dtype)


def zoom_size(shape, factor):
    return tuple(int(round(n * factor)) for n in shape)


def sample(grid, points, outside=1.0, dtype=np.float64, coefficients=None):
    """(values [P], gradient [P, 3]) of one grid [D, H, W] at points [P, 3] in index coordinates."""
    grid = np.asarray(grid)
    c = prefilter(grid, dtype) if coefficients is None else coefficients
    pts = np.asarray(points).astype(dtype)
    P = len(pts)
    inside = np.ones(P, bool)
    per_axis = []
    for a, n in enumerate(grid.shape):
        x = pts[:, a]
        with np.errstate(invalid="ignore"):
            inside &= (x >= 0) & (x <= n - 1)
        xs = np.where(np.isfinite(x), x, 0).clip(0, n - 1)
        f = np.minimum(np.floor(xs).astype(np.int64), max(n - 2, 0))
        t = xs - f
        per_axis.append((np.stack([mirror(f - 1 + k, n) for k in range(4)]), weights(t, 3, dtype), dweights(t, dtype)))
    (idd, wd, dd), (ih, wh, dh), (iw, ww, dw) = per_axis
    values = np.zeros(P, dtype)
    grad = np.zeros((P, 3), dtype)
    for i in range(4):
        for j in range(4):
            for k in range(4):
                v = c[idd[i], ih[j], iw[k]]
                values += wd[i] * wh[j] * ww[k] * v
                grad[:, 0] += dd[i] * wh[j] * ww[k] * v
                grad[:, 1] += wd[i] * dh[j] * ww[k] * v
                grad[:, 2] += wd[i] * wh[j] * dw[k] * v
    values[~inside] = outside
    grad[~inside] = 0
    return values, grad
