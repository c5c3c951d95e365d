"""The distance transforms of K21 restated in float64 numpy, by brute force, from the contract in include/shapegan_hip.h (not from
csrc/edt_core.h): every site is found explicitly, and every voxel takes the minimum over ALL sites of its grid.

A site lives in index coordinates u (one real number per axis); a voxel p is at the integers; the squared distance between them is
sum over the axes of ((p - u) * spacing)^2, with the spacing the float32 the library is given.  `voxels`: the sites are the voxels
with v < level (`inside`) or !(v < level).  `crossings`: the sites are the points where a grid edge crosses the level; the header
defines the crossing's coordinate in float32, u = (float)a + t, t = (level - va) / (vb - va), so these two roundings are taken as they
are (they are the definition of WHERE the site is — the same bits marching cubes emits) and everything after them is float64."""
import numpy as np


def spacing3(spacing):
    s = (spacing,) * 3 if np.isscalar(spacing) else tuple(spacing)
    return np.array([np.float32(x) for x in s], dtype=np.float64)


def voxel_sites(grid, level, inside=True):
    """[N, 3] index coordinates (float64 integers) of the sites of the `voxels` transform, in linear-index order."""
    grid = np.asarray(grid, dtype=np.float32)
    below = grid < np.float32(level)
    return np.argwhere(below if inside else ~below).astype(np.float64)


def crossing_sites(grid, level):
    """[N, 3] index coordinates of the crossings of `level` on the edges of the grid: float32 values (see above) held in float64."""
    grid = np.asarray(grid, dtype=np.float32)
    level = np.float32(level)
    out = []
    for axis in range(3):
        n = grid.shape[axis]
        if n < 2:
            continue
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, n - 1), slice(1, n)
        va, vb = grid[tuple(lo)], grid[tuple(hi)]
        cross = (va < level) != (vb < level)
        idx = np.argwhere(cross)
        if not len(idx):
            continue
        a, b = va[cross], vb[cross]
        with np.errstate(all="ignore"):
            t = ((level - a) / (b - a)).astype(np.float32)                 # one float32 subtraction each, one float32 division
            u = (idx[:, axis].astype(np.float32) + t).astype(np.float32)   # one float32 addition
        site = idx.astype(np.float64)
        site[:, axis] = u.astype(np.float64)
        out.append(site)
    return np.concatenate(out) if out else np.zeros((0, 3))


def world_float32(sites, spacing):
    """The float32 world positions the library reports for sites given in index coordinates: coordinate * spacing, one rounding."""
    sp = np.array([np.float32(x) for x in ((spacing,) * 3 if np.isscalar(spacing) else spacing)], dtype=np.float32)
    return (sites.astype(np.float32) * sp[None, :]).astype(np.float32)


def transform(shape, sites, spacing, chunk=1 << 22):
    """(T [D, H, W] float64: the squared distance of every voxel to its nearest site, +inf without sites; the index of that site)."""
    sp = spacing3(spacing)
    voxels = np.stack(np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij"), axis=-1).reshape(-1, 3)
    T = np.full(len(voxels), np.inf)
    arg = np.full(len(voxels), -1, dtype=np.int64)
    if len(sites):
        rows = max(1, chunk // len(sites))
        for b in range(0, len(voxels), rows):
            d = (voxels[b:b + rows, None, :] - sites[None, :, :]) * sp
            d2 = (d * d).sum(axis=2)
            arg[b:b + rows] = d2.argmin(axis=1)
            T[b:b + rows] = d2[np.arange(d2.shape[0]), arg[b:b + rows]]
    return T.reshape(shape), arg.reshape(shape)


def squared_to(shape, points, spacing):
    """Squared distance (float64) of every voxel of `shape` to its own point: points [D, H, W, 3] in index coordinates."""
    sp = spacing3(spacing)
    voxels = np.stack(np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij"), axis=-1)
    d = (voxels - points) * sp
    return (d * d).sum(axis=-1)


def finish(grid, T, level, value_scale=1.0, keep_band=False):
    """The signed distance of the header's finishing step, float64: s sqrt(T); with keep_band the voxels with a 6-neighbour on the other
    side keep (v - level) value_scale, the subtraction and the product as float32 operations (they are the definition)."""
    grid = np.asarray(grid, dtype=np.float32)
    below = grid < np.float32(level)
    out = np.where(below, -1.0, 1.0) * np.sqrt(T)
    if keep_band:
        band = np.zeros(grid.shape, dtype=bool)
        for axis in range(3):
            if grid.shape[axis] < 2:
                continue
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, -1), slice(1, None)
            differ = below[tuple(lo)] != below[tuple(hi)]
            band[tuple(lo)] |= differ
            band[tuple(hi)] |= differ
        kept = ((grid - np.float32(level)).astype(np.float32) * np.float32(value_scale)).astype(np.float32)
        out = np.where(band, kept.astype(np.float64), out)
    return out
