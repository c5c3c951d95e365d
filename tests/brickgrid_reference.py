"""The narrow-band rule of include/shapegan_hip.h, K18, restated in numpy from the header alone.

Input is the DENSE grid [S,R,R,R] (float32, masked points already 1): the rule only ever looks at values the dense grid holds.  The
continuation is written as a dilation of the evaluated points (all of them, every round), not as the per-brick region masks of the
kernels.
"""
import numpy as np


def _corners(dense, B):
    S, R = dense.shape[0], dense.shape[1]
    nbx = R // B
    c = dense.reshape(S, nbx, B, nbx, B, nbx, B)[:, :, [0, B - 1]][:, :, :, :, [0, B - 1]][:, :, :, :, :, :, [0, B - 1]]
    return c.transpose(0, 1, 3, 5, 2, 4, 6).reshape(S, nbx, nbx, nbx, 8)      # corner n = (n >> 2 & 1, n >> 1 & 1, n & 1)


def _neighbour_differs(side):
    """[S,nbx,nbx,nbx] bool: some of the 26 neighbours (inside the lattice) has the other value."""
    n = side.shape[1]
    out = np.zeros_like(side)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                if dx == dy == dz == 0:
                    continue
                a = [slice(max(0, -d), n - max(0, d)) for d in (dx, dy, dz)]
                b = [slice(max(0, d), n - max(0, -d)) for d in (dx, dy, dz)]
                out[(slice(None), *a)] |= side[(slice(None), *a)] != side[(slice(None), *b)]
    return out


def _dilate2(x):
    """Chebyshev dilation by 2 lattice steps of a bool [S,R,R,R]."""
    for axis in (1, 2, 3):
        R = x.shape[axis]
        p = np.zeros_like(x)
        for d in (-2, -1, 0, 1, 2):
            src = [slice(None)] * 4
            dst = [slice(None)] * 4
            src[axis] = slice(max(0, d), R - max(0, -d))
            dst[axis] = slice(max(0, -d), R - max(0, d))
            p[tuple(dst)] |= x[tuple(src)]
        x = p
    return x


def _to_points(bricks, B):
    return bricks.repeat(B, axis=1).repeat(B, axis=2).repeat(B, axis=3)


def _any_in_brick(points, B):
    S, R = points.shape[0], points.shape[1]
    nbx = R // B
    return points.reshape(S, nbx, B, nbx, B, nbx, B).any(axis=(2, 4, 6))


def narrow_band(dense, B, level=0.0, band=0.0, pad=True, mask=None):
    """-> dict(state [S,nb] bool, fill [S,nb], rounds: list of ascending global brick ids per round, grid [S,R,R,R])."""
    dense = np.asarray(dense, dtype=np.float32)
    S, R = dense.shape[0], dense.shape[1]
    nbx = R // B
    level32, band32 = np.float32(level), np.float32(band)
    c = _corners(dense, B)
    fill = c[..., 0].copy()
    inside = c < level32
    fside = inside[..., 0]
    mixed = inside.any(-1) & ~inside.all(-1)
    near = (np.abs(c - level32) <= band32).any(-1)
    border = np.zeros((nbx, nbx, nbx), dtype=bool)
    border[[0, -1]] = border[:, [0, -1]] = border[:, :, [0, -1]] = True
    active = mixed | near | (bool(pad) & border[None] & inside.any(-1)) | _neighbour_differs(fside)
    rounds = []
    new = active.copy()
    pin = dense < level32
    while new.any():
        rounds.append(np.flatnonzero(new.reshape(-1)).astype(np.int32))
        ev = _to_points(active, B)
        near_in, near_out = _dilate2(ev & pin), _dilate2(ev & ~pin)
        new = ~active & np.where(fside, _any_in_brick(near_out, B), _any_in_brick(near_in, B))
        active = active | new
    grid = np.where(_to_points(active, B), dense, _to_points(fill, B)).astype(np.float32)
    if mask is not None:
        grid[:, ~np.asarray(mask, dtype=bool).reshape(R, R, R)] = 1.0
    return dict(state=active.reshape(S, -1), fill=fill.reshape(S, -1), rounds=rounds, grid=grid)
