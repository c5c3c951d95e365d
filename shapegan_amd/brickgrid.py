"""Narrow-band voxel grids: a field evaluated only in bricks near its level set (csrc/brickgrid.hip, K18; CPU tensors run the twin).

    result = narrow_band_grids(evaluate, shapes=S, resolution=R, device=dev, brick=4, level=0.0)
    result.grid        # [S,R,R,R]: the field in every active brick, one constant (the brick's fill) in every other
    result.stats       # {"evaluated_points": [S], "active_bricks": [S], "rounds": n, ...}

`evaluate(points [N,3] float32, shape_index [N] int32) -> values [N] float32` is the field: SDFNet.voxel_grids passes the network
(one sg_sdfnet_fwd launch per call), the tests pass analytic fields.  It must give a point the same value wherever the point
stands in a call; the rule, and what it guarantees about marching cubes of the result, are stated in include/shapegan_hip.h, K18.

Host synchronisation: every round of the continuation reads the count of newly active bricks back from the device (it sizes the
next launch), so a call synchronises 2 + (rounds of continuation) times.  Like meshing (mesh.marching_cubes), which synchronises
too, this path is not meant for graph capture.
"""
import math

import numpy as np
import torch

from . import lib as L
from .lib import check, ptr, stream

BRICK_SIZES = (4, 8, 16)
_axis_cache = {}


def axis_tables(resolution, device):
    """The three per-axis float32 tables [R] of util.get_voxel_coordinates(R): linspace(-1, 1, R) in float64, cast last, so that
    (x[i], y[j], z[k]) is bit for bit row i R^2 + j R + k of that grid."""
    device = torch.device(device)
    key = (int(resolution), str(device))
    if key not in _axis_cache:
        axis = torch.from_numpy(np.linspace(-1.0, 1.0, int(resolution)).astype(np.float32)).to(device)
        _axis_cache[key] = (axis, axis.clone(), axis.clone())
    return _axis_cache[key]


def default_band(resolution, brick, lipschitz=1.0, spacing=None):
    """lipschitz * sqrt(3) * (B - 1) / 2 * h: the largest distance from a point of a brick to the nearest of its corners, times a
    Lipschitz bound of the field.  h: the lattice spacing (2 / (R - 1) for the grid of util.get_voxel_coordinates)."""
    h = 2.0 / (resolution - 1) if spacing is None else float(spacing)
    return float(lipschitz) * (brick - 1) / 2.0 * h * math.sqrt(3.0)


def options(narrow_band):
    """The keyword arguments SDFNet.voxel_grids takes for a caller's `narrow_band` argument: False / True, or a dict of the brick
    path's own arguments (brick, band, lipschitz), which switches it on."""
    if isinstance(narrow_band, dict):
        unknown = set(narrow_band) - {"brick", "band", "lipschitz"}
        if unknown:
            raise ValueError("narrow_band: unknown options %s" % sorted(unknown))
        return dict(narrow_band=True, **narrow_band)
    return dict(narrow_band=bool(narrow_band))


class BrickGrid(object):
    """What narrow_band_grids returns: grid [S,R,R,R], state [S,nb] int32 (0 inactive, else active), fill [S,nb], round_lists (the
    ascending global brick ids that became active in each round, int32 tensors) and the stats dict (which carries `state` too)."""

    def __init__(self, grid, state, fill, round_lists, stats):
        self.grid, self.state, self.fill, self.round_lists, self.stats = grid, state, fill, round_lists, stats


def check_arguments(shapes, resolution, brick, mask=None, band=None):
    """The refusals, before any launch."""
    S, R, B = int(shapes), int(resolution), int(brick)
    if B not in BRICK_SIZES:
        raise ValueError("narrow band: brick must be one of %s, got %d" % (BRICK_SIZES, B))
    if R <= 0 or R % B != 0:
        raise ValueError("narrow band: the resolution (%d) must be a positive multiple of the brick size (%d)" % (R, B))
    if S <= 0:
        raise ValueError("narrow band: no shapes")
    if S * (R // B) ** 3 > 2147483647 or S > 65535:
        raise ValueError("narrow band: %d shapes at %d^3 exceed the int32 brick ids of one call" % (S, R))
    if mask is not None and mask.numel() != R ** 3:
        raise ValueError("narrow band: the mask has %d entries, the lattice %d" % (mask.numel(), R ** 3))
    if band is not None and not band >= 0:
        raise ValueError("narrow band: band must be >= 0, got %r" % (band,))
    return S, R, B


def narrow_band_grids(evaluate, shapes, resolution, device, brick=4, level=0.0, band=None, lipschitz=1.0, pad=True, mask=None,
                      axes=None):
    """Runs the seed phase and the continuation to its fixed point and returns a BrickGrid.  mask: [R^3] (or [R,R,R]) bool / uint8
    tensor shared by all shapes, False = the point is left out and is 1; axes: three [R] float32 tensors (default: axis_tables).
    pad: whether the grid will be meshed with the virtual shell of 1 around it (seed rule (c)).  Synchronises once per round."""
    S, R, B = check_arguments(shapes, resolution, brick, mask, band)
    dev = torch.device(device)
    level = float(level)
    ax = axis_tables(R, dev) if axes is None else tuple(L.f32c(a).to(dev) for a in axes)
    if len(ax) != 3 or any(a.numel() != R for a in ax):
        raise ValueError("narrow band: three axis tables of %d entries are needed" % R)
    if band is None:
        band = default_band(R, B, lipschitz, spacing=abs(float(ax[0][1]) - float(ax[0][0])) if R > 1 else 0.0)
    if mask is not None:
        mask = mask.reshape(-1).to(device=dev, dtype=torch.uint8).contiguous()
    nb = (R // B) ** 3
    n, ppb = S * nb, B ** 3
    lib = L.load()
    i32 = dict(dtype=torch.int32, device=dev)
    f32 = dict(dtype=torch.float32, device=dev)
    state, flag, brick_list, count = torch.empty(n, **i32), torch.empty(n, **i32), torch.empty(n, **i32), torch.empty(1, **i32)
    fill = torch.empty(n, **f32)
    grid = torch.empty((S, R, R, R), **f32)
    ws = L.workspace("brick_compact", lib.sg_brick_compact_workspace_bytes(S, R, B), dev)

    def list_points(bricks, m, corners):
        k = m * (8 if corners else ppb)
        points, sid = torch.empty((k, 3), **f32), torch.empty(k, **i32)
        check(lib.sg_brick_points(ptr(bricks), m, int(corners), S, R, B, ptr(ax[0]), ptr(ax[1]), ptr(ax[2]), ptr(points), ptr(sid),
                                  stream()), "brick_points")
        return points, sid

    def values_of(points, sid):
        v = evaluate(points, sid)
        if v.shape != (points.shape[0],) or v.dtype != torch.float32 or v.device != points.device:
            raise ValueError("narrow band: evaluate must return float32 [N] on the device of the points")
        return v.contiguous()

    round_lists = []
    try:
        points, sid = list_points(None, n, True)
        corner_values = values_of(points, sid)
        check(lib.sg_brick_seed(ptr(corner_values), ptr(mask), S, R, B, level, float(band), int(bool(pad)), ptr(state), ptr(fill),
                                ptr(flag), ptr(grid), stream()), "brick_seed")
        max_rounds = 3 * R // B
        while True:
            check(lib.sg_brick_compact(ptr(state), ptr(flag), S, R, B, ptr(brick_list), ptr(count), ptr(ws), ws.numel(), stream()),
                  "brick_compact")
            m = int(count.item())      # the one device -> host read of a round: it sizes the round's launches
            if m == 0:
                break
            if len(round_lists) >= max_rounds:
                raise RuntimeError("narrow band: the continuation did not end within %d rounds" % max_rounds)
            bricks = brick_list[:m].clone()
            round_lists.append(bricks)
            points, sid = list_points(bricks, m, False)
            values = values_of(points, sid)
            check(lib.sg_brick_scatter(ptr(values), ptr(bricks), m, ptr(mask), S, R, B, ptr(grid), stream()), "brick_scatter")
            check(lib.sg_brick_grow(ptr(bricks), m, ptr(grid), ptr(state), ptr(fill), S, R, B, level, ptr(flag), stream()), "brick_grow")
    finally:
        L.reset_call_state()
    state = state.view(S, nb)
    active = (state != 0).sum(dim=1).cpu().tolist()
    stats = {
        "resolution": R, "brick": B, "band": float(band), "level": level, "rounds": len(round_lists),
        "bricks_per_round": [int(b.numel()) for b in round_lists],
        "active_bricks": active,
        "state": state,
        "corner_points": 8 * nb,
        # every point the field was asked for, per shape: the 8 corners of every brick and the points of the active bricks
        "evaluated_points": [8 * nb + a * ppb for a in active],
        "dense_points": R ** 3,
    }
    return BrickGrid(grid, state, fill.view(S, nb), round_lists, stats)
