"""Distance transforms of voxel grids: exact Euclidean distance transform and redistancing (K21 of include/shapegan_hip.h;
csrc/edt.hip, CPU tensors on the twin).

    dist = distance_transform(occupancy)                        # scipy.ndimage.distance_transform_edt, batched
    sdf = redistance_grids(voxels_32)                           # world distances everywhere, not only inside the +-0.1 truncation
    grids = occupancy_to_sdf(load_binvox(path)[0], clamp=0.1)   # what VoxelDataset hands a trainer, from an occupancy grid
    batch = mesh.marching_cubes(voxels_32, level=1.5, pad_value=4.0, spacing=2 / 32, origin=-1, redistance=True)   # an offset surface

The voxel models and VoxelDataset (datasets.py:7-40) hold distances clamped to +-0.1 and stored as sdf / 0.1: more than a voxel or
two from the surface a grid says +-1 and nothing else.  `redistance_grids` measures every voxel's distance to the points where the
grid crosses the level on its edges (the vertices marching cubes would emit) and keeps the grid's own values next to the surface,
where they are the better distances.  `distance_transform` is the transform of an occupancy mask with scipy's semantics.

Inputs are numpy arrays or tensors, [D, H, W] or [S, D, H, W], contiguous or not; the work is fp32 and the results are tensors on the
input's device (a numpy array is a CPU tensor: the twin).  Nothing here is differentiable: a grid that requires grad raises.
"""
import numpy as np
import torch

from . import lib as L
from . import ops

MAX_AXIS = L.abi.core_defines("edt_core.h")["SG_EDT_MAX_AXIS"]
_MAX_ELEMENTS = 1 << 29      # of one call: the scratch of the per-axis form is up to five arrays of this size


def max_grids_per_call(shape):
    """Largest number of grids of `shape` (D, H, W) one library call takes: the batch is split beyond it."""
    return max(1, _MAX_ELEMENTS // (int(shape[0]) * int(shape[1]) * int(shape[2])))


def _grids(what, grids, floating=True):
    """(contiguous [S, D, H, W] — fp32 when `floating` —, was it a single grid?)"""
    if isinstance(grids, np.ndarray):
        grids = torch.from_numpy(np.ascontiguousarray(grids))
    if not torch.is_tensor(grids) or (floating and not grids.dtype.is_floating_point):
        raise ValueError("%s: expected %s array or tensor" % (what, "a floating-point" if floating else "an"))
    if grids.requires_grad:
        raise ValueError("%s: not differentiable — detach the grids" % what)
    single = grids.dim() == 3
    if single:
        grids = grids.unsqueeze(0)
    if grids.dim() != 4:
        raise ValueError("%s: expected [D, H, W] or [S, D, H, W], got %s" % (what, tuple(grids.shape)))
    if min(grids.shape[1:]) < 1 or max(grids.shape[1:]) > MAX_AXIS:
        raise ValueError("%s: every grid axis must hold 1 to %d values, got %s" % (what, MAX_AXIS, tuple(grids.shape[1:])))
    return (L.f32c(grids) if floating else grids.contiguous()), single


def _each(grids, fn):
    """fn on chunks of the batch; fn returns a tensor or a tuple of tensors."""
    per, S = max_grids_per_call(grids.shape[1:]), grids.shape[0]
    parts = [fn(grids[b:min(b + per, S)]) for b in range(0, S, per)] or [fn(grids)]
    if len(parts) == 1:
        return parts[0]
    return tuple(torch.cat(x) for x in zip(*parts)) if isinstance(parts[0], tuple) else torch.cat(parts)


def _default_spacing(shape):
    return 2.0 / max(shape)


def distance_transform(masks, spacing=1, return_indices=False, squared=False):
    """scipy.ndimage.distance_transform_edt(mask, sampling=spacing) of every mask: per voxel the distance to the nearest voxel where
    the mask is 0 (so a 0 voxel gives 0), +inf in a mask without zeros.  squared=True returns the squared distances, exact with unit
    spacing.  return_indices=True also returns, as scipy does, the coordinates of such a voxel: int64 [S, 3, D, H, W] ([3, D, H, W] for
    one mask), -1 where there is none; among equally near voxels the choice is the library's (the header states it), not scipy's.
    The root is sg_edt_finish's without a grid: correctly rounded, the same bits on the GPU and in the twin, which torch.sqrt does
    not promise."""
    m, single = _grids("distance_transform", masks, floating=False)

    def one(chunk):
        g = (chunk != 0).to(torch.float32)
        out = ops.edt_voxels(g, level=0.5, inside=True, spacing=spacing, nearest=return_indices)
        sq, idx = out if return_indices else (out, None)
        dist = sq if squared else ops.edt_finish(None, sq)
        return (dist, idx) if return_indices else dist

    out = _each(m, one)
    if not return_indices:
        return out[0] if single else out
    dist, idx = out
    D, H, W = m.shape[1:]
    idx = idx.long()
    coords = torch.stack((idx // (H * W), idx // W % H, idx % W), dim=1)
    coords = torch.where(idx.unsqueeze(1) < 0, torch.full_like(coords, -1), coords)
    return (dist[0], coords[0]) if single else (dist, coords)


def redistance_grids(grids, level=0.0, spacing=None, value_scale=0.1, keep_band=True, return_closest=False):
    """Signed world distances [S, D, H, W] to the `level` set of every grid: per voxel the distance to the nearest point where the grid
    crosses `level` on a grid edge (by linear interpolation: marching cubes' vertices), negative where the grid is below the level;
    +-inf in a grid that never crosses it.  spacing: the world length of an index step (one or one per axis; default 2 / the longest
    axis: grids that span [-1, 1]).  keep_band: voxels with a 6-neighbour on the other side of the level keep their own value,
    (v - level) * value_scale — value_scale is world distance per grid unit, 0.1 for VoxelDataset grids, 1 for raw distances.
    return_closest=True also returns the crossing's world position [S, D, H, W, 3] (NaN where there is none)."""
    g, single = _grids("redistance_grids", grids)
    spacing = _default_spacing(g.shape[1:]) if spacing is None else spacing

    def one(chunk):
        out = ops.edt_crossings(chunk, level=level, spacing=spacing, closest=return_closest)
        sq, where = out if return_closest else (out, None)
        sdf = ops.edt_finish(chunk, sq, level=level, value_scale=value_scale, keep_band=keep_band)
        return (sdf, where) if return_closest else sdf

    out = _each(g, one)
    if return_closest:
        return (out[0][0], out[1][0]) if single else out
    return out[0] if single else out


def occupancy_to_sdf(occupancy, spacing=None, clamp=None):
    """An occupancy grid (non-zero: occupied) as a signed distance grid: occupied voxels count as -0.5 and free ones as +0.5, so the
    surface crosses every edge between the two at its midpoint, and every voxel gets its signed world distance to those midpoints
    (spacing as in redistance_grids).  clamp=0.1 returns clamp(sdf, +-clamp) / clamp: what VoxelDataset hands a trainer."""
    m, single = _grids("occupancy_to_sdf", occupancy, floating=False)
    spacing = _default_spacing(m.shape[1:]) if spacing is None else spacing

    def one(chunk):
        g = torch.where(chunk != 0, -0.5, 0.5).to(torch.float32)
        sdf = ops.edt_finish(g, ops.edt_crossings(g, level=0.0, spacing=spacing), level=0.0, keep_band=False)
        return sdf if clamp is None else ops.voxel_prepare(sdf, clamp, clamp)

    out = _each(m, one)
    return out[0] if single else out


def offset_grids(grids, distance, level=0.0, spacing=None, value_scale=0.1, keep_band=True):
    """redistance_grids(...) - distance: the signed world distance to the surface moved outward by `distance` (inward when negative);
    its zero level is the offset surface."""
    return redistance_grids(grids, level, spacing, value_scale, keep_band) - float(distance)


def load_binvox(path):
    """Reads a .binvox file (the format ShapeNet ships its voxelisations in): the text header `#binvox 1`, `dim dx dy dz`, `translate
    tx ty tz`, `scale s`, `data`, then (value, count) byte pairs that run through the voxels with y fastest, then z, then x.  Returns
    (occupancy bool [dx, dy, dz] — a CPU tensor —, translate (tx, ty, tz), scale).  The parser runs on the host."""
    with open(path, "rb") as fh:
        if not fh.readline().strip().startswith(b"#binvox"):
            raise ValueError("load_binvox: %s does not start with #binvox" % path)
        dims, translate, scale = None, (0.0, 0.0, 0.0), 1.0
        while True:
            line = fh.readline()
            if not line:
                raise ValueError("load_binvox: %s has no data section" % path)
            words = line.split()
            if not words:
                continue
            if words[0] == b"dim":
                dims = tuple(int(w) for w in words[1:4])
            elif words[0] == b"translate":
                translate = tuple(float(w) for w in words[1:4])
            elif words[0] == b"scale":
                scale = float(words[1])
            elif words[0] == b"data":
                break
        raw = np.frombuffer(fh.read(), dtype=np.uint8)
    if dims is None or len(dims) != 3 or min(dims) < 1:
        raise ValueError("load_binvox: %s has no usable dim line" % path)
    if raw.size % 2:
        raise ValueError("load_binvox: %s: the data section is not (value, count) pairs" % path)
    flat = np.repeat(raw[0::2] != 0, raw[1::2])
    if flat.size != dims[0] * dims[1] * dims[2]:
        raise ValueError("load_binvox: %s holds %d voxels, its header says %s" % (path, flat.size, dims))
    voxels = flat.reshape(dims[0], dims[2], dims[1]).transpose(0, 2, 1)
    return torch.from_numpy(np.ascontiguousarray(voxels)), translate, scale
