"""Upscaling voxel grids: cubic B-spline zoom and sampling (K20 of include/shapegan_hip.h; csrc/spline.hip, CPU tensors on the twin).

    fine = zoom_grids(voxels_32, zoom=4)                    # scipy.ndimage.zoom(voxels_32, 4) of create_plot.py:826-828, batched
    values, grad = sample_grids(voxels_32, points, gradient=True)
    batch = mesh.marching_cubes(voxels_32, spacing=2 / 32, origin=-1, upscale=4)

The voxel models (model/gan.py Generator, model/autoencoder.py, the progressive GAN at its final size) produce 32^3 grids; meshing them
as they are gives stair-stepped surfaces.  `zoom_grids` is scipy.ndimage.zoom at its defaults: a cubic B-spline prefilter with the mirror
boundary, then a resampling at o (n - 1) / (N - 1).  `sample_grids` is scipy.ndimage.map_coordinates(order=3, mode='constant') with
the rule of the header for points outside.  PyTorch has neither: F.interpolate is trilinear in 3-D, and its 2-D bicubic is the Keys
kernel, which needs no prefilter and does not reproduce a B-spline.

Inputs are numpy arrays or tensors of any float dtype, [D, H, W] or [S, D, H, W], contiguous or not; the work is fp32 and the results
are tensors on the input's device (a numpy array is a CPU tensor: the twin).  Nothing here is differentiable: a grid that requires
grad raises.
"""
import numpy as np
import torch

from . import lib as L
from . import ops

MAX_AXIS = L.abi.core_defines("spline_core.h")["SG_SPLINE_MAX_AXIS"]
TILE = tuple(L.abi.core_defines("spline_core.h")["SG_SPLINE_TILE_%s" % a] for a in "DHW")
_MAX_ELEMENTS = 1 << 31      # of one array of one call: 8 GiB of fp32; the library's own limit is 2^36


def max_grids_per_call(shape, size=None):
    """Largest number of grids of `shape` (D, H, W), zoomed to `size`, that one library call takes: the batch is split beyond it
    (the counterpart of mesh.max_shapes_per_call)."""
    cells = int(shape[0]) * int(shape[1]) * int(shape[2])
    if size is not None:
        cells = max(cells, int(size[0]) * int(size[1]) * int(size[2]))
    return max(1, _MAX_ELEMENTS // cells)


def _grids(what, grids):
    """(fp32 contiguous [S, D, H, W], was it a single grid?)"""
    if isinstance(grids, np.ndarray):
        grids = torch.from_numpy(np.ascontiguousarray(grids))
    if not torch.is_tensor(grids) or not grids.dtype.is_floating_point:
        raise ValueError("%s: expected a floating-point array or tensor" % what)
    if grids.requires_grad:
        raise ValueError("%s: not differentiable — detach the grids" % what)
    single = grids.dim() == 3
    if single:
        grids = grids.unsqueeze(0)
    if grids.dim() != 4:
        raise ValueError("%s: expected [D, H, W] or [S, D, H, W], got %s" % (what, tuple(grids.shape)))
    if min(grids.shape[1:]) < 1 or max(grids.shape[1:]) > MAX_AXIS:
        raise ValueError("%s: every grid axis must hold 1 to %d values, got %s" % (what, MAX_AXIS, tuple(grids.shape[1:])))
    return L.f32c(grids), single


def _chunks(S, per):
    return [(b, min(b + per, S)) for b in range(0, S, per)] or [(0, 0)]


def _each(grids, per, fn):
    parts = [fn(grids[b:e]) for b, e in _chunks(grids.shape[0], per)]
    return parts[0] if len(parts) == 1 else torch.cat(parts)


def spline_coefficients(grids):
    """The cubic B-spline coefficients of the grids, in their shape: what zoom_grids and sample_grids interpolate with.  Computing
    them once serves any number of zoom_grids(..., coefficients=True) / sample_grids(..., coefficients=True) calls."""
    g, single = _grids("spline_coefficients", grids)
    out = _each(g, max_grids_per_call(g.shape[1:]), ops.spline_prefilter)
    return out[0] if single else out


def zoom_size(shape, zoom):
    """scipy.ndimage.zoom's size rule: round(n * zoom) per axis (zoom: a factor or one per axis)."""
    factors = (float(zoom),) * 3 if np.isscalar(zoom) else tuple(float(z) for z in zoom)
    if len(factors) != 3:
        raise ValueError("zoom_grids: zoom is a factor or one per axis, got %r" % (zoom,))
    return tuple(int(round(int(n) * z)) for n, z in zip(shape, factors))


def zoom_grids(grids, zoom=None, size=None, order=3, coefficients=False):
    """scipy.ndimage.zoom(grid, zoom, order=order) of every grid: [S, D', H', W'] (or [D', H', W']), D' = round(D * zoom), or `size`
    = (D', H', W') outright.  order 3 (cubic B-spline, interpolating) or 1 (trilinear at the same positions).  Downscaling uses the
    same formula, without anti-aliasing.  coefficients=True: `grids` already holds spline_coefficients (order 3)."""
    if (zoom is None) == (size is None):
        if zoom is None:
            zoom = 4
        else:
            raise ValueError("zoom_grids: give zoom or size, not both")
    if order not in (1, 3):
        raise ValueError("zoom_grids: order 1 or 3, got %r" % (order,))
    if coefficients and order != 3:
        raise ValueError("zoom_grids: coefficients belong to order 3")
    g, single = _grids("zoom_grids", grids)
    size = zoom_size(g.shape[1:], zoom) if size is None else tuple(int(n) for n in size)
    if len(size) != 3 or min(size) < 1 or max(size) > MAX_AXIS:
        raise ValueError("zoom_grids: the output size must be three lengths in 1 .. %d, got %r" % (MAX_AXIS, size))

    def one(chunk):
        return ops.spline_zoom(chunk if (coefficients or order == 1) else ops.spline_prefilter(chunk), size, order)

    out = _each(g, max_grids_per_call(g.shape[1:], size), one)
    return out[0] if single else out


def sample_grids(grids, points, gradient=False, outside=1.0, coefficients=False):
    """The cubic B-spline interpolant of every grid at points [S, P, 3] ([P, 3] for one grid) given in index coordinates (d, h, w):
    values [S, P] and, with gradient=True, their gradient [S, P, 3] with respect to those coordinates.  A point outside [0, n - 1] on
    any axis gives `outside` and a zero gradient; a point on a face is inside.  coefficients=True: `grids` already holds
    spline_coefficients."""
    g, single = _grids("sample_grids", grids)
    if isinstance(points, np.ndarray):
        points = torch.from_numpy(np.ascontiguousarray(points))
    if not torch.is_tensor(points) or not points.dtype.is_floating_point:
        raise ValueError("sample_grids: points must be a floating-point array or tensor")
    if single and points.dim() == 2:
        points = points.unsqueeze(0)
    if points.dim() != 3 or points.shape[0] != g.shape[0] or points.shape[2] != 3:
        raise ValueError("sample_grids: points must be [S = %d, P, 3], got %s" % (g.shape[0], tuple(points.shape)))
    if points.device != g.device:
        raise RuntimeError("sample_grids: the grids are on %s, the points on %s" % (g.device, points.device))
    points = L.f32c(points.detach())
    per = max(1, min(max_grids_per_call(g.shape[1:]), _MAX_ELEMENTS // max(1, 3 * points.shape[1])))
    parts = []
    for b, e in _chunks(g.shape[0], per):
        c = g[b:e] if coefficients else ops.spline_prefilter(g[b:e])
        parts.append(ops.spline_sample(c, points[b:e].contiguous(), gradient, outside))
    if gradient:
        values, grad = (parts[0] if len(parts) == 1 else tuple(torch.cat(x) for x in zip(*parts)))
        return (values[0], grad[0]) if single else (values, grad)
    values = parts[0] if len(parts) == 1 else torch.cat(parts)
    return values[0] if single else values

