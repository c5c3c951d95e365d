"""Geometry taken from the network instead of the voxel grid: meshes whose vertices lie on the level set and carry its exact normals,
and oriented point clouds on the surface.

marching_cubes places a vertex by linear interpolation along a cell edge and takes its normal from central differences of the grid;
at 64^3 that staircase shows in every render and export.  The network knows better: f and grad f at a vertex give the true surface a
Newton step or two away, and grad f / |grad f| is its normal there.  Both come from SDFNet.project_to_level_set — one fused launch
per batch of points (csrc/sdfnet_project.hip) that keeps nothing of the forward but sign bits on the chip, where the reference
(model/sdf_net.py:118-156) takes one first-order step through autograd and assumes |grad f| = 1.
"""
import math

import torch

from .brickgrid import options as narrow_band_options
from .mesh import MeshBatch, marching_cubes


def cell_diagonal(voxel_resolution):
    """The diagonal of one cell of the get_mesh grid (spacing 2 / R): how far a marching-cubes vertex can be from the surface it
    brackets, and the default limit of refine_meshes for callers that know the grid."""
    return math.sqrt(3.0) * 2.0 / int(voxel_resolution)


def _unit(grad):
    n = grad.norm(dim=1, keepdim=True)
    return torch.where(n > 0, grad / n.clamp_min(1e-30), torch.zeros_like(grad)), n.squeeze(1)


def _shape_stats(values, shape_index, nshapes):
    """(mean, max) of values [V] per shape; 0 for a shape without vertices."""
    total = torch.zeros(nshapes, dtype=torch.float64, device=values.device).index_add_(0, shape_index, values.double())
    count = torch.zeros(nshapes, dtype=torch.float64, device=values.device).index_add_(0, shape_index, torch.ones_like(values, dtype=torch.float64))
    top = torch.zeros(nshapes, dtype=values.dtype, device=values.device).scatter_reduce_(0, shape_index, values, "amax", include_self=True)
    return (total / count.clamp_min(1)).cpu().tolist(), top.cpu().tolist()


def refine_meshes(sdf_net, latent_codes, mesh_batch, level=0.0, iterations=3, max_move=None, tolerance=1e-4):
    """Projects every vertex of shape s of `mesh_batch` onto f(., latent_codes[s]) = level by `iterations` Newton steps and replaces
    its normal by grad f / |grad f| (toward increasing values, the convention of marching_cubes).  Faces and offsets are untouched.
    A vertex keeps its position and normal if its final |f - level| > tolerance, if it moved farther than max_move in total (None:
    no limit; callers that know the grid pass cell_diagonal(R) — a vertex that jumped to another sheet is worse than one that
    stayed), or if its gradient vanished.  -> (MeshBatch, stats); stats: per shape "vertices", "kept_back", and mean / max
    |f - level| "before" and "after" (lists of S)."""
    if iterations < 1:
        raise ValueError("refine_meshes needs at least one iteration, got %r" % (iterations,))
    if max_move is not None and not float(max_move) > 0:
        raise ValueError("max_move must be positive or None, got %r" % (max_move,))
    S = len(mesh_batch)
    vo_host = mesh_batch._offsets()[0]
    v = mesh_batch.vertices
    shape_index = torch.repeat_interleave(torch.arange(S, device=v.device), mesh_batch.vert_offsets[1:] - mesh_batch.vert_offsets[:-1])
    stats = {"vertices": [int(n) for n in (vo_host[1:] - vo_host[:-1])], "kept_back": [0] * S, "mean_before": [0.0] * S,
             "max_before": [0.0] * S, "mean_after": [0.0] * S, "max_after": [0.0] * S}
    if v.shape[0] == 0:
        return mesh_batch, stats
    proj = sdf_net.surface_projector(latent_codes)
    _, f0, _ = proj.run(v, vo_host, mesh_batch.vert_offsets, iterations=0)
    x, f, g = proj.run(v, vo_host, mesh_batch.vert_offsets, level=level, iterations=iterations, rule="newton",
                       max_step=0.0 if max_move is None else float(max_move))
    normal, gnorm = _unit(g)
    moved = (x - v).norm(dim=1)
    keep = ~((f - level).abs() <= tolerance) | ~(gnorm > 0) | ~torch.isfinite(x).all(dim=1)
    if max_move is not None:
        keep = keep | ~(moved <= float(max_move))
    vertices = torch.where(keep.unsqueeze(1), v, x)
    normals = torch.where(keep.unsqueeze(1), mesh_batch.normals, normal)
    before = (f0 - level).abs()
    after = torch.where(keep, before, (f - level).abs())
    stats["kept_back"] = torch.zeros(S, dtype=torch.int64, device=v.device).index_add_(0, shape_index, keep.long()).cpu().tolist()
    stats["mean_before"], stats["max_before"] = _shape_stats(before, shape_index, S)
    stats["mean_after"], stats["max_after"] = _shape_stats(after, shape_index, S)
    return MeshBatch(vertices, normals, mesh_batch.faces, mesh_batch.vert_offsets, mesh_batch.tri_offsets), stats


def sample_oriented_clouds(sdf_net, latent_codes, count, voxel_resolution=32, level=0.0, iterations=5, generator=None, narrow_band=False):
    """`count` points on the level set of every code [S,L] with their unit normals: voxel_grids -> marching_cubes ->
    MeshBatch.sample_surface gives samples that are area-uniform on a coarse mesh, `iterations` Newton steps (each at most a cell
    diagonal long) put them on the true surface.  Random starts in the cube are not used: most of the cube lies where the trained
    network is flat and its gradient noise, and a projection from there never arrives — the reason the reference discards by
    sdf_cutoff (model/sdf_net.py:130-156).  -> (points [S,count,3], normals [S,count,3], valid [S] bool); a shape whose grid never
    crosses `level` has valid False and rows of zeros."""
    codes = latent_codes.detach().reshape(-1, sdf_net.latent_code_size)
    S, R = codes.shape[0], int(voxel_resolution)
    with torch.no_grad():
        grids = sdf_net.voxel_grids(codes, R, sphere_only=True, level=level, **narrow_band_options(narrow_band))
        batch = marching_cubes(grids, level=level, spacing=2.0 / R, origin=-1.0, pad=True, pad_value=1.0)
        start, empty = batch.sample_surface(count, generator=generator, return_empty=True)
        x, _, g = sdf_net.project_to_level_set(start.reshape(-1, 3), codes, None, level=level, iterations=iterations, rule="newton",
                                               max_step=cell_diagonal(R))
        normals, _ = _unit(g)
        valid = empty == 0
        mask = valid.view(S, 1, 1)
        points = torch.where(mask, x.view(S, int(count), 3), torch.zeros((), device=x.device))
        normals = torch.where(mask, normals.view(S, int(count), 3), torch.zeros((), device=x.device))
    return points, normals, valid
