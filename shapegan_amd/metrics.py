"""Point-cloud sampling of generated and dataset shapes for evaluation (metrics.py:1-46 of the reference), batched on the device.

The reference meshes each shape with skimage and samples it with trimesh in a Python loop of `sample_count` iterations.  Here a
chunk of shapes goes through one SDFNet launch (the voxel grid shared by every shape), one marching-cubes call and one sampling
launch (shapegan_amd.mesh); only the finished point clouds come back to the host.  Signatures, defaults, coordinates and return
values (numpy [S, P, 3], float64) are the reference's; an empty mesh leaves zeros and prints the reference's warning.  The
reference's `if '...' in sys.argv` script blocks (file I/O, pyrender) are not ported.
"""
import numpy as np
import torch

from .brickgrid import options as narrow_band_options
from .mesh import marching_cubes, max_shapes_per_call
from .model import LATENT_CODE_SIZE
from .util import device, standard_normal_distribution

LEVEL = 0

# points of one SDFNet launch of sample_point_clouds (64 M: a 256 MB output; the reference's default 128^3 grid is 2 M per shape)
_MAX_GRID_POINTS = 1 << 26


def rescale_point_cloud(point_cloud, method=None):
    if method == 'half_unit_sphere':
        point_cloud /= np.linalg.norm(point_cloud, axis=1).max() * 2
    elif method == 'half_unit_cube':
        point_cloud /= np.abs(point_cloud).max() * 2


def _collect(result, begin, points, empty, rescale):
    points, empty = points.cpu().numpy(), empty.cpu().numpy()
    for i in range(points.shape[0]):
        if empty[i]:
            print("Warning: Empty mesh.")
            continue
        point_cloud = points[i].astype(np.float64)
        rescale_point_cloud(point_cloud, method=rescale)
        result[begin + i, :, :] = point_cloud


def shapes_per_chunk(voxel_resolution, padded_grid):
    """Shapes evaluated, meshed and sampled together: bounded by the meshing call's int32 limits and by _MAX_GRID_POINTS."""
    g = voxel_resolution + (2 if padded_grid else 0)
    return max(1, min(max_shapes_per_call((g, g, g), pad=True), _MAX_GRID_POINTS // voxel_resolution ** 3))


def sample_point_clouds(sdf_net, sample_count, point_cloud_size, voxel_resolution=128, rescale='half_unit_sphere', latent_codes=None,
                        narrow_band=False, generator=None, clean=False):
    """get_uniform_surface_points(z, point_cloud_size, voxel_resolution, sphere_only=False, level=LEVEL) + rescale for
    `sample_count` latent codes (standard normal when None), in chunks of shapes_per_chunk(voxel_resolution, True).
    narrow_band: the grids come from the brick path of SDFNet.voxel_grids, built for LEVEL (True, or a dict of its
    arguments brick / band / lipschitz; voxel_resolution a multiple of the brick).
    generator: the torch.Generator of the surface samples (default: the device's own).
    clean: a rule of topology.clean_meshes ("largest", True, a dict): the clouds are sampled from the cleaned meshes."""
    result = np.zeros((sample_count, point_cloud_size, 3))
    if latent_codes is None:
        latent_codes = standard_normal_distribution.sample((sample_count, LATENT_CODE_SIZE)).to(device)
    size = 2
    chunk = shapes_per_chunk(voxel_resolution, True)
    for begin in range(0, sample_count, chunk):
        z = latent_codes[begin:min(begin + chunk, sample_count)]
        grids = sdf_net.voxel_grids(z, voxel_resolution, sphere_only=False, level=LEVEL, **narrow_band_options(narrow_band))
        batch = marching_cubes(grids, level=LEVEL, spacing=size / voxel_resolution, origin=-size / 2, pad=True, pad_value=1.0)
        if clean:
            batch = batch.clean(clean)
        points, empty = batch.sample_surface(point_cloud_size, generator=generator, return_empty=True)
        _collect(result, begin, points, empty, rescale)
    return result


def sample_from_voxels(voxels, point_cloud_size, rescale='half_unit_sphere', clean=False, upscale=None, redistance=False):
    """Meshes each voxel grid of `voxels` [B,R,R,R] (numpy or tensor) padded with 1 at level 0 and samples it
    (metrics.py:31-46); computed on `util.device`.  clean: as sample_point_clouds.
    upscale: a zoom factor: every grid goes through the cubic B-spline zoom of shapegan_amd.voxelzoom before it is meshed
    (marching_cubes(upscale=), create_plot.py:826-828); the chunks are sized by the upscaled resolution.
    redistance: marching_cubes(redistance=): the grids get their distances back beyond the truncation before they are meshed."""
    result = np.zeros((voxels.shape[0], point_cloud_size, 3))
    size = 2
    voxel_resolution = voxels.shape[1]
    if isinstance(voxels, np.ndarray):
        voxels = torch.from_numpy(voxels)
    voxels = voxels.to(device=device, dtype=torch.float32)
    chunk = shapes_per_chunk(voxel_resolution if upscale is None else int(round(voxel_resolution * upscale)), False)
    for begin in range(0, voxels.shape[0], chunk):
        batch = marching_cubes(voxels[begin:begin + chunk], level=0, spacing=size / voxel_resolution, origin=-size / 2, pad=True,
                               pad_value=1.0, upscale=upscale, redistance=redistance)
        if clean:
            batch = batch.clean(clean)
        points, empty = batch.sample_surface(point_cloud_size, return_empty=True)
        _collect(result, begin, points, empty, rescale)
    return result
