"""MeshRenderer end to end on the C++ twin: what a picture of a known shape must look like, batches against single renders, and the
reference's get_image / set_voxels / set_mesh interface (rendering/__init__.py:110-162, :330-361)."""
import os

import numpy as np
import pytest
import torch

from shapegan_amd import mesh as M
from shapegan_amd.rendering import MeshRenderer, raster
from shapegan_amd.util import crop_image


def sphere_grid(R, radius, centre=(0.0, 0.0, 0.0)):
    """SDF of a sphere sampled where set_voxels places the voxels: index i sits at (i + 1) * 2 / R - 1 (the padded grid)."""
    ax = (torch.arange(R, dtype=torch.float32) + 1) * (2.0 / R) - 1
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    return ((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2).sqrt() - radius


def model_mask(image):
    """Pixels showing the model: its albedo (0.8, 0.1, 0.1) keeps red at least 0.35 above green under every light; floor, shadow and
    background are grey."""
    return image[..., 0].astype(int) - image[..., 1].astype(int) > 40


def is_grey(image):
    return (image[..., 0] == image[..., 1]) & (image[..., 1] == image[..., 2])


@pytest.fixture(scope="module")
def sphere_image():
    v = MeshRenderer(size=200, ssaa=1, shadow_size=256)
    v.set_voxels(sphere_grid(32, 0.5))
    return v, v.get_image()


def test_sphere_default_view(sphere_image):
    v, image = sphere_image
    assert image.shape == (200, 200, 3) and image.dtype == np.uint8
    assert v.model_size == 1.4 and abs(v.ground_level + 0.5) < 1e-3
    # orientation: the centre of the sphere faces the camera and the light: neither culled nor black
    # (ambient alone is 0.5 * 0.8 * 255 = 102 in red; the rim term vanishes for a normal that faces the camera)
    r, g, b = (int(c) for c in image[100, 100])
    assert r > 120 and g < 60 and g == b, image[100, 100]
    # the silhouette: a sphere of radius r on the view axis at distance D projects to a disc of NDC radius f r / sqrt(D^2 - r^2),
    # f = 1.73205 (PROJECTION_MATRIX), D = 2 * 1.4.  Marching cubes puts the vertices on the sphere (the field is an exact distance)
    # and the facets inside it: at h = 1/16 the sagitta h^2 / (8 r) = 1e-3 shrinks the area by 0.4 %; counting whole pixels of a disc
    # of radius 31.4 is good to its perimeter's square root, 0.5 %.  Measured: 3089 pixels against 3104.3, -0.5 % (coverage is exact
    # integer arithmetic: the brute-force reference of tests/raster_reference.py counts the same samples).
    rho = 1.73205081 * 0.5 / np.sqrt(2.8 ** 2 - 0.25)
    disc = np.pi * (rho * 100) ** 2
    area = model_mask(image).sum()
    print("silhouette %d pixels, projected disc %.1f" % (area, disc))
    assert abs(area - disc) <= 0.03 * disc
    ys, xs = np.nonzero(model_mask(image))
    assert abs(xs.mean() - 99.5) < 1.0 and abs(ys.mean() - 99.5) < 1.0
    for corner in ((0, 0), (0, 199), (199, 0), (199, 199)):
        assert tuple(image[corner]) == (255, 255, 255)
    floor = is_grey(image) & (image[..., 0] < 250)
    assert floor.sum() > 100, "the shadow on the floor is missing"
    assert ys.max() < np.nonzero(floor)[0].max()          # the shadow reaches below the sphere on the screen


def test_smooth_normals_face_outward():
    """K12's vertex normals point outward; used as they are (no `* -1`), the side toward the light is lit."""
    batch = M.marching_cubes(sphere_grid(32, 0.5), spacing=2.0 / 32, origin=-1.0)
    v = MeshRenderer(size=64, ssaa=1, shadow_size=128)
    v.set_mesh(batch.mesh(0), smooth=True)
    assert v.model_size == 1.08
    smooth = v.get_image()
    v.set_mesh(batch.mesh(0), smooth=False)
    flat = v.get_image()
    assert smooth[32, 32, 0] > 120 and abs(int(smooth[32, 32, 0]) - int(flat[32, 32, 0])) < 40
    assert np.array_equal(model_mask(smooth), model_mask(flat))
    v.set_mesh(None)
    assert np.array_equal(v.get_image(), flat)
    class Shifted(object):
        vertices, faces, vertex_normals = batch.mesh(0).vertices * 3 + 5, batch.mesh(0).faces, batch.mesh(0).vertex_normals
    v.set_mesh(Shifted, center_and_scale=True)
    assert abs(v.ground_level + 1.0) < 0.05 and model_mask(v.get_image()).sum() > 2 * model_mask(flat).sum()


def test_batch_equals_singles_bit_for_bit():
    grids = torch.stack([sphere_grid(32, 0.5), torch.ones(32, 32, 32), sphere_grid(32, 0.3, (0.2, -0.3, 0.1))])
    v = MeshRenderer(size=72, ssaa=2, shadow_size=128)
    batch = v.render_voxels(grids)
    tensor = v.render_voxels(grids, return_tensor=True)
    assert len(batch) == 3 and tensor.shape == (3, 72, 72, 3) and tensor.dtype == torch.uint8
    for i in range(3):
        single = MeshRenderer(size=72, ssaa=2, shadow_size=128)
        single.set_voxels(grids[i])
        assert np.array_equal(single.get_image(), batch[i]), i
        assert np.array_equal(tensor[i].numpy(), batch[i])
    assert is_grey(batch[1]).all() and (batch[1] == 255).all(axis=2).any()          # the empty grid: floor and background only
    assert model_mask(batch[0]).any() and model_mask(batch[2]).any()
    meshes = v.render_meshes(M.marching_cubes(grids, spacing=2.0 / 32, origin=-1.0))
    assert len(meshes) == 3 and v.model_size == 1.08 and model_mask(meshes[0]).sum() > model_mask(batch[0]).sum()


def test_a_grid_without_sign_change_keeps_the_previous_mesh():
    v = MeshRenderer(size=48, ssaa=1, shadow_size=64)
    v.set_voxels(sphere_grid(16, 0.5))
    before = v.get_image()
    v.set_voxels(torch.ones(16, 16, 16))
    assert np.array_equal(v.get_image(), before)
    v.set_voxels(sphere_grid(16, 0.5).numpy()[None, None])          # arrays and extra unit dimensions
    assert np.array_equal(v.get_image(), before)


def test_supersampling_is_the_block_mean():
    v = MeshRenderer(size=40, ssaa=1, shadow_size=64)
    v.set_voxels(sphere_grid(16, 0.5))
    fine = v.get_image()
    v2 = MeshRenderer(size=20, ssaa=2, shadow_size=64)
    v2.set_voxels(sphere_grid(16, 0.5))
    mean = fine.reshape(20, 2, 20, 2, 3).astype(np.int64).sum(axis=(1, 3))
    assert np.array_equal(v2.get_image(), ((2 * mean + 4) // 8).astype(np.uint8))


def test_get_image_options(tmp_path, monkeypatch):
    v = MeshRenderer(size=64, start_thread=False, ssaa=1, shadow_size=64)
    assert v.rotation == [147, 20] and v.model_color == (0.8, 0.1, 0.1) and v.ground_level == -1 and v.size == 64
    v.set_voxels(sphere_grid(16, 0.5))
    image = v.get_image()
    assert np.array_equal(v.get_image(greyscale=True), image[:, :, 0])
    assert np.array_equal(v.get_image(flip_red_blue=True), image[:, :, ::-1])
    assert np.array_equal(v.get_image(crop=True), crop_image(image))
    small = v.get_image(output_size=32)
    assert small.shape == (32, 32, 3) and small.dtype == np.uint8 and model_mask(small).any()
    v.rotation = [30, 40]
    assert not np.array_equal(v.get_image(), image)
    v.model_color = (0.1, 0.1, 0.9)
    assert not model_mask(v.get_image()).any()
    with pytest.raises(NotImplementedError, match="binary-voxel"):
        v.set_voxels(np.ones((8, 8, 8)), use_marching_cubes=False)
    monkeypatch.chdir(tmp_path)
    v.save_screenshot()
    v.save_screenshot()
    assert sorted(os.listdir("screenshots")) == ["0000.png", "0001.png"]
    v.stop()
    v.delete_buffers()


def test_snapshot_directory(tmp_path):
    from PIL import Image
    v = MeshRenderer(size=48, ssaa=1, shadow_size=64)
    v.snapshot_directory = str(tmp_path / "shots")
    v.set_voxels(sphere_grid(16, 0.5))
    v.set_voxels(sphere_grid(16, 0.4))
    assert sorted(os.listdir(v.snapshot_directory)) == ["000000.png", "000001.png"]
    assert np.array_equal(np.asarray(Image.open(os.path.join(v.snapshot_directory, "000001.png"))), v.get_image())
    assert MeshRenderer.snapshot_directory is None


def test_nothing_to_draw():
    """T = 0, S = 1: no launch of zero size, the picture is floor and background."""
    v = MeshRenderer(size=40, ssaa=2, shadow_size=64)
    image = v.get_image()
    assert image.shape == (40, 40, 3) and is_grey(image).all() and (image == 255).all()          # nothing casts a shadow
    soup = raster.Soup(torch.zeros(0, 3, 3), None, torch.zeros(2, dtype=torch.int64))
    view = raster.draw_view(soup, np.eye(4), 33, 33, cull_back=True, ground=True)
    assert view.nactive == 0 and view.lists.numel() == 0 and view.ground.tolist() == [-1.0] and view.dropped.tolist() == [0]
    assert bool((view.id == -1).all()) and bool((view.depth == 1.0).all()) and int(view.tile_counts.sum()) == 0
