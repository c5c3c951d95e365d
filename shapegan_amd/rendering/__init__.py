"""Rendering (the reference's rendering/ package without pygame and OpenGL): raymarching.render_image sphere-traces SDFNet shapes
(csrc/raymarch.hip); MeshRenderer draws meshes and voxel grids with the tiled rasteriser (csrc/raster.hip, stages in
rendering/raster.py); rendering/math.py has the camera helpers.

MeshRenderer keeps the reference's interface (rendering/__init__.py:54-361) — the constructor arguments, `rotation`, `model_color`,
`model_size`, `ground_level`, `set_voxels`, `set_mesh`, `get_image`, `save_screenshot`, `stop` — but is headless: there is no window,
no thread and no mouse, `get_image` renders on demand.  It adds `render_voxels` / `render_meshes`, which draw a batch of shapes in
one pass, and `snapshot_directory`, which leaves a PNG of every shape a training script shows.

Where it runs follows the data: a CUDA tensor is meshed and drawn by the HIP kernels, a CPU tensor or numpy array by the twin
(`device=` moves everything to one device instead).  Supersampling: the picture is drawn at size * ssaa and every ssaa x ssaa block
averaged on the device — the box resolve of the reference's 4-sample multisampling.
"""
import os

import numpy as np
import torch

from .. import mesh as M
from ..util import crop_image, ensure_directory
from . import raster
from .math import get_camera_transform

DEFAULT_ROTATION = (147, 20)


class MeshRenderer(object):
    snapshot_directory = None      # class-level default: `python -m shapegan_amd.dropin --viewer-dir DIR` sets it before the script runs

    def __init__(self, size=800, start_thread=True, background_color=(1, 1, 1, 1), ssaa=2, shadow_size=1024, device=None):
        del start_thread           # accepted for the reference's call sites: nothing to start
        self.size = int(size)
        self.ssaa = int(ssaa)
        self.shadow_size = int(shadow_size)
        self.device = None if device is None else torch.device(device)
        self.rotation = list(DEFAULT_ROTATION)
        self.model_size = 1
        self.background_color = background_color
        self.model_color = (0.8, 0.1, 0.1)
        self.ground_level = -1
        self.running = True
        self._soup = None
        self._snapshots = 0

    # ---- what is shown ------------------------------------------------------------------------------------------------------------
    def _place(self, t):
        return t if self.device is None else t.to(self.device)

    def _empty_soup(self):
        dev = self.device or torch.device("cpu")
        return raster.Soup(torch.zeros((0, 3, 3), device=dev), None, torch.zeros(2, dtype=torch.int64, device=dev))

    def _show(self, soup):
        self._soup = soup
        self.ground_level = float(soup.positions[:, :, 1].min()) if soup.positions.shape[0] else -1
        if self.snapshot_directory is not None:
            ensure_directory(self.snapshot_directory)
            self._save(os.path.join(self.snapshot_directory, "%06d.png" % self._snapshots), self.get_image())
            self._snapshots += 1

    @staticmethod
    def _grids(voxels):
        if isinstance(voxels, np.ndarray):
            voxels = torch.from_numpy(voxels)
        return voxels.detach()

    def _mesh_voxels(self, grids, pad, level, upscale=None):
        R = grids.shape[-2]        # the reference's voxels.shape[1]
        return M.marching_cubes(self._place(grids), level=level, spacing=2.0 / R, origin=-1.0, pad=bool(pad), upscale=upscale)

    def set_voxels(self, voxels, use_marching_cubes=True, shade_smooth=False, pad=True, level=0, upscale=None):
        """upscale: a zoom factor: the grid goes through the cubic B-spline zoom of shapegan_amd.voxelzoom before it is meshed
        (create_plot.py:826-828); None: it is meshed as it is."""
        if not use_marching_cubes:
            raise NotImplementedError("MeshRenderer.set_voxels(use_marching_cubes=False): the binary-voxel cube mesh "
                                      "(create_binary_voxel_mesh) is not implemented; pass an SDF grid")
        voxels = self._grids(voxels)
        if voxels.dim() > 3:
            voxels = voxels.squeeze()
        if voxels.dim() != 3:
            raise ValueError("set_voxels: expected one grid of rank 3, got %s" % (tuple(voxels.shape),))
        batch = self._mesh_voxels(voxels, pad, level, upscale)
        if batch.faces.shape[0] == 0:
            return                 # no sign change: the previous mesh stays (the reference's `except ValueError: pass`)
        self.model_size = 1.4
        self._show(raster.pack(batch, smooth=shade_smooth))

    def set_mesh(self, mesh, smooth=False, center_and_scale=False):
        if mesh is None:
            return
        vertices = torch.as_tensor(np.asarray(mesh.vertices, dtype=np.float32))
        faces = torch.as_tensor(np.asarray(mesh.faces, dtype=np.int64))
        positions = self._place(vertices)[self._place(faces)]
        if center_and_scale:
            flat = positions.reshape(-1, 3)
            flat = flat - (flat.min(dim=0)[0] + flat.max(dim=0)[0]) / 2
            positions = (flat / flat.norm(dim=1).max()).reshape(-1, 3, 3)
        normals = None
        if smooth:
            normals = self._place(torch.as_tensor(np.asarray(mesh.vertex_normals, dtype=np.float32)))[self._place(faces)]
        self.model_size = 1.08
        offsets = torch.tensor([0, positions.shape[0]], dtype=torch.int64, device=positions.device)
        self._show(raster.Soup(positions, normals, offsets))

    # ---- drawing ------------------------------------------------------------------------------------------------------------------
    def _draw(self, soup, ground=None):
        """[S, size, size, 3] uint8 on the soup's device.  ground: [S] fp32 to use instead of each shape's own min y."""
        light_vp = get_camera_transform(6, self.rotation[0], 50, project=True)
        camera_vp = get_camera_transform(self.model_size * 2, self.rotation[0], self.rotation[1], project=True)
        n = self.size * self.ssaa
        light = raster.draw_view(soup, light_vp, self.shadow_size, self.shadow_size, cull_back=False, shadow=True)
        cam = raster.draw_view(soup, camera_vp, n, n, cull_back=True, ground=ground is None)
        params = raster.shading_params(camera_vp, light_vp, self.model_color, self.background_color)
        samples = raster.shade(soup, cam, light.depth, cam.ground if ground is None else ground, params)
        return raster.resolve(samples, self.ssaa)

    def render_meshes(self, batch, smooth=False, return_tensor=False):
        """Draws every mesh of a MeshBatch in one pass, each over its own ground level: a list of [size, size, 3] uint8 arrays, or
        the tensor [S, size, size, 3] on the batch's device."""
        self.model_size = 1.08
        return self._finish(self._draw(raster.pack(batch, smooth=smooth)), return_tensor)

    def render_voxels(self, grids, shade_smooth=False, pad=True, level=0, return_tensor=False, upscale=None):
        """The same for SDF grids [S, R, R, R]; a grid without a sign change gives floor and background only.  upscale: as set_voxels."""
        grids = self._grids(grids)
        if grids.dim() != 4:
            raise ValueError("render_voxels: expected [S, R, R, R], got %s" % (tuple(grids.shape),))
        self.model_size = 1.4
        return self._finish(self._draw(raster.pack(self._mesh_voxels(grids, pad, level, upscale), smooth=shade_smooth)), return_tensor)

    @staticmethod
    def _finish(images, return_tensor):
        return images if return_tensor else list(images.cpu().numpy())

    def get_image(self, crop=False, output_size=None, greyscale=False, flip_red_blue=False):
        soup = self._soup if self._soup is not None else self._empty_soup()
        ground = torch.full((1,), float(self.ground_level), dtype=torch.float32, device=soup.device)
        array = self._draw(soup, ground=ground)[0].cpu().numpy()
        if output_size is None:
            output_size = self.size
        if greyscale:
            array = array[:, :, 0]
        elif flip_red_blue:
            array = array[:, :, ::-1]
        array = np.ascontiguousarray(array)
        if crop:
            array = crop_image(array)
        if output_size != self.size:
            from PIL import Image
            array = np.asarray(Image.fromarray(array).resize((output_size, output_size), Image.BICUBIC))
        return array

    @staticmethod
    def _save(filename, array):
        from PIL import Image
        Image.fromarray(array).save(filename)

    def save_screenshot(self):
        ensure_directory('screenshots')
        index = 0
        while os.path.isfile("screenshots/{:04d}.png".format(index)):
            index += 1
        filename = "screenshots/{:04d}.png".format(index)
        self._save(filename, self.get_image())
        print("Screenshot saved to " + filename + ".")

    def delete_buffers(self):
        pass

    def stop(self):
        self.running = False
