"""DeepSDF decoder `SDFNet` (model/sdf_net.py:23-61 + inference helpers :63-95,118-156) on the fused MFMA kernel.

state_dict keys: `layers1.{0,2,4,6}.{weight,bias}`, `layers2.{0,2,4,6}.{weight,bias}` — the shipped
examples/gan_generator_voxels_*.to checkpoints load unchanged.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..mesh import marching_cubes
from ..brickgrid import options as narrow_band_options
from ..util import get_points_in_unit_sphere, get_voxel_coordinates
from . import LATENT_CODE_SIZE, LATENT_CODES_FILENAME, SavableModule  # noqa: F401  (re-exported: train_sdf_autodecoder.py:13)

SDF_NET_BREADTH = 256


class SDFVoxelizationHelperData(object):
    """Cached sample grid (and unit-sphere mask, |p| < 1.1) per resolution — model/sdf_net.py:7-19."""

    def __init__(self, device, voxel_resolution, sphere_only=True):
        sample_points = get_voxel_coordinates(voxel_resolution)
        if sphere_only:
            unit_sphere_mask = np.linalg.norm(sample_points, axis=1) < 1.1
            sample_points = sample_points[unit_sphere_mask, :]
            self.unit_sphere_mask = unit_sphere_mask.reshape(voxel_resolution, voxel_resolution, voxel_resolution)
        self.sample_points = torch.tensor(sample_points, device=device)
        self.point_count = self.sample_points.shape[0]


sdf_voxelization_helper = dict()


def _mlp(sizes, last_act):
    mods = []
    for i in range(len(sizes) - 1):
        mods.append(nn.Linear(in_features=sizes[i], out_features=sizes[i + 1]))
        mods.append(nn.ReLU(inplace=True) if i + 2 < len(sizes) else last_act)
    return nn.Sequential(*mods)


class SDFNet(SavableModule):
    def __init__(self, latent_code_size=LATENT_CODE_SIZE, device='cuda'):
        super().__init__(filename="sdf_net.to")
        b = SDF_NET_BREADTH
        self.latent_code_size = latent_code_size
        # parameter containers only; the forward below never calls them (model/sdf_net.py:26-52)
        self.layers1 = _mlp([3 + latent_code_size, b, b, b, b], nn.ReLU(inplace=True))
        self.layers2 = _mlp([b + latent_code_size + 3, b, b, b, 1], nn.Tanh())
        self._pack_points = ops._PackCache()
        self._pack_shapes = ops._PackCache()
        if device == 'cuda' and not torch.cuda.is_available():
            device = 'cpu'  # construct-only (state_dict / checkpoint handling); forward needs the GPU
        self.to(device)

    def _params(self):
        out = []
        for seq in (self.layers1, self.layers2):
            for i in (0, 2, 4, 6):
                out += [seq[i].weight, seq[i].bias]
        return out

    def forward(self, points, latent_codes):
        """points [N,3], latent_codes [N,L] -> sdf [N]   (model/sdf_net.py:56-61)."""
        return ops.SDFNetPoints.apply(self._pack_points, points, latent_codes, torch.is_grad_enabled(), *self._params()).squeeze()

    def forward_shapes(self, points, latent_codes, points_per_shape):
        """points [S*pps,3], latent_codes [S,L] -> sdf [S*pps]: row s*pps+q uses latent s.  Same function as
        forward(points, latent.repeat_interleave(pps)) without materialising the tiled latents."""
        return ops.SDFNetShapes.apply(self._pack_shapes, points, latent_codes, int(points_per_shape), None, None, None,
                                      torch.is_grad_enabled(), *self._params())

    def prepare_latents(self, latent_table):
        """Weight pack (if stale) and per-shape latent fold for the forward_shapes / forward_segments call that follows with the same
        table — lets a trainer run them next to its batch assembly (ops._PackCache.prepare_fold)."""
        self._pack_shapes.prepare_fold(self._params(), latent_table)

    def forward_segments(self, points, latent_table, shape_index, segment_offsets, latent_reg=None):
        """points [N,3] grouped by shape, latent_table [S,L], shape_index [N] (int32), segment_offsets [S+1] (int64):
        sdf[i] = SDFNet(points[i], latent_table[shape_index[i]]).  The auto-decoder's latent_codes[model_indices]
        gather (train_sdf_autodecoder.py:80) without the [N,L] tensor: latent columns fold into per-shape biases and
        the latent-table gradient comes out dense, [S,L], from per-shape sums.
        latent_reg: None or (row_weight [S] | None, scale): the backward adds row_weight[s] * scale * latent_table[s] to the latent
        gradient (see ops.SDFNetShapes)."""
        return ops.SDFNetShapes.apply(self._pack_shapes, points, latent_table, 0, shape_index, segment_offsets, latent_reg,
                                      torch.is_grad_enabled(), *self._params())

    def latent_loss_and_grad(self, points, sdf, latent_table, segment_offsets, cutoff=0.1, sigma=0.0, window=None, fused=True):
        """The objective a latent code is fitted with, and its gradient, the weights frozen: points [N,3] grouped by shape, sdf [N],
        latent_table [S,L], segment_offsets [S+1] (int64) ->
            loss [S]   = mean_p |SDFNet(x_p, z_s) - clamp(sdf_p, +-cutoff)|   (the data term only)
            grad [S,L] = d/dz_s (loss_s + sigma * mean_k z_{s,k}^2).
        window = (start, count): shape s uses min(count, n_s) of its n_s points (count <= 0: all), the i-th being
        (start + i) mod n_s.  fused: one launch runs forward, loss and the latent-only backward of a tile (csrc/latent_fit.hip);
        False composes the same from forward_segments and autograd.  No parameter is touched, no .grad written."""
        off = ops.check_segments(points, sdf, latent_table, segment_offsets)
        start, count = (0, 0) if window is None else (int(window[0]), int(window[1]))
        if start < 0:
            raise ValueError("the window starts at %d" % start)
        if fused:
            fit = ops.LatentFit(self._pack_shapes, self._params(), points, sdf, segment_offsets, off, cutoff)
            return fit.step(latent_table, start, count, sigma)
        return ops.latent_step_composed(self._pack_shapes, self._params(), points, sdf, latent_table, off, cutoff, sigma, start, count)

    def latent_pose_loss_and_grad(self, points, sdf, latent_table, poses, segment_offsets, cutoff=0.1, sigma=0.0, window=None):
        """latent_loss_and_grad for clouds in their own frame: points [N,3] are OBSERVED coordinates q and poses [S,16] hold, per
        shape, the row-major 3x4 affine A|t to the canonical frame (x = A q + t) and at float 12 the scale ts of the targets ->
            loss [S]         = mean_p |SDFNet(A q_p + t, z_s) - clamp(ts sdf_p, +-cutoff)|
            grad_z [S,L]     = d/dz_s (loss_s + sigma * mean_k z_{s,k}^2)
            grad_pose [S,16] = d loss_s / d poses[s] (floats 13..15 zero).
        One fused launch per chunk of shapes (csrc/latent_fit.hip); the point gradient it contracts never leaves the chip."""
        off = ops.check_segments(points, sdf, latent_table, segment_offsets)
        ops.check_poses(poses, latent_table.shape[0], points.device)
        start, count = (0, 0) if window is None else (int(window[0]), int(window[1]))
        if start < 0:
            raise ValueError("the window starts at %d" % start)
        fit = ops.LatentPoseFit(self._pack_shapes, self._params(), points, sdf, segment_offsets, off, cutoff)
        return fit.step(latent_table, poses, start, count, sigma)

    def surface_projector(self, latent_codes):
        """ops.SurfaceProjector for these codes [S,L] (or one code [L]): weight image and latent fold made once, for callers that
        project many batches of points onto the same shapes."""
        return ops.SurfaceProjector(self._pack_shapes, self._params(), latent_codes)

    def _project(self, points, latent_codes, segment_offsets, **kw):
        proj = self.surface_projector(latent_codes)
        off = ops.check_point_segments(points, proj.S, segment_offsets)
        seg_off = torch.from_numpy(off).to(points.device) if segment_offsets is None else segment_offsets.contiguous()
        return proj.run(points, off, seg_off, **kw)

    def sdf_and_gradient(self, points, latent_codes, segment_offsets=None):
        """points [N,3] grouped by shape, latent_codes [S,L] (or [L]: one shape owns all points) -> (sdf [N], grad [N,3]): the
        network's value and its unnormalised gradient with respect to the point, from one fused launch (csrc/sdfnet_project.hip)
        that keeps nothing of the forward but sign bits on the chip.  segment_offsets [S+1] (int64): shape s owns the points
        [off[s], off[s+1]); None: N = S * pps, equal runs.  No autograd graph is built, no .grad is written, `points` is left as
        it is (model/sdf_net.py:118-128 takes the same gradient through autograd and normalises it)."""
        _, sdf, grad = self._project(points, latent_codes, segment_offsets, iterations=0)
        return sdf, grad

    def project_to_level_set(self, points, latent_codes, segment_offsets=None, level=0.0, iterations=5, rule="newton", max_step=0.1):
        """Moves every point toward f(., z_s) = level by `iterations` steps along the gradient, all in one launch:
        rule "newton": x -= (f - level) g / |g|^2; "unit": x -= (f - level) g / |g|, the reference's step, which takes |g| = 1 for
        granted (model/sdf_net.py:146).  A step longer than max_step is cut to it (0: no limit); where g = 0 the point stays.
        -> (points [N,3] (new), sdf [N] and grad [N,3] at the returned points).  Arguments as in sdf_and_gradient."""
        return self._project(points, latent_codes, segment_offsets, level=level, iterations=iterations, rule=rule, max_step=max_step)

    # ---- inference helpers (reference signatures) ----
    def evaluate_in_batches(self, points, latent_code, batch_size=100000, return_cpu_tensor=True):
        """One latent for all points (model/sdf_net.py:63-75).  The fused kernel streams any N in one launch, so
        `batch_size` only bounds the launch size."""
        n = points.shape[0]
        with torch.no_grad():
            z = latent_code.reshape(1, -1)
            result = torch.empty(n, dtype=torch.float32, device=points.device)
            for begin in range(0, n, batch_size):
                chunk = points[begin:begin + batch_size]
                result[begin:begin + chunk.shape[0]] = self.forward_shapes(chunk, z, chunk.shape[0])
        return result.cpu() if return_cpu_tensor else result

    def _helper(self, voxel_resolution, sphere_only):
        key = (voxel_resolution, sphere_only)
        # (one grid per resolution, as in the reference; remade when a network on another device asks for it)
        if key not in sdf_voxelization_helper or sdf_voxelization_helper[key].sample_points.device != self.device:
            sdf_voxelization_helper[key] = SDFVoxelizationHelperData(self.device, voxel_resolution, sphere_only)
        return sdf_voxelization_helper[key]

    def get_voxels(self, latent_code, voxel_resolution, sphere_only=True, pad=True):
        """SDF voxel grid; outside the |p|<1.1 sphere the grid is 1 (model/sdf_net.py:77-95)."""
        helper = self._helper(voxel_resolution, sphere_only)
        distances = self.evaluate_in_batches(helper.sample_points, latent_code).numpy()
        if sphere_only:
            voxels = np.ones((voxel_resolution,) * 3, dtype=np.float32)
            voxels[helper.unit_sphere_mask] = distances
        else:
            voxels = distances.reshape(voxel_resolution, voxel_resolution, voxel_resolution)
            if pad:
                voxels = np.pad(voxels, 1, mode='constant', constant_values=1)
        return voxels

    def grid_values(self, latent_codes, points):
        """SDF of every shape at every point of one shared grid: latent_codes [S,L], points [P,3] -> [S,P] on the points' device.
        One sg_sdfnet_fwd launch with points_period = P: the grid is not tiled S times.  Any P and S: where a 64-point tile could
        straddle two shapes (several shapes of P points, P no multiple of 128: every sphere-masked grid) each point names its
        shape, as in forward_segments."""
        z = ops.f32c(latent_codes.detach().reshape(-1, self.latent_code_size))
        points = ops.f32c(points)
        S, P = z.shape[0], points.shape[0]
        with torch.no_grad():
            packed, zb1, zb5 = self._pack_shapes.get_with_fold(self._params(), z)
            out = torch.empty((S, P), dtype=torch.float32, device=points.device)
            sid = None
            if S > 1 and P % 128 != 0:
                sid = torch.arange(S, dtype=torch.int32, device=points.device).repeat_interleave(P)
            lib = ops._lib()
            ops.check(lib.sg_sdfnet_fwd(ops.ptr(points), P, None, None, z.shape[1], ops.ptr(packed), 3, ops.ptr(zb1), ops.ptr(zb5), P,
                                        ops.ptr(sid), ops.ptr(out), None, S * P, S * P, ops.stream()), "sdfnet_fwd")
        return out

    def voxel_grids(self, latent_codes, voxel_resolution, sphere_only=True, pad=True, narrow_band=False, level=0, brick=4, band=None,
                    lipschitz=1.0, return_stats=False):
        """get_voxels for a batch of latent codes [S,L], built on the device without a host round trip: [S,R,R,R], or
        [S,R+2,R+2,R+2] when not sphere_only and pad (the same values as get_voxels, shape by shape).

        narrow_band: the network runs only in bricks of brick^3 points (4, 8 or 16; R a multiple of it) near the `level` set; every
        other brick holds one constant (shapegan_amd/brickgrid.py; the rule and its guarantee: include/shapegan_hip.h, K18).  Same
        shape, dtype, device and padding; marching cubes of it at `level` is bit for bit that of the dense grid, apart from
        pieces smaller than a brick that no brick corner came within `band` (default: lipschitz * sqrt(3) (brick - 1) / 2 lattice
        steps) of.  brick defaults to 4, the one size that was never slower than the dense path in DESIGN 3.15's table (8 is the
        faster one at 256^3).  The grid is only good for the level it was built for.  Unlike the dense path this one reads a count back from the
        device once per round of its continuation: it synchronises, as marching_cubes does, and is not meant for graph capture.
        return_stats: (grids, stats) with stats = {"evaluated_points": per shape, "rounds", "active_bricks": per shape, ...}."""
        helper = self._helper(voxel_resolution, sphere_only)
        R = voxel_resolution
        if narrow_band:
            grids, stats = self._narrow_band_grids(latent_codes, helper, R, sphere_only, pad, level, brick, band, lipschitz)
        else:
            d = self.grid_values(latent_codes, helper.sample_points)
            S = d.shape[0]
            stats = {"resolution": R, "rounds": 0, "active_bricks": None, "evaluated_points": [helper.point_count] * S,
                     "dense_points": R ** 3}
            if sphere_only:
                grids = torch.ones((S, R * R * R), dtype=torch.float32, device=d.device)
                grids[:, self._mask_tensor(helper, d.device)] = d
                grids = grids.view(S, R, R, R)
            else:
                grids = d.view(S, R, R, R)
        if not sphere_only and pad:
            grids = torch.nn.functional.pad(grids, (1, 1, 1, 1, 1, 1), mode='constant', value=1.0)
        return (grids, stats) if return_stats else grids

    @staticmethod
    def _mask_tensor(helper, device):
        if getattr(helper, "unit_sphere_mask_t", None) is None or helper.unit_sphere_mask_t.device != device:
            helper.unit_sphere_mask_t = torch.from_numpy(helper.unit_sphere_mask.reshape(-1)).to(device)
        return helper.unit_sphere_mask_t

    def point_evaluator(self, latent_codes):
        """evaluate(points [N,3], shape_index [N] int32) -> sdf [N] for the codes [S,L]: one sg_sdfnet_fwd launch per call, each point
        with the folded biases of the shape it names.  A point gets the same bits wherever it stands in a launch (the k order of
        every layer and the last layer's 16-row groups are fixed per point: csrc/sdfnet_tile.h), and the same as grid_values."""
        z = ops.f32c(latent_codes.detach().reshape(-1, self.latent_code_size))
        lib = ops._lib()
        with torch.no_grad():
            packed, zb1, zb5 = self._pack_shapes.get_with_fold(self._params(), z)

        def evaluate(points, shape_index):
            n = points.shape[0]
            out = torch.empty(n, dtype=torch.float32, device=points.device)
            ops.check(lib.sg_sdfnet_fwd(ops.ptr(points), 0, None, None, z.shape[1], ops.ptr(packed), 3, ops.ptr(zb1), ops.ptr(zb5), n,
                                        ops.ptr(shape_index), ops.ptr(out), None, n, n, ops.stream()), "sdfnet_fwd")
            return out
        return evaluate, z.shape[0]

    def _narrow_band_grids(self, latent_codes, helper, R, sphere_only, pad, level, brick, band, lipschitz):
        from ..brickgrid import check_arguments, narrow_band_grids
        check_arguments(latent_codes.reshape(-1, self.latent_code_size).shape[0], R, brick, None, band)
        dev = helper.sample_points.device
        evaluate, S = self.point_evaluator(latent_codes)
        mask = self._mask_tensor(helper, dev) if sphere_only else None
        with torch.no_grad():
            result = narrow_band_grids(evaluate, S, R, dev, brick=brick, level=level, band=band, lipschitz=lipschitz, pad=pad, mask=mask)
        return result.grid, result.stats

    def get_mesh(self, latent_code, voxel_resolution=64, sphere_only=True, raise_on_empty=False, level=0, narrow_band=False, refine=0,
                 clean=False, simplify=None):
        """Marching cubes of the SDF grid (model/sdf_net.py:97-112) on the device: a mesh.Mesh, None when the grid does not cross
        `level` (ValueError with raise_on_empty).  Coordinates are the reference's: the grid of get_voxels padded once more with
        1, spacing 2 / R, shifted by -1 — grid index i lands at (i + 1 + t) 2/R - 1 (sphere_only) or (i + 2 + t) 2/R - 1 (the
        grid get_voxels pads itself).  narrow_band: the grid is built for `level` by the brick path of voxel_grids (True, or a dict
        of its arguments brick / band / lipschitz).  refine = K > 0: every vertex is then moved onto the network's own level set by K
        Newton steps and given its exact normal (surface.refine_meshes, at most a cell diagonal away); 0 is the marching-cubes mesh.
        clean: a rule of topology.clean_meshes ("largest", True, a dict) applied to the marching-cubes mesh before refine; a mesh of
        which nothing is left counts as empty.  False: no cleaning.  simplify: an int (the most triangles to keep) or a dict of the
        arguments of simplify.simplify_meshes, applied last, after clean and refine (a grid so coarse that no triangle
        survives gives a Mesh without triangles, not None); None: the mesh as it is."""
        size = 2
        grids = self.voxel_grids(latent_code.reshape(1, -1), voxel_resolution, sphere_only=sphere_only, level=level,
                                 **narrow_band_options(narrow_band))
        batch = marching_cubes(grids, level=level, spacing=size / voxel_resolution, origin=-size / 2, pad=True, pad_value=1.0)
        if clean:
            batch = batch.clean(clean)
        if batch.faces.shape[0] == 0:
            if raise_on_empty:
                raise ValueError("Surface level must be within volume data range.")
            return None
        if refine:
            from ..surface import cell_diagonal, refine_meshes
            batch, _ = refine_meshes(self, latent_code.reshape(1, -1), batch, level=level, iterations=int(refine),
                                     max_move=cell_diagonal(voxel_resolution))
        if simplify is not None and simplify is not False:
            from ..simplify import apply_option
            batch = apply_option(batch, simplify)
        return batch.mesh(0)

    def get_uniform_surface_points(self, latent_code, point_count=1000, voxel_resolution=64, sphere_only=True, level=0,
                                   narrow_band=False, clean=False):
        """get_mesh(...).sample(point_count) (model/sdf_net.py:114-116): AttributeError when the mesh is empty, as there."""
        mesh = self.get_mesh(latent_code, voxel_resolution=voxel_resolution, sphere_only=sphere_only, level=level,
                             narrow_band=narrow_band, clean=clean)
        return mesh.sample(point_count)

    def get_normals(self, latent_code, points):
        """d sdf / d points, normalised (model/sdf_net.py:118-128)."""
        if latent_code.requires_grad or points.requires_grad:
            raise Exception('get_normals may only be called with tensors that don\'t require grad.')
        points.requires_grad = True
        sdf = self.forward_shapes(points, latent_code.reshape(1, -1), points.shape[0])
        sdf.backward(torch.ones(sdf.shape[0], device=self.device))
        normals = points.grad
        normals /= torch.norm(normals, dim=1).unsqueeze(dim=1)
        return normals

    def get_surface_points(self, latent_code, sample_size=100000, sdf_cutoff=0.1, return_normals=False,
                           use_unit_sphere=True):
        """Project random samples onto the zero level set along the SDF gradient (model/sdf_net.py:130-156)."""
        if use_unit_sphere:
            points = get_points_in_unit_sphere(n=sample_size, device=self.device) * 1.1
        else:
            points = torch.rand((sample_size, 3), device=self.device) * 2.2 - 1
        points.requires_grad = True
        sdf = self.forward_shapes(points, latent_code.reshape(1, -1), points.shape[0])
        sdf.backward(torch.ones((sdf.shape[0]), device=self.device))
        normals = points.grad
        normals /= torch.norm(normals, dim=1).unsqueeze(dim=1)
        points.requires_grad = False
        points -= normals * sdf.detach().unsqueeze(dim=1)
        mask = (torch.abs(sdf) < sdf_cutoff) & torch.all(torch.isfinite(points), dim=1)
        points, normals = points[mask, :], normals[mask, :]
        return (points, normals) if return_normals else points

    def get_surface_points_in_batches(self, latent_code, amount=1000):
        result = torch.zeros((amount, 3), device=self.device)
        position, tries = 0, 20
        while position < amount and tries > 0:
            points = self.get_surface_points(latent_code, sample_size=amount * 6)
            used = min(amount - position, points.shape[0])
            result[position:position + used, :] = points[:used, :]
            position += used
            tries -= 1
        return result
