"""Encoding unseen shapes with a trained DeepSDF auto-decoder: fit latent codes to SDF samples with the network frozen, then mesh them.

An auto-decoder (model/sdf_net.py, train_sdf_autodecoder.py) has no encoder: the only shapes with a latent code are the rows of the
training table.  The code of a new shape is the minimiser of

    mean_p |SDFNet(x_p, z) - clamp(sdf_p, +-cutoff)| + sigma * mean_k z_k^2

over z (Park et al., DeepSDF, section 4.2 / eq. 10).  The reference never wrote this step (create_plot.py's sdf_net_reconstruction only renders
training codes).  fit_latent_codes runs it for a batch of shapes at once — every shape is independent — on the fused kernel of
csrc/latent_fit.hip (SDFNet.latent_loss_and_grad), with Adam through sg_adam_step; reconstruct_meshes turns codes into a MeshBatch.

    python -m shapegan_amd.reconstruct --net models/sdf_net.to --models DIR --out codes.to [--meshes OUTDIR] [--chamfer]
    python -m shapegan_amd.reconstruct --net models/sdf_net.to --clouds DIR --out codes.to       # point clouds: .npy, .xyz, .ply
    python -m shapegan_amd.reconstruct --net models/sdf_net.to --models DIR --partial 5 --out codes.to --chamfer     # shape completion

    python -m shapegan_amd.reconstruct --net models/sdf_net.to --clouds DIR --pose similarity --pose-starts 4 --out codes.to --poses-out poses.to

--clouds and --partial fit to the SDF of an oriented point cloud (shapegan_amd.cloudsdf, mesh_to_sdf's 'normal' sign) instead of a mesh's.
--pose fits a pose per shape together with its code (fit_codes_and_poses, csrc/latent_fit.hip): a partial scan's bounding sphere is
not the object's and a sensor's cloud is not upright, and the network is the only model of where the shape should be.
"""
import argparse
import os
import sys

import torch

from . import lib as L
from . import ops
from .brickgrid import options as narrow_band_options
from .mesh import marching_cubes


def _segments(points, sdf, segment_offsets, points_per_shape):
    """points [N,3] / sdf [N] with runs, from either calling form ([S,P,3] / [S,P] batches, or flat tensors with offsets or a fixed
    run length)."""
    if points.dim() == 3:
        S, P = points.shape[0], points.shape[1]
        points, sdf = points.reshape(S * P, 3), sdf.reshape(S * P)
        points_per_shape = P
    if segment_offsets is None:
        if not points_per_shape or points.shape[0] % int(points_per_shape):
            raise ValueError("fit_latent_codes: give segment_offsets, or points_per_shape dividing the %d points" % points.shape[0])
        segment_offsets = torch.arange(points.shape[0] // int(points_per_shape) + 1, dtype=torch.int64) * int(points_per_shape)
    return points, sdf, segment_offsets.to(device=points.device, dtype=torch.int64)


def fit_latent_codes(sdf_net, points, sdf, segment_offsets=None, points_per_shape=None, iterations=800, lr=5e-3, sigma=0.01, cutoff=0.1,
                     init=None, points_per_step=None, shuffle=True, seed=0, fused=True):
    """Latent codes [S,L] of S shapes from their SDF samples, and the data term [S] at those codes (one evaluation over all points).

    points [N,3] / sdf [N] grouped by shape with segment_offsets [S+1] (int64) or a fixed points_per_shape, or batches [S,P,3] /
    [S,P].  Adam with torch's defaults; init None starts from zeros.  points_per_step: iteration k uses the window
    (k * points_per_step, points_per_step) of every shape's samples, wrapping around (None: all points every iteration); shuffle
    permutes every shape's samples once, seeded, on the device, so that the windows are random mini-batches.  The network's
    parameters are not touched and no .grad of theirs is written.  fused=False runs the same loop on forward_segments + autograd."""
    points, sdf, seg = _segments(points, sdf, segment_offsets, points_per_shape)
    points, sdf = L.f32c(points.detach()), L.f32c(sdf.detach())
    S, Lz, dev = seg.numel() - 1, sdf_net.latent_code_size, points.device
    z = torch.zeros((S, Lz), dtype=torch.float32, device=dev) if init is None else L.f32c(init.detach().to(dev)).clone()
    off = ops.check_segments(points, sdf, z, seg)
    if shuffle and points_per_step:
        # one permutation per shape: sort random keys inside every run (the shape index is the major key)
        g = torch.Generator(device=dev).manual_seed(int(seed))
        sid = torch.repeat_interleave(torch.arange(S, device=dev), (seg[1:] - seg[:-1]))
        lo, hi = int(off[0]), int(off[-1])
        order = torch.argsort(sid.double() + torch.rand(hi - lo, generator=g, device=dev, dtype=torch.float64) * 0.5) + lo
        points, sdf = points.clone(), sdf.clone()
        points[lo:hi], sdf[lo:hi] = points[order], sdf[order]
    params = sdf_net._params()
    count = int(points_per_step) if points_per_step else 0
    if fused:
        fit = ops.LatentFit(sdf_net._pack_shapes, params, points, sdf, seg, off, cutoff)

        def step(start, cnt, sg):
            return fit.step(z, start, cnt, sg)
    else:
        composed = ops.LatentFitComposed(sdf_net._pack_shapes, params, points, sdf, off, cutoff)

        def step(start, cnt, sg):
            return composed.step(z, start, cnt, sg)
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    lib = ops._lib()
    for k in range(int(iterations)):
        _, grad = step(k * count, count, sigma)
        ops.check(lib.sg_adam_step(ops.ptr(z), ops.ptr(grad), ops.ptr(m), ops.ptr(v), z.numel(), float(lr), 0.9, 0.999, 1e-8, k + 1, 1.0,
                                   ops.stream()), "adam_step")
    loss, _ = step(0, 0, 0.0)
    return z, loss


# ---- pose with the code: clouds in an unknown similarity frame (csrc/latent_fit.hip) ------------------------------------------------
# which of (rotation vector, translation, log scale) a pose model leaves free
POSE_MODELS = {"translation": (False, True, False), "translation+scale": (False, True, True), "rigid": (True, True, False),
               "similarity": (True, True, True)}


def rotation_matrices(omega):
    """R(omega) [S,3,3] of rotation vectors [S,3] (Rodrigues): I + a K + b K^2 with K the cross-product matrix, a = sin(th) / th,
    b = (1 - cos(th)) / th^2 = (sin(th/2) / (th/2))^2 / 2; below th^2 = 1e-6 both by their series, so the map and its autograd are exact
    at omega = 0."""
    x = (omega * omega).sum(dim=1)
    small = x < 1e-6
    th = torch.where(small, torch.ones_like(x), x).sqrt()
    half = torch.sin(0.5 * th) / (0.5 * th)
    a = torch.where(small, 1 - x / 6 + x * x / 120, torch.sin(th) / th)
    b = torch.where(small, 0.5 - x / 24 + x * x / 720, 0.5 * half * half)
    zero = torch.zeros_like(x)
    wx, wy, wz = omega[:, 0], omega[:, 1], omega[:, 2]
    K = torch.stack([zero, -wz, wy, wz, zero, -wx, -wy, wx, zero], dim=1).reshape(-1, 3, 3)
    eye = torch.eye(3, dtype=omega.dtype, device=omega.device).expand_as(K)
    return eye + a[:, None, None] * K + b[:, None, None] * (K @ K)


def pose_rows(theta):
    """theta [S,7] = (rotation vector, translation, log s) -> the kernel's pose rows [S,16]: A = s R(omega) and t as a row-major 3x4,
    ts = s at float 12, zeros behind.  Small batched torch; autograd carries the kernel's grad_pose back to theta."""
    s = theta[:, 6].exp()
    A = s[:, None, None] * rotation_matrices(theta[:, 0:3])
    At = torch.cat([A, theta[:, 3:6, None]], dim=2).reshape(-1, 12)
    return torch.cat([At, s[:, None], torch.zeros((theta.shape[0], 3), dtype=theta.dtype, device=theta.device)], dim=1)


def rotation_vectors(R):
    """The rotation vectors [S,3] of rotation matrices [S,3,3] (float64 on the host; angles up to pi)."""
    R = R.detach().double().cpu()
    v = 0.5 * torch.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], dim=1)
    sn, cs = v.norm(dim=1), ((R.diagonal(dim1=1, dim2=2).sum(dim=1) - 1) / 2).clamp(-1, 1)
    ang = torch.atan2(sn, cs)
    w = v * torch.where(sn > 1e-12, ang / sn.clamp_min(1e-300), torch.ones_like(sn))[:, None]
    for i in (cs < -0.999).nonzero().flatten().tolist():      # near pi the antisymmetric part vanishes: the axis from (R + I) / 2
        B = 0.5 * (R[i] + torch.eye(3, dtype=torch.float64))
        j = int(B.diagonal().argmax())
        axis = B[:, j] / B[j, j].sqrt()
        if float((axis * v[i]).sum()) < 0:
            axis = -axis
        w[i] = axis * ang[i]
    return w


class Poses(object):
    """Similarity poses of S shapes: matrix [S,3,4] = A|t with A = s R maps observed q to canonical x = A q + t, scale [S] = s (the
    targets of the fit were scaled by it).  theta [S,7] (rotation vector, translation, log s) when the poses come from a fit."""

    def __init__(self, matrix, scale, theta=None):
        self.matrix, self.scale, self.theta = matrix, scale, theta

    @classmethod
    def from_theta(cls, theta):
        rows = pose_rows(theta.detach())
        return cls(rows[:, :12].reshape(-1, 3, 4).contiguous(), rows[:, 12].contiguous(), theta.detach())

    def __len__(self):
        return self.matrix.shape[0]

    def to_canonical(self, points, s):
        """x = A_s q + t_s for points [..., 3] of shape s (s may be an index tensor [...] with one shape per point)."""
        M = self.matrix[s].to(points.device)
        return (points.unsqueeze(-2) * M[..., :, :3]).sum(dim=-1) + M[..., :, 3]

    def to_observed(self, points, s):
        """q = A_s^-1 (x - t_s), with A^-1 = A^T / s^2 (A is a scaled rotation)."""
        M, sc = self.matrix[s].to(points.device), self.scale[s].to(points.device)
        d = points - M[..., :, 3]
        return (d.unsqueeze(-1) * M[..., :, :3]).sum(dim=-2) / (sc * sc)[..., None]

    def rotate_to_observed(self, normals, s):
        """Directions of the canonical frame in the observed one: R_s^T n."""
        M, sc = self.matrix[s].to(normals.device), self.scale[s].to(normals.device)
        return (normals.unsqueeze(-1) * M[..., :, :3]).sum(dim=-2) / sc[..., None]

    def save(self, path):
        torch.save({"matrix": self.matrix.cpu(), "scale": self.scale.cpu()}, path)

    @classmethod
    def load(cls, path, device="cpu"):
        d = torch.load(path, map_location="cpu")
        return cls(d["matrix"].to(device), d["scale"].to(device))


def _initial_theta(S, K, pose_init, up, dev):
    """theta [K * S, 7]: start k of shape s (row k * S + s) is pose_init (None: the identity) after a yaw of 2 pi k / K about `up`."""
    axis = torch.tensor([float(c) for c in up], dtype=torch.float64)
    if axis.numel() != 3 or not float(axis.norm()) > 0:
        raise ValueError("up must be a non-zero direction (x, y, z), got %r" % (up,))
    axis = axis / axis.norm()
    yaw = torch.stack([axis * (2 * 3.141592653589793 * k / K) for k in range(K)])      # [K, 3]
    theta = torch.zeros((K, S, 7), dtype=torch.float64)
    if pose_init is None:
        theta[:, :, 0:3] = yaw[:, None, :]
    else:
        if len(pose_init) != S:
            raise ValueError("pose_init holds %d poses for %d shapes" % (len(pose_init), S))
        M, sc = pose_init.matrix.detach().double().cpu(), pose_init.scale.detach().double().cpu()
        R0 = M[:, :, :3] / sc[:, None, None]
        for k in range(K):
            theta[k, :, 0:3] = rotation_vectors(R0 @ rotation_matrices(yaw[k:k + 1]).expand(S, 3, 3))
        theta[:, :, 3:6] = M[None, :, :, 3]
        theta[:, :, 6] = sc.log()[None, :]
    return theta.reshape(K * S, 7).float().to(dev)


def fit_codes_and_poses(sdf_net, points, sdf, segment_offsets=None, points_per_shape=None, iterations=800, lr=5e-3, sigma=0.01, cutoff=0.1,
                        init=None, points_per_step=None, shuffle=True, seed=0, pose="similarity", pose_lr=1e-3, pose_init=None,
                        rotation_starts=1, up=(0, 1, 0)):
    """fit_latent_codes for clouds that are NOT in the network's frame: minimises over the code z and a pose per shape
        mean_p |SDFNet(s R q_p + t, z) - clamp(s sdf_p, +-cutoff)| + sigma * mean_k z_k^2
    and returns (codes [S,L], poses, loss [S]) — `poses` a Poses (matrix [S,3,4], scale [S], to_canonical / to_observed, save / load),
    loss the data term at the result.  The arguments of fit_latent_codes mean what they mean there.

    pose: "translation", "translation+scale", "rigid" or "similarity" — which of the rotation vector, the translation and log s are
    free; the others stay at their initial values (pose_init: a Poses, None: the identity).  Adam on the codes with `lr`, Adam on the
    pose parameters with `pose_lr`, both through sg_adam_step; the step itself is one fused launch (csrc/latent_fit.hip), the map
    from the parameters to the kernel's pose rows and its backward are small batched torch.
    rotation_starts = K > 1: a fit from a wrong basin does not turn a chair around, so every shape is fitted from K yaw angles
    2 pi k / K about `up` (after pose_init) and the start with the smallest final data term is kept.  The K fits run as K * S shapes of
    one call: points and targets are repeated K times on the device (16 K bytes per point) and so are codes and Adam moments."""
    if pose not in POSE_MODELS:
        raise ValueError("pose must be one of %s, got %r" % (sorted(POSE_MODELS), pose))
    K = int(rotation_starts)
    if K < 1 or K != rotation_starts:
        raise ValueError("rotation_starts must be an integer >= 1, got %r" % (rotation_starts,))
    points, sdf, seg = _segments(points, sdf, segment_offsets, points_per_shape)
    points, sdf = L.f32c(points.detach()), L.f32c(sdf.detach())
    S, Lz, dev = seg.numel() - 1, sdf_net.latent_code_size, points.device
    z = torch.zeros((S, Lz), dtype=torch.float32, device=dev) if init is None else L.f32c(init.detach().to(dev)).clone()
    off = ops.check_segments(points, sdf, z, seg)
    theta = _initial_theta(S, K, pose_init, up, dev)
    lo, hi = int(off[0]), int(off[-1])
    if shuffle and points_per_step:
        # one permutation per shape, as fit_latent_codes draws it
        g = torch.Generator(device=dev).manual_seed(int(seed))
        sid = torch.repeat_interleave(torch.arange(S, device=dev), (seg[1:] - seg[:-1]))
        order = torch.argsort(sid.double() + torch.rand(hi - lo, generator=g, device=dev, dtype=torch.float64) * 0.5) + lo
        points, sdf = points.clone(), sdf.clone()
        points[lo:hi], sdf[lo:hi] = points[order], sdf[order]
    if K > 1:
        points, sdf = points[lo:hi].repeat(K, 1), sdf[lo:hi].repeat(K)
        seg = torch.cat([seg[:1] - lo] + [seg[1:] - lo + k * (hi - lo) for k in range(K)])
        z = z.repeat(K, 1)
        off = seg.cpu().numpy()
    free = POSE_MODELS[pose]
    mask = torch.tensor([float(free[0])] * 3 + [float(free[1])] * 3 + [float(free[2])], dtype=torch.float32, device=dev)
    count = int(points_per_step) if points_per_step else 0
    fit = ops.LatentPoseFit(sdf_net._pack_shapes, sdf_net._params(), points, sdf, seg, off, cutoff)

    def step(start, cnt, sg):
        th = theta.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            rows = pose_rows(th)
        loss, gz, grows = fit.step(z, rows.detach(), start, cnt, sg)
        gth, = torch.autograd.grad(rows, th, grows)
        return loss, gz, L.f32c(gth * mask)
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    mt, vt = torch.zeros_like(theta), torch.zeros_like(theta)
    lib = ops._lib()
    for k in range(int(iterations)):
        _, gz, gth = step(k * count, count, sigma)
        ops.check(lib.sg_adam_step(ops.ptr(z), ops.ptr(gz), ops.ptr(m), ops.ptr(v), z.numel(), float(lr), 0.9, 0.999, 1e-8, k + 1, 1.0,
                                   ops.stream()), "adam_step")
        ops.check(lib.sg_adam_step(ops.ptr(theta), ops.ptr(gth), ops.ptr(mt), ops.ptr(vt), theta.numel(), float(pose_lr), 0.9, 0.999,
                                   1e-8, k + 1, 1.0, ops.stream()), "adam_step")
    loss, _, _ = step(0, 0, 0.0)
    if K > 1:
        best = loss.reshape(K, S).argmin(dim=0)
        row = best * S + torch.arange(S, device=dev)
        z, theta, loss = z[row].contiguous(), theta[row].contiguous(), loss[row].contiguous()
    return z, Poses.from_theta(theta), loss


def reconstruct_meshes(sdf_net, latent_codes, voxel_resolution=64, level=0, narrow_band=False, refine=0, clean=False, simplify=None,
                       poses=None):
    """MeshBatch of the level sets of the codes [S,L]: shape s is SDFNet.get_mesh(latent_codes[s], voxel_resolution, level=level), all
    grids and the marching cubes in batched launches.  narrow_band: the grids come from the brick path of SDFNet.voxel_grids, built for
    `level` (True, or a dict of its arguments brick / band / lipschitz).  refine = K > 0: the vertices are moved onto the network's level
    set by K Newton steps and carry its normals (surface.refine_meshes with the cell diagonal as the limit), as get_mesh(refine=K).
    clean: a rule of topology.clean_meshes ("largest", True, a dict), applied after marching cubes and before refine.  simplify: an int
    (the most triangles per shape) or a dict of the arguments of simplify.simplify_meshes, applied last; None: nothing.
    poses: the Poses of fit_codes_and_poses — after all of the above the vertices are mapped back to the observed frame
    (Poses.to_observed) and the unit normals rotated with them; None: the meshes stay in the network's frame."""
    codes = latent_codes.detach().reshape(-1, sdf_net.latent_code_size)
    if poses is not None and len(poses) != codes.shape[0]:
        raise ValueError("%d poses for %d codes" % (len(poses), codes.shape[0]))
    grids = sdf_net.voxel_grids(codes, voxel_resolution, sphere_only=True, level=level, **narrow_band_options(narrow_band))
    batch = marching_cubes(grids, level=level, spacing=2 / voxel_resolution, origin=-1, pad=True, pad_value=1.0)
    if clean:
        batch = batch.clean(clean)
    if refine:
        from .surface import cell_diagonal, refine_meshes
        batch, _ = refine_meshes(sdf_net, codes, batch, level=level, iterations=int(refine), max_move=cell_diagonal(voxel_resolution))
    if simplify is not None and simplify is not False:
        from .simplify import apply_option
        batch = apply_option(batch, simplify)
    if poses is not None:
        from .mesh import MeshBatch
        counts = batch.vert_offsets[1:] - batch.vert_offsets[:-1]
        sid = torch.repeat_interleave(torch.arange(len(batch), device=counts.device), counts).to(poses.matrix.device)
        batch = MeshBatch(poses.to_observed(batch.vertices, sid).contiguous(), poses.rotate_to_observed(batch.normals, sid).contiguous(),
                          batch.faces, batch.vert_offsets, batch.tri_offsets)
    return batch


def write_obj(path, mesh):
    with open(path, "w") as fh:
        for x, y, zc in mesh.vertices:
            fh.write("v %.7g %.7g %.7g\n" % (x, y, zc))
        for a, b, c in mesh.faces:
            fh.write("f %d %d %d\n" % (a + 1, b + 1, c + 1))


def main(argv=None):
    from . import evaluation, prepare
    from .model.sdf_net import SDFNet
    ap = argparse.ArgumentParser(description="Fit SDFNet latent codes to the meshes of a directory.")
    ap.add_argument("--net", required=True, help="state_dict of a trained SDFNet (models/sdf_net.to)")
    ap.add_argument("--models", default=None, help="directory searched for .obj files")
    ap.add_argument("--clouds", default=None, help="directory searched for point clouds (.npy [P,3] or [P,6], .xyz, .ply) instead of --models")
    ap.add_argument("--partial", type=int, default=None, metavar="V",
                    help="with --models: fit to the cloud that the first V scans see instead of the mesh (shape completion); the cloud is a random "
                         "subset of at most --points of the texels those scans drew (seeded by --seed)")
    ap.add_argument("--sample-count", type=int, default=11, help="cloud fits: the nearest samples whose normals vote on the sign")
    ap.add_argument("--k-normals", type=int, default=16, help="cloud fits: the neighbours a normal is estimated from")
    ap.add_argument("--view", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"),
                    help="--clouds without normals: the scanner position the estimated normals face, in the coordinates of the cloud FILES (a sensor at "
                         "its own origin: 0 0 0); the normals are estimated before the clouds are centred and scaled to the unit sphere")
    ap.add_argument("--out", required=True, help="where the codes [S,L] are torch.save'd")
    ap.add_argument("--meshes", default=None, help="directory for one reconstructed .obj per model")
    ap.add_argument("--chamfer", action="store_true", help="print the Chamfer distance between input and reconstruction")
    ap.add_argument("--device", default="cuda" if torch.cuda.is_available() else "cpu")
    ap.add_argument("--points", type=int, default=30000, help="SDF samples per model")
    ap.add_argument("--points-per-step", type=int, default=0)
    ap.add_argument("--iterations", type=int, default=800)
    ap.add_argument("--lr", type=float, default=5e-3)
    ap.add_argument("--sigma", type=float, default=0.01)
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--narrow-band", action="store_true", help="evaluate the network only in bricks near the surface")
    ap.add_argument("--refine", type=int, default=0, help="Newton steps that move the mesh vertices onto the network's level set")
    ap.add_argument("--clean", nargs="?", const="default", default=None, choices=("default", "largest"),
                    help="drop floating pieces of the reconstructions: below 1 %% of the area (default) or all but the largest")
    ap.add_argument("--simplify", type=int, default=None, metavar="N",
                    help="simplify the reconstructions to at most N triangles each (after --clean and --refine)")
    ap.add_argument("--scan-count", type=int, default=50)
    ap.add_argument("--scan-resolution", type=int, default=1024)
    ap.add_argument("--chamfer-points", type=int, default=2048)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pose", default=None, choices=sorted(POSE_MODELS),
                    help="fit a pose per shape together with its code (fit_codes_and_poses): for clouds that are not centred, scaled or "
                         "upright as the network's shapes are; meshes and --chamfer are then in the frame the fit was given: the clouds as "
                         "--clouds / --partial centre and scale them, with --models the mesh scaled to the unit sphere, not the files' coordinates")
    ap.add_argument("--pose-starts", type=int, default=1, metavar="K", help="with --pose: fit from K yaw angles about +y and keep the best")
    ap.add_argument("--pose-lr", type=float, default=None, help="with --pose: Adam's learning rate for the pose parameters (default 1e-3)")
    ap.add_argument("--poses-out", default=None, metavar="FILE", help="with --pose: where the poses (matrix [S,3,4], scale [S]) are torch.save'd")
    args = ap.parse_args(argv)
    if args.pose is None and (args.poses_out is not None or args.pose_starts != 1 or args.pose_lr is not None):
        ap.error("--poses-out, --pose-starts and --pose-lr go with --pose")
    if args.pose_starts < 1:
        ap.error("--pose-starts needs K >= 1")
    if (args.models is None) == (args.clouds is None):
        ap.error("exactly one of --models and --clouds is required")
    if args.partial is not None and (args.models is None or args.partial < 1):
        ap.error("--partial V goes with --models and needs V >= 1")
    if args.clouds is not None and args.chamfer:
        ap.error("--chamfer scores against the mesh of --models")

    dev = torch.device(args.device)
    state = torch.load(args.net, map_location="cpu")
    net = SDFNet(latent_code_size=state["layers1.0.weight"].shape[1] - 3, device=args.device)
    net.load_state_dict(state)
    L.bump_param_epoch()
    g = torch.Generator().manual_seed(args.seed)
    if args.clouds is not None:
        from . import cloudsdf
        files = cloudsdf.get_cloud_files(args.clouds)
        if not files:
            raise SystemExit("no point clouds under %s" % args.clouds)
        meshes = None
        try:
            source = cloudsdf.CloudSDF.from_files(files, view=args.view, k_normals=args.k_normals, device=dev)
        except ValueError as e:
            raise SystemExit("%s: %s" % (args.clouds, e))
        points, sdf, ok = source.sample_sdf_near_surface(args.points, generator=g, sample_count=args.sample_count)
    else:
        files = prepare.get_model_files(args.models)
        if not files:
            raise SystemExit("no .obj files under %s" % args.models)
        meshes = []
        for path in files:
            v, f = prepare.load_obj(path)
            meshes.append((prepare.scale_to_unit_sphere(v), f))
        scans = prepare.SurfaceScans(meshes, 1.0, args.scan_count, args.scan_resolution, device=dev)
        if args.partial is not None:
            from . import cloudsdf
            source = cloudsdf.CloudSDF.from_scans(scans, keep=range(min(args.partial, args.scan_count)), k_normals=args.k_normals,
                                                  max_points=args.points, generator=g)
            points, sdf, ok = source.sample_sdf_near_surface(args.points, generator=g, sample_count=args.sample_count)
        else:
            points, sdf, ok = scans.sample_sdf_near_surface(args.points, generator=g)
    poses = None
    if args.pose is None:
        codes, loss = fit_latent_codes(net, points, sdf, iterations=args.iterations, lr=args.lr, sigma=args.sigma,
                                       points_per_step=args.points_per_step or None, seed=args.seed)
    else:
        codes, poses, loss = fit_codes_and_poses(net, points, sdf, iterations=args.iterations, lr=args.lr, sigma=args.sigma,
                                                 points_per_step=args.points_per_step or None, seed=args.seed, pose=args.pose,
                                                 pose_lr=1e-3 if args.pose_lr is None else args.pose_lr, rotation_starts=args.pose_starts)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    torch.save(codes.cpu(), args.out)
    if args.poses_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.poses_out)), exist_ok=True)
        poses.save(args.poses_out)
    batch = None
    if args.meshes or args.chamfer:
        from .topology import clean_option
        batch = reconstruct_meshes(net, codes, args.resolution, narrow_band=args.narrow_band, refine=args.refine,
                                   clean=clean_option(args.clean), simplify=args.simplify, poses=poses)
    if args.meshes:
        os.makedirs(args.meshes, exist_ok=True)
        for i, mesh in enumerate(batch.meshes()):
            write_obj(os.path.join(args.meshes, "%04d.obj" % i), mesh)
    chamfer = [None] * len(files)
    if args.chamfer:
        n = args.chamfer_points
        recon, empty = batch.sample_surface(n, generator=g, return_empty=True)
        from .mesh import Mesh
        truth = torch.stack([torch.from_numpy(Mesh(v, f).sample(n, generator=g)) for v, f in meshes]).to(dev)
        d = evaluation.chamfer_distance(truth, recon).cpu()
        chamfer = [None if int(empty[i]) else float(d[i]) for i in range(len(files))]
    for i, path in enumerate(files):
        line = "%s: loss %.6f%s" % (path, float(loss[i]), "" if bool(ok[i]) else " (bad %s: too little inside)" % ("mesh" if args.clouds is None and args.partial is None else "cloud"))
        if args.chamfer:
            line += ", chamfer %s" % ("n/a (empty reconstruction)" if chamfer[i] is None else "%.6f" % chamfer[i])
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
