"""Training data from meshes: SDF voxel grids, uniform / surface point sets and DeepSDF clouds (K16 of include/shapegan_hip.h).

    python -m shapegan_amd.prepare --models data/shapenet/03001627 --dataset chairs --uniform-and-surface --sdf-clouds

Reference: prepare_shapenet_dataset.py:69-131 and prepare_data.py, which sit on mesh_to_sdf, trimesh, pyrender and an OpenGL context.
Here the same files come from three native pieces: K14's rasteriser draws the depth maps of K orthographic scans, sg_meshsdf_distance
finds the exact distance from every query point to the triangles, sg_meshsdf_sign calls a point outside when a scan sees it
(mesh_to_sdf's "depth" method, the one USE_DEPTH_BUFFER = True selects).  Two deliberate differences from mesh_to_sdf: the
magnitude is the distance to the triangles, not to a scanned point cloud, and the scans are orthographic, not perspective.  mesh_to_sdf's other method, 'normal' (USE_DEPTH_BUFFER = False), needs no triangles:
shapegan_amd/cloudsdf.py has it for point clouds, and CloudSDF.from_scans for the scan points of a SurfaceScans.

GPU tensors run the HIP kernels, CPU tensors the twin.  Random numbers are drawn with a CPU `torch.Generator` and moved to the device:
one seed gives the same query points on either.  File layout, dtypes and the bad-mesh markers are the reference's, so
`datasets.VoxelDataset`, `PointDataset` and `load_sdf_clouds` read the result.
"""
import argparse
import ctypes
import math
import os
import queue
import threading

import numpy as np
import torch

from . import lib as L
from .lib import check, ptr, stream
from .rendering import raster

MAX_SCANS = L.abi.DEFINES["SG_MESHSDF_MAX_SCANS"]
CHUNK = L.abi.DEFINES["SG_MESHSDF_CHUNK"]      # triangle records per LDS stage of the distance kernel


class BadMeshException(Exception):
    """The mesh gives no usable SDF: a voxel grid with a jump, or (almost) nothing inside."""


# ---- meshes -------------------------------------------------------------------------------------------------------------------------
def load_obj(path):
    """Wavefront .obj -> (vertices [V, 3] float64, faces [F, 3] int64): `v` and `f` lines only; polygons are fanned into triangles
    from their first corner; `a`, `a/b`, `a//c` and `a/b/c` index forms; negative indices count back from the vertices read so far."""
    vertices, faces = [], []
    with open(path, "r", errors="replace") as fh:
        for line in fh:
            parts = line.split()
            if not parts:
                continue
            if parts[0] == "v":
                vertices.append([float(parts[1]), float(parts[2]), float(parts[3])])
            elif parts[0] == "f":
                corners = []
                for token in parts[1:]:
                    i = int(token.split("/")[0])
                    corners.append(i - 1 if i > 0 else len(vertices) + i)
                for k in range(1, len(corners) - 1):
                    faces.append([corners[0], corners[k], corners[k + 1]])
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("%s: a face names a vertex that does not exist" % path)
    return v, f


def _centred(vertices):
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    if not len(v):
        return v, v
    lo, hi = v.min(axis=0), v.max(axis=0)
    return v - (lo + hi) / 2, hi - lo


def scale_to_unit_cube(vertices):
    """Centre on the bounding box, then multiply by 2 / (largest extent): the mesh fills [-1, 1] along its longest axis."""
    v, extent = _centred(vertices)
    scale = float(extent.max()) if len(v) else 0.0
    return v * (2.0 / scale) if scale > 0 else v


def scale_to_unit_sphere(vertices):
    """Centre on the bounding box, then divide by the largest distance from the centre."""
    v, _ = _centred(vertices)
    norm = float(np.linalg.norm(v, axis=1).max()) if len(v) else 0.0
    return v / norm if norm > 0 else v


def scan_directions(count):
    """`count` directions on a Fibonacci sphere, float64 [count, 3] (the contract of include/shapegan_hip.h, K16)."""
    i = np.arange(count, dtype=np.float64)
    y = 1.0 - (2.0 * i + 1.0) / count
    r = np.sqrt(1.0 - y * y)
    phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([r * np.cos(phi), y, r * np.sin(phi)], axis=1)


def scan_frame(d):
    """(u, v) of a scan that looks along -d from far away: u = normalize(up x d), v = d x u."""
    up = np.array([1.0, 0.0, 0.0]) if abs(d[1]) > 0.9 else np.array([0.0, 1.0, 0.0])
    u = np.cross(up, d)
    u = u / np.linalg.norm(u)
    return u, np.cross(d, u)


def scan_view(d, bounding_radius):
    """The orthographic 4x4 view of direction d: rows u / rho, v / rho, -d / rho, (0, 0, 0, 1)."""
    u, v = scan_frame(d)
    vp = np.zeros((4, 4), dtype=np.float64)
    vp[0, :3], vp[1, :3], vp[2, :3] = u / bounding_radius, v / bounding_radius, -d / bounding_radius
    vp[3, 3] = 1.0
    return vp


# ---- the two entry points --------------------------------------------------------------------------------------------------------------
def mesh_distance(soup, points, want_tri=True, want_closest=True, split=0):
    """sg_meshsdf_distance on points [S, Q, 3]: (dist2 [S, Q], tri [S, Q] int32 or None, closest [S, Q, 3] or None, split used).
    split > 0 forces the triangle split of the HIP kernel (tests, tuning); the twin has none and reports 0."""
    S, T, dev = len(soup), soup.positions.shape[0], soup.device
    points = L.f32c(points)
    if points.dim() != 3 or points.shape[0] != S or points.shape[2] != 3 or points.device != dev:
        raise ValueError("mesh_distance: points must be [S = %d, Q, 3] on %s, got %s on %s" % (S, dev, tuple(points.shape), points.device))
    Q = points.shape[1]
    lib = L.load()
    nbytes = lib.sg_meshsdf_distance_workspace_bytes(S, T, Q)
    if nbytes == 0:
        raise ValueError("mesh_distance: sizes out of range (S = %d, T = %d, Q = %d)" % (S, T, Q))
    ws = L.workspace("meshsdf", nbytes, dev)
    dist2 = torch.empty((S, Q), dtype=torch.float32, device=dev)
    tri = torch.empty((S, Q), dtype=torch.int32, device=dev) if want_tri else None
    closest = torch.empty((S, Q, 3), dtype=torch.float32, device=dev) if want_closest else None
    chosen = ctypes.c_int(0)
    try:
        if dev.type == "cuda":
            rc = lib.sg_meshsdf_distance_impl(ptr(soup.positions) if T else None, ptr(soup.tri_offsets), S, T, ptr(points), Q, ptr(dist2),
                                              ptr(tri), ptr(closest), ptr(ws), ws.numel(), int(split), ctypes.addressof(chosen), stream())
        else:
            rc = lib.sg_meshsdf_distance(ptr(soup.positions) if T else None, ptr(soup.tri_offsets), S, T, ptr(points), Q, ptr(dist2),
                                         ptr(tri), ptr(closest), ptr(ws), ws.numel(), stream())
        check(rc, "meshsdf_distance")
    finally:
        L.reset_call_state()
    return dist2, tri, closest, chosen.value


def mesh_sign(points, depth, vps, bias, dist2=None, want_outside=True):
    """sg_meshsdf_sign on points [S, Q, 3] with depth [K, S, N, N] and vps [K, 4, 4] float64: (sdf [S, Q] or None, outside [S, Q] uint8
    or None); sdf is computed iff dist2 is given."""
    points = L.f32c(points)
    if points.dim() != 3 or points.shape[2] != 3:
        raise ValueError("mesh_sign: points must be [S, Q, 3], got %s" % (tuple(points.shape),))
    S, Q, dev = points.shape[0], points.shape[1], points.device
    if (depth.dim() != 4 or depth.shape[1] != S or depth.shape[2] != depth.shape[3] or depth.dtype != torch.float32 or depth.device != dev
            or not depth.is_contiguous()):
        raise ValueError("mesh_sign: depth must be contiguous float32 [K, S = %d, N, N] on %s, got %s %s on %s"
                         % (S, dev, depth.dtype, tuple(depth.shape), depth.device))
    K, N = depth.shape[0], depth.shape[-1]
    vps = np.asarray(vps, dtype=np.float64)
    if vps.shape != (K, 4, 4):
        raise ValueError("mesh_sign: vps must be [K = %d, 4, 4], got %s" % (K, vps.shape))
    if dist2 is not None and (dist2.shape != (S, Q) or dist2.dtype != torch.float32 or dist2.device != dev):
        raise ValueError("mesh_sign: dist2 must be float32 [S, Q] = [%d, %d] on %s" % (S, Q, dev))
    sdf = torch.empty((S, Q), dtype=torch.float32, device=dev) if dist2 is not None else None
    outside = torch.empty((S, Q), dtype=torch.uint8, device=dev) if want_outside else None
    lib = L.load()
    try:
        check(lib.sg_meshsdf_sign(ptr(points), S, Q, ptr(depth), raster._doubles(vps), K, N, float(bias), ptr(dist2), ptr(sdf),
                                  ptr(outside), stream()), "meshsdf_sign")
    finally:
        L.reset_call_state()
    return sdf, outside


def _unit_sphere_points(count, generator):
    """`count` points uniform in the unit ball, float32 on the CPU: rejection from the cube, in the generator's order."""
    kept, have = [], 0
    while have < count:
        p = torch.rand((2 * (count - have) + 64, 3), generator=generator) * 2.0 - 1.0
        p = p[p.norm(dim=1) < 1.0]
        kept.append(p)
        have += p.shape[0]
    return torch.cat(kept)[:count].contiguous()


# ---- scans ------------------------------------------------------------------------------------------------------------------------------
class SurfaceScans(object):
    """K orthographic depth scans of S meshes, and everything the reference asks of mesh_to_sdf's SurfacePointCloud.

    meshes: one (vertices, faces) pair — the single-mesh form: results carry no shape axis and a bad mesh raises BadMeshException —
    or a list of pairs — the batch form: results have a leading S axis and come with a per-shape `ok` mask (bool [S], on the CPU).
    The meshes must lie inside the ball of `bounding_radius` (sqrt 3 for the unit cube, 1 for the unit sphere)."""

    def __init__(self, meshes, bounding_radius, scan_count=50, scan_resolution=1024, device="cuda", bias=None):
        self.single = isinstance(meshes, tuple)
        meshes = [meshes] if self.single else list(meshes)
        if not meshes:
            raise ValueError("SurfaceScans: no mesh")
        if not 1 <= scan_count <= MAX_SCANS:
            raise ValueError("SurfaceScans: 1 <= scan_count <= %d" % MAX_SCANS)
        self.device = torch.device(device)
        self.radius, self.K, self.N = float(bounding_radius), int(scan_count), int(scan_resolution)
        self.bias = float(np.float32(2.0 / self.N)) if bias is None else float(bias)      # one texel in NDC units
        soups, counts = [], []
        for vertices, faces in meshes:
            v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
            f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
            soups.append(v[f].astype(np.float32).reshape(-1, 3, 3))
            counts.append(len(f))
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.soup = raster.Soup(torch.from_numpy(np.concatenate(soups)).to(self.device), None, torch.from_numpy(offsets).to(self.device))
        self.S = len(meshes)
        self.directions = scan_directions(self.K)
        self.vps = np.stack([scan_view(d, self.radius) for d in self.directions])
        self.depth = torch.empty((self.K, self.S, self.N, self.N), dtype=torch.float32, device=self.device)
        for k in range(self.K):
            self.depth[k].copy_(raster.draw_view(self.soup, self.vps[k], self.N, self.N, cull_back=False).depth)

    # ---- queries ----------------------------------------------------------------------------------------------------------------------
    def _points(self, points):
        p = torch.as_tensor(points)
        p = L.f32c(p.to(self.device))
        if self.single and p.dim() == 2:
            p = p.unsqueeze(0)
        if p.dim() != 3 or p.shape[0] != self.S or p.shape[2] != 3:
            raise ValueError("SurfaceScans: points must be [%s, 3]" % ("Q" if self.single else "S = %d, Q" % self.S))
        return p.contiguous()

    def _out(self, t):
        return t[0] if self.single else t

    def is_outside(self, points):
        """bool [S, Q]: at least one scan sees the point."""
        _, outside = mesh_sign(self._points(points), self.depth, self.vps, self.bias)
        return self._out(outside.bool())

    def get_sdf(self, points, return_closest=False):
        """sdf [S, Q]: the distance to the triangles, negative where no scan sees the point (and the closest points [S, Q, 3])."""
        p = self._points(points)
        dist2, _, closest, _ = mesh_distance(self.soup, p, want_tri=False, want_closest=return_closest)
        sdf, _ = mesh_sign(p, self.depth, self.vps, self.bias, dist2=dist2, want_outside=False)
        return (self._out(sdf), self._out(closest)) if return_closest else self._out(sdf)

    def get_voxels(self, resolution, check_result=False):
        """voxels [S, R, R, R]: voxels[s][i][j][k] = the SDF at (c_i, c_j, c_k), c = -1 + 2 i / (R - 1).  check_result: the single form
        raises BadMeshException for a grid that fails check_voxels, the batch form returns (voxels, ok)."""
        R = int(resolution)
        c = torch.linspace(-1.0, 1.0, R, dtype=torch.float64)
        grid = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), dim=-1).reshape(1, R ** 3, 3).float()
        points = grid.to(self.device).expand(self.S, R ** 3, 3).contiguous()
        dist2, _, _, _ = mesh_distance(self.soup, points, want_tri=False, want_closest=False)
        sdf, _ = mesh_sign(points, self.depth, self.vps, self.bias, dist2=dist2, want_outside=False)
        voxels = sdf.reshape(self.S, R, R, R)
        if not check_result:
            return self._out(voxels)
        ok = check_voxels(voxels)
        if self.single:
            if not bool(ok[0]):
                raise BadMeshException()
            return voxels[0]
        return voxels, ok

    # ---- the scanned surface ------------------------------------------------------------------------------------------------------------
    def _covered(self, s):
        """The flat indices into [K, N, N] of the texels of shape s that a scan drew, increasing."""
        return (self.depth[:, s] < 1.0).reshape(-1).nonzero().reshape(-1)

    def _unproject(self, s, flat):
        """World points [M, 3] float32 of the texels `flat` of shape s: p = rho (c0 u + c1 v - t d) at the texel centres, in float64."""
        N = self.N
        k, iy, ix = flat // (N * N), (flat // N) % N, flat % N
        t = self.depth[:, s].reshape(-1)[flat].double()
        c0 = (ix.double() + 0.5) * (2.0 / N) - 1.0
        c1 = 1.0 - (iy.double() + 0.5) * (2.0 / N)
        frames = np.stack([np.concatenate(scan_frame(d) + (d,)) for d in self.directions])      # [K, 9]: u, v, d
        fr = torch.from_numpy(frames).to(self.device)[k]
        p = c0[:, None] * fr[:, 0:3] + c1[:, None] * fr[:, 3:6] - t[:, None] * fr[:, 6:9]
        return (p * self.radius).float()

    def scan_points(self):
        """The covered texels of every scan as world points: [M, 3] (single) or a list of S such tensors."""
        out = [self._unproject(s, self._covered(s)) for s in range(self.S)]
        return out[0] if self.single else out

    def _random_scan_points(self, count, generator):
        """[S, count, 3] random scan points (zeros for a shape no scan drew) and has [S] bool (CPU)."""
        out = torch.zeros((self.S, count, 3), dtype=torch.float32, device=self.device)
        has = torch.zeros(self.S, dtype=torch.bool)
        for s in range(self.S):
            covered = self._covered(s)
            r = torch.rand(count, generator=generator, dtype=torch.float64)
            if covered.numel():
                pick = (r * covered.numel()).long().clamp_(max=covered.numel() - 1).to(self.device)
                out[s] = self._unproject(s, covered[pick])
                has[s] = True
        return out, has

    def _finish(self, results, ok):
        if self.single:
            if not bool(ok[0]):
                raise BadMeshException()
            return tuple(r[0] for r in results)
        return tuple(results) + (ok,)

    def sample_sdf_near_surface(self, number_of_points=200000, min_size=0.015, generator=None):
        """DeepSDF's sampling: n_s = int(n 47 / 50) // 2 random scan points plus N(0, 0.0025^2) noise, the same points plus
        N(0, 0.00025^2) noise, the rest uniform in the unit sphere; (points [S, n, 3], sdf [S, n]).  The mesh is bad when fewer than
        min_size of the uniform part is inside."""
        g = generator if generator is not None else torch.Generator().manual_seed(torch.initial_seed())
        n = int(number_of_points)
        ns = int(n * 47 / 50) // 2
        nu = n - 2 * ns
        surface, has = self._random_scan_points(ns, g)
        coarse = torch.randn((self.S, ns, 3), generator=g) * 0.0025
        fine = torch.randn((self.S, ns, 3), generator=g) * 0.00025
        uniform = _unit_sphere_points(self.S * nu, g).reshape(self.S, nu, 3)
        points = torch.cat([surface + coarse.to(self.device), surface + fine.to(self.device), uniform.to(self.device)], dim=1).contiguous()
        dist2, _, _, _ = mesh_distance(self.soup, points, want_tri=False, want_closest=False)
        sdf, _ = mesh_sign(points, self.depth, self.vps, self.bias, dist2=dist2, want_outside=False)
        inside = (sdf[:, n - nu:] < 0).sum(dim=1).cpu().double() / max(nu, 1)
        return self._finish((points, sdf), has & (inside >= min_size))

    def get_uniform_and_surface_points(self, number_of_points=64 ** 3, generator=None):
        """prepare_shapenet_dataset.py:69-86: uniform points in the unit sphere with their SDF, and their closest surface points plus
        N(0, 0.0025^2) noise with theirs; (uniform [S, n, 3], uniform_sdf [S, n], surface [S, n, 3], surface_sdf [S, n]).  The mesh is
        bad when less than 0.01 of the uniform points is inside."""
        g = generator if generator is not None else torch.Generator().manual_seed(torch.initial_seed())
        n = int(number_of_points)
        uniform = _unit_sphere_points(self.S * n, g).reshape(self.S, n, 3).to(self.device)
        noise = (torch.randn((self.S, n, 3), generator=g) * 0.0025).to(self.device)
        dist2, _, closest, _ = mesh_distance(self.soup, uniform, want_tri=False, want_closest=True)
        uniform_sdf, _ = mesh_sign(uniform, self.depth, self.vps, self.bias, dist2=dist2, want_outside=False)
        surface = (closest + noise).contiguous()
        near2, _, _, _ = mesh_distance(self.soup, surface, want_tri=False, want_closest=False)
        surface_sdf, _ = mesh_sign(surface, self.depth, self.vps, self.bias, dist2=near2, want_outside=False)
        inside = (uniform_sdf < 0).sum(dim=1).cpu().double() / n
        has_triangles = (self.soup.tri_offsets[1:] > self.soup.tri_offsets[:-1]).cpu()
        return self._finish((uniform, uniform_sdf, surface, surface_sdf), has_triangles & (inside >= 0.01))


def check_voxels(voxels):
    """mesh_to_sdf's test of a grid [S, R, R, R] (or [R, R, R]): good when the largest difference between neighbours along any axis is
    below 2 / R * sqrt(3) * 1.1.  Returns bool [S] on the CPU (a Python bool for one grid)."""
    v = torch.as_tensor(voxels)
    one = v.dim() == 3
    v = v.unsqueeze(0) if one else v
    R = v.shape[-1]
    worst = torch.zeros(v.shape[0], dtype=v.dtype, device=v.device)
    for axis in (1, 2, 3):
        d = (v.narrow(axis, 1, R - 1) - v.narrow(axis, 0, R - 1)).abs().reshape(v.shape[0], -1)
        if d.shape[1]:
            worst = torch.maximum(worst, d.max(dim=1).values)
    ok = (worst < 2.0 / R * 3 ** 0.5 * 1.1).cpu()      # NaN compares false: a grid with a NaN is bad
    return bool(ok[0]) if one else ok


# ---- the command line: prepare_shapenet_dataset.py ------------------------------------------------------------------------------------
def get_hash(filename):
    """ShapeNet's <hash>/models/model_normalized.obj: the third-last path component."""
    return filename.replace(os.sep, "/").split("/")[-3]


def get_model_files(directory, extension=".obj"):
    found = []
    for root, _, files in os.walk(directory):
        found.extend(os.path.join(root, name) for name in files if name.endswith(extension))
    return sorted(found)


class Layout(object):
    """The reference's directory layout under `data/<dataset>/`."""

    def __init__(self, data, dataset):
        self.data, self.root = data, os.path.join(data, dataset)

    def voxels(self, name, resolution):
        return os.path.join(self.root, "voxels_%d" % resolution, get_hash(name) + ".npy")

    def uniform(self, name):
        return os.path.join(self.root, "uniform", get_hash(name) + ".npy")

    def surface(self, name):
        return os.path.join(self.root, "surface", get_hash(name) + ".npy")

    def cloud(self, name):
        return os.path.join(self.root, "cloud", get_hash(name) + ".npy")

    def bad(self, name):
        return os.path.join(self.root, "bad_meshes", get_hash(name))

    def mark_bad(self, name):
        os.makedirs(os.path.dirname(self.bad(name)), exist_ok=True)
        open(self.bad(name), "w").close()


def _save(path, array):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.save(path, array)


def _read_ahead(items, load):
    """load(item) for every item on ONE reader thread, one item ahead of the consumer (as datasets.VoxelStream reads)."""
    slots = queue.Queue(maxsize=1)

    def run():
        for item in items:
            try:
                slots.put((item, load(item), None))
            except Exception as e:      # handed to the consumer, which decides
                slots.put((item, None, e))
        slots.put(None)

    reader = threading.Thread(target=run, daemon=True)
    reader.start()
    while True:
        got = slots.get()
        if got is None:
            break
        yield got
    reader.join()


def _rows(points, values):
    return np.concatenate([points.cpu().numpy(), values.cpu().numpy()[:, None]], axis=1).astype(np.float32)


def process_models(models, dataset, data="data", resolutions=(8, 16, 32, 64), uniform_and_surface=False, sdf_clouds=False, scan_count=50,
                   scan_resolution=1024, batch=1, device="cuda", cloud_size=200000, sample_size=64 ** 3, seed=0, log=print):
    """prepare_shapenet_dataset.py's process_model_files without worker processes: `batch` meshes per pass on the device, the .obj files
    parsed one batch ahead on a reader thread.  Writes only what is missing; returns the number of files written."""
    layout = Layout(data, dataset)
    generator = torch.Generator().manual_seed(seed)
    written = 0

    def todo(name):
        if os.path.exists(layout.bad(name)):
            return None
        need_voxels = [r for r in resolutions if not os.path.exists(layout.voxels(name, r))]
        need_points = uniform_and_surface and not (os.path.exists(layout.uniform(name)) and os.path.exists(layout.surface(name)))
        need_cloud = sdf_clouds and not os.path.exists(layout.cloud(name))
        return (need_voxels, need_points, need_cloud) if (need_voxels or need_points or need_cloud) else None

    names = [n for n in get_model_files(models) if todo(n) is not None]
    groups = [names[i:i + batch] for i in range(0, len(names), batch)]
    def load_group(group):
        """(mesh or the exception that reading it raised) per file: a broken file costs that one model, as in the reference."""
        loaded = []
        for n in group:
            try:
                loaded.append(load_obj(n))
            except Exception as e:
                loaded.append(e)
        return loaded

    for group, loaded, error in _read_ahead(groups, load_group):
        if error is not None:
            raise error
        for n, m in zip(group, loaded):
            if isinstance(m, Exception):
                log("Skipping %s: %s: %s" % (get_hash(n), type(m).__name__, m))
        group, meshes = [n for n, m in zip(group, loaded) if not isinstance(m, Exception)], [m for m in loaded if not isinstance(m, Exception)]
        alive = [(n, m) for n, m in zip(group, meshes) if len(m[1])]
        for n, m in zip(group, meshes):
            if not len(m[1]):
                log("Skipping bad mesh. (%s)" % get_hash(n))
                layout.mark_bad(n)
        # voxels: the unit cube inside the ball of radius sqrt 3
        wanted = [(n, m) for n, m in alive if todo(n)[0]]
        if wanted:
            scans = SurfaceScans([(scale_to_unit_cube(m[0]), m[1]) for _, m in wanted], 3 ** 0.5, scan_count, scan_resolution, device)
            good, grids = torch.ones(len(wanted), dtype=torch.bool), {}
            for r in resolutions:      # the reference recomputes every resolution of a mesh that lacks one
                grids[r], ok = scans.get_voxels(r, check_result=True)
                good &= ok
            for i, (n, _) in enumerate(wanted):
                if not bool(good[i]):
                    log("Skipping bad mesh. (%s)" % get_hash(n))
                    layout.mark_bad(n)
                    continue
                for r in resolutions:
                    _save(layout.voxels(n, r), grids[r][i].cpu().numpy())
                    written += 1
            del scans, grids
        # point sets: the unit sphere
        wanted = [(n, m) for n, m in alive if todo(n) is not None and (todo(n)[1] or todo(n)[2])]
        if wanted:
            scans = SurfaceScans([(scale_to_unit_sphere(m[0]), m[1]) for _, m in wanted], 1.0, scan_count, scan_resolution, device)
            good = torch.ones(len(wanted), dtype=torch.bool)
            points = cloud = None
            if any(todo(n)[1] for n, _ in wanted):
                points = scans.get_uniform_and_surface_points(sample_size, generator)
                good &= points[-1]
            if any(todo(n)[2] for n, _ in wanted):
                cloud = scans.sample_sdf_near_surface(cloud_size, 0.015, generator)
                good &= cloud[-1]
            for i, (n, _) in enumerate(wanted):
                if not bool(good[i]):
                    log("Skipping bad mesh. (%s)" % get_hash(n))
                    layout.mark_bad(n)
                    continue
                need = todo(n)
                if points is not None and need[1]:
                    _save(layout.uniform(n), _rows(points[0][i], points[1][i]))
                    _save(layout.surface(n), _rows(points[2][i], points[3][i]))
                    written += 2
                if cloud is not None and need[2]:
                    _save(layout.cloud(n), _rows(cloud[0][i], cloud[1][i]))
                    written += 1
            del scans
    return written


def combine_sdf_clouds(models, dataset, data="data"):
    """prepare_shapenet_dataset.py:167-188: every cloud of the set, in the sorted order of the model files, into data/sdf_points.to
    [M n, 3] and data/sdf_values.to [M n] (torch.save).  Returns the number of clouds."""
    layout = Layout(data, dataset)
    files = [layout.cloud(n) for n in get_model_files(models) if os.path.exists(layout.cloud(n))]
    clouds = [np.load(f) for f in files]
    points = torch.from_numpy(np.concatenate([c[:, :3] for c in clouds])) if clouds else torch.zeros((0, 3))
    values = torch.from_numpy(np.concatenate([c[:, 3] for c in clouds])) if clouds else torch.zeros(0)
    os.makedirs(data, exist_ok=True)
    torch.save(points.float().contiguous(), os.path.join(data, "sdf_points.to"))
    torch.save(values.float().contiguous(), os.path.join(data, "sdf_values.to"))
    return len(files)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m shapegan_amd.prepare", description=__doc__.split("\n")[0])
    ap.add_argument("--models", required=True, help="directory of .obj files in ShapeNet's layout (<hash>/models/<name>.obj)")
    ap.add_argument("--dataset", required=True, help="name of the set: files go to <data>/<dataset>/")
    ap.add_argument("--data", default="data")
    ap.add_argument("--resolutions", type=int, nargs="*", default=[8, 16, 32, 64])
    ap.add_argument("--uniform-and-surface", action="store_true")
    ap.add_argument("--sdf-clouds", action="store_true")
    ap.add_argument("--scan-count", type=int, default=50)
    ap.add_argument("--scan-resolution", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--device", default="cuda", choices=("cuda", "cpu"))
    ap.add_argument("--cloud-size", type=int, default=200000)
    ap.add_argument("--sample-size", type=int, default=64 ** 3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    written = process_models(a.models, a.dataset, a.data, tuple(a.resolutions), a.uniform_and_surface, a.sdf_clouds, a.scan_count,
                             a.scan_resolution, max(1, a.batch), a.device, a.cloud_size, a.sample_size, a.seed)
    print("%d files written" % written)
    if a.sdf_clouds:
        print("%d clouds combined" % combine_sdf_clouds(a.models, a.dataset, a.data))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
