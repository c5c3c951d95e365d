"""Signed distances from oriented point clouds: k nearest neighbours, normals and mesh_to_sdf's 'normal' sign (K19 of include/shapegan_hip.h).

    scans = prepare.SurfaceScans(mesh, 1.0)                 # or any cloud: a depth scan, a LiDAR sweep, load_cloud("scan.ply")
    cloud = CloudSDF.from_scans(scans, keep=range(5))       # a partial observation: 5 of the 50 views
    points, sdf = cloud.sample_sdf_near_surface(30000)      # what reconstruct.fit_latent_codes takes

Reference: mesh_to_sdf's SurfacePointCloud.get_sdf with use_depth_buffer = False (its default; demo_training.py:16, create_plot.py:636,
prepare_shapenet_dataset.py:33,129 with USE_DEPTH_BUFFER = False): the distance to the nearest sample of an oriented cloud, the sign
from a vote of the normals of the sample_count = 11 nearest samples.  prepare.SurfaceScans is the 'depth' method and needs triangles;
this module needs points only.  The search is a brute-force walk on the device (csrc/cloud.hip), the twin on CPU tensors; there is
no kd-tree and no eager-PyTorch path.

Clouds are dense [S, P, 3] tensors or ragged pairs (points [N, 3], offsets [S + 1] int64); neighbour indices are local to a shape's cloud.
"""
import os

import numpy as np
import torch

from . import lib as L
from .lib import check, ptr, stream

MAX_K = L.abi.DEFINES["SG_CLOUD_MAX_K"]
QUERY_TILE = L.abi.DEFINES["SG_CLOUD_QUERY_TILE"]
STAGE = L.abi.DEFINES["SG_CLOUD_STAGE"]


# ---- calling forms ----------------------------------------------------------------------------------------------------------------------
def _ragged(clouds, what, device=None):
    """(points [N, 3] fp32 contiguous, offsets [S + 1] int64 on the same device, dense shape (S, P) or None)."""
    if isinstance(clouds, (tuple, list)) and len(clouds) == 2 and torch.is_tensor(clouds[1]) and clouds[1].dim() == 1 \
            and not clouds[1].dtype.is_floating_point:
        points, offsets = clouds
        points = L.f32c(torch.as_tensor(points) if device is None else torch.as_tensor(points).to(device))
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("%s: ragged points must be [N, 3], got %s" % (what, tuple(points.shape)))
        offsets = offsets.to(device=points.device, dtype=torch.int64).contiguous()
        if offsets.numel() < 2:
            raise ValueError("%s: offsets must hold S + 1 >= 2 entries" % what)
        return points, offsets, None
    points = torch.as_tensor(clouds)
    points = L.f32c(points if device is None else points.to(device))
    if points.dim() != 3 or points.shape[2] != 3 or points.shape[0] < 1:
        raise ValueError("%s: expected [S, P, 3] or (points [N, 3], offsets [S + 1]), got %s" % (what, tuple(points.shape)))
    S, P = points.shape[0], points.shape[1]
    offsets = torch.arange(S + 1, dtype=torch.int64, device=points.device) * P
    return points.reshape(S * P, 3), offsets, (S, P)


def _check_k(k):
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("cloudsdf: 1 <= k <= %d, got %d" % (MAX_K, k))
    return k


def _p(t):
    return ptr(t) if t is not None and t.numel() else None


def _check_arrays(what, points, cloud_offsets, queries=None, query_offsets=None):
    """The raw wrappers pass pointers: anything but contiguous float32 [*, 3] and int64 [S + 1] on ONE device would be read as garbage."""
    dev = points.device
    for name, a in (("points", points), ("queries", queries)):
        if a is not None and (not torch.is_tensor(a) or a.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != 3 or not a.is_contiguous()
                              or a.device != dev):
            raise ValueError("%s: %s must be a contiguous float32 [*, 3] tensor on %s" % (what, name, dev))
    for name, o in (("cloud_offsets", cloud_offsets), ("query_offsets", query_offsets)):
        if o is not None and (not torch.is_tensor(o) or o.dtype != torch.int64 or o.dim() != 1 or o.numel() != cloud_offsets.numel()
                              or o.numel() < 2 or not o.is_contiguous() or o.device != dev):
            raise ValueError("%s: %s must be a contiguous int64 [S + 1] tensor on %s" % (what, name, dev))


# ---- the three entry points -----------------------------------------------------------------------------------------------------------------
def knn_ragged(points, cloud_offsets, queries, query_offsets, k, exclude_self=False):
    """sg_cloud_knn: (idx [M, k] int32, d2 [M, k] fp32)."""
    _check_arrays("knn_ragged", points, cloud_offsets, queries, query_offsets)
    k, S, N, M, dev = _check_k(k), cloud_offsets.numel() - 1, points.shape[0], queries.shape[0], points.device
    idx = torch.empty((M, k), dtype=torch.int32, device=dev)
    d2 = torch.empty((M, k), dtype=torch.float32, device=dev)
    lib = L.load()
    try:
        check(lib.sg_cloud_knn(_p(points), ptr(cloud_offsets), _p(queries), ptr(query_offsets), S, N, M, k, 1 if exclude_self else 0,
                               _p(idx), _p(d2), stream()), "cloud_knn")
    finally:
        L.reset_call_state()
    return idx, d2


def normals_ragged(points, cloud_offsets, idx, view=None, view_per_point=False):
    """sg_cloud_normals: (normals [N, 3], variation [N]) from the lists idx [N, k] of a self-query with exclude_self."""
    _check_arrays("normals_ragged", points, cloud_offsets)
    S, N, dev = cloud_offsets.numel() - 1, points.shape[0], points.device
    k = _check_k(idx.shape[1])
    if idx.shape[0] != N or idx.dtype != torch.int32 or idx.device != dev:
        raise ValueError("cloudsdf: idx must be int32 [N = %d, k] on %s" % (N, dev))
    if view is not None:
        view = L.f32c(view.to(dev))
        if tuple(view.shape) != ((N, 4) if view_per_point else (S, 4)):
            raise ValueError("cloudsdf: view must be [%d, 4], got %s" % (N if view_per_point else S, tuple(view.shape)))
    idx = idx.contiguous()      # a local name: the tensor behind a pointer must outlive the call
    normals = torch.empty((N, 3), dtype=torch.float32, device=dev)
    variation = torch.empty((N,), dtype=torch.float32, device=dev)
    lib = L.load()
    try:
        check(lib.sg_cloud_normals(_p(points), ptr(cloud_offsets), S, N, _p(idx), k, _p(view), 1 if view_per_point else 0,
                                   _p(normals), _p(variation), stream()), "cloud_normals")
    finally:
        L.reset_call_state()
    return normals, variation


def sdf_ragged(points, normals, cloud_offsets, queries, query_offsets, k=11, want_nearest=False):
    """sg_cloud_sdf: sdf [M] (and nearest [M] int32)."""
    _check_arrays("sdf_ragged", points, cloud_offsets, queries, query_offsets)
    k, S, N, M, dev = _check_k(k), cloud_offsets.numel() - 1, points.shape[0], queries.shape[0], points.device
    if tuple(normals.shape) != (N, 3) or normals.device != dev or not normals.dtype.is_floating_point:
        raise ValueError("cloudsdf: normals must be floating point [N = %d, 3] on %s" % (N, dev))
    normals = L.f32c(normals)      # a local name: the tensor behind a pointer must outlive the call
    sdf = torch.empty((M,), dtype=torch.float32, device=dev)
    nearest = torch.empty((M,), dtype=torch.int32, device=dev) if want_nearest else None
    lib = L.load()
    try:
        check(lib.sg_cloud_sdf(_p(points), _p(normals), ptr(cloud_offsets), _p(queries), ptr(query_offsets), S, N, M, k, _p(sdf),
                               _p(nearest), stream()), "cloud_sdf")
    finally:
        L.reset_call_state()
    return (sdf, nearest) if want_nearest else sdf


# ---- the public functions -----------------------------------------------------------------------------------------------------------------
def knn(clouds, queries=None, k=16):
    """The k nearest points of each shape's cloud for every query, in the order (squared distance, index): (idx, d2), [S, Q, k] for dense
    queries and [M, k] for ragged ones; slots beyond the cloud's size hold -1 / +inf.  queries None: every point against its own cloud,
    itself (by index) left out."""
    points, co, dense = _ragged(clouds, "knn")
    if queries is None:
        idx, d2 = knn_ragged(points, co, points, co, k, exclude_self=True)
    else:
        q, qo, dense = _ragged(queries, "knn", points.device)
        if qo.numel() != co.numel():
            raise ValueError("knn: %d clouds but %d query sets" % (co.numel() - 1, qo.numel() - 1))
        idx, d2 = knn_ragged(points, co, q, qo, k)
    if dense is not None:
        idx, d2 = idx.reshape(dense[0], dense[1], -1), d2.reshape(dense[0], dense[1], -1)
    return idx, d2


def _views(view, S, N, dense, dev):
    """(view [S, 4] or [N, 4] or None, per point?) from [3] / [4] (all shapes), [S, 3 | 4], or per point [N, 3 | 4] / [S, P, 3 | 4]; three
    components are a scanner POSITION (w = 1)."""
    if view is None:
        return None, False
    v = torch.as_tensor(view).to(device=dev, dtype=torch.float32)
    if v.shape[-1] == 3:
        v = torch.cat([v, torch.ones(v.shape[:-1] + (1,), dtype=torch.float32, device=dev)], dim=-1)
    if v.shape[-1] != 4:
        raise ValueError("cloudsdf: a view has 3 or 4 components")
    if v.dim() == 1:
        return v.expand(S, 4).contiguous(), False
    if v.dim() == 3 and dense is not None and tuple(v.shape[:2]) == dense:
        return v.reshape(N, 4).contiguous(), True
    if v.dim() == 2 and v.shape[0] == S and (dense is not None or v.shape[0] != N):
        return v.contiguous(), False
    if v.dim() == 2 and v.shape[0] == N:
        return v.contiguous(), True
    raise ValueError("cloudsdf: view must be [4], [S, 4] or one per point, got %s" % (tuple(v.shape),))


def estimate_normals(clouds, k=16, view=None, return_variation=False):
    """Unit normals by PCA of each point's k nearest neighbours, in the form of `clouds`.  view: a scanner position [3], (x, y, z, w)
    with w = 0 for the direction toward an orthographic scanner, per shape or per point: the normals face it.  view None: unoriented —
    the largest component is positive, which is no consistent orientation.  A point without a plane through its neighbourhood gets
    (0, 0, 0) and the variation -1."""
    points, co, dense = _ragged(clouds, "estimate_normals")
    S, N = co.numel() - 1, points.shape[0]
    idx, _ = knn_ragged(points, co, points, co, k, exclude_self=True)
    v, per_point = _views(view, S, N, dense, points.device)
    normals, variation = normals_ragged(points, co, idx, v, per_point)
    if dense is not None:
        normals, variation = normals.reshape(dense[0], dense[1], 3), variation.reshape(dense)
    return (normals, variation) if return_variation else normals


class CloudSDF(object):
    """The point-cloud counterpart of prepare.SurfaceScans: the SDF of oriented clouds at arbitrary points.

    points [P, 3] (and normals [P, 3]) — the single form: results carry no shape axis and a bad cloud raises BadMeshException — or a
    batch: [S, P, 3], a list of [P_i, 3] arrays, or flat [N, 3] with offsets [S + 1]; results have a leading S axis and come with a per-shape
    `ok` mask.  Without normals they are estimated from k_normals neighbours and oriented by `view` (estimate_normals)."""

    def __init__(self, points, normals=None, offsets=None, view=None, k_normals=16, device=None, _view_per_point=False):
        as_list = isinstance(points, (list, tuple)) and not torch.is_tensor(points)
        if as_list:
            if not len(points):
                raise ValueError("CloudSDF: no cloud")
            parts = [torch.as_tensor(np.asarray(p) if not torch.is_tensor(p) else p).reshape(-1, 3) for p in points]
            if device is None:      # the device of the first cloud that is on one
                device = next((p.device for p in parts if p.is_cuda), parts[0].device)
            parts = [p.to(device=device, dtype=torch.float32) for p in parts]
            if normals is not None and not torch.is_tensor(normals):      # one array per cloud (a tensor: already flat, [N, 3])
                normals = torch.cat([torch.as_tensor(np.asarray(n) if not torch.is_tensor(n) else n).reshape(-1, 3).to(device=device, dtype=torch.float32)
                                     for n in normals])
            offsets = torch.tensor([0] + [p.shape[0] for p in parts], dtype=torch.int64).cumsum(0)
            points = torch.cat(parts)
        points = torch.as_tensor(points)
        self.device = torch.device(device) if device is not None else points.device
        self.single = points.dim() == 2 and offsets is None
        if self.single:
            points, offsets = points.reshape(-1, 3), torch.tensor([0, points.shape[0]], dtype=torch.int64)
        if offsets is not None:
            self.points, self.offsets, dense = _ragged((points, torch.as_tensor(offsets)), "CloudSDF", self.device)
        else:
            self.points, self.offsets, dense = _ragged(points, "CloudSDF", self.device)
        self.S, self.N = self.offsets.numel() - 1, self.points.shape[0]
        self.sizes = (self.offsets[1:] - self.offsets[:-1]).cpu()
        if normals is None:
            # from_scans names the per-point form outright: a batch with as many points as shapes must not be read as per-shape views
            v, per_point = (view, True) if _view_per_point else _views(view, self.S, self.N, dense, self.device)
            idx, _ = knn_ragged(self.points, self.offsets, self.points, self.offsets, k_normals, exclude_self=True)
            self.normals, self.variation = normals_ragged(self.points, self.offsets, idx, v, per_point)
        else:
            self.normals = L.f32c(torch.as_tensor(normals).to(self.device)).reshape(-1, 3)
            self.variation = None
            if self.normals.shape[0] != self.N:
                raise ValueError("CloudSDF: %d normals for %d points" % (self.normals.shape[0], self.N))

    @classmethod
    def from_scans(cls, scans, keep=None, k_normals=16, max_points=None, generator=None):
        """The cloud of the texels that the scans of a prepare.SurfaceScans drew.  keep: the views that count (indices into its K
        directions) — a partial observation; None: all.  Normals are estimated and face the scan that saw the point: the per-point view
        is (d_k, 0).  max_points: at most so many points per shape, a random subset drawn with `generator` (in texel order): 50 scans at
        1024 x 1024 are millions of points, and the search is brute force."""
        kept = None if keep is None else torch.tensor(sorted(set(int(k) for k in keep)), dtype=torch.int64, device=scans.device)
        if kept is not None and kept.numel() and (int(kept[0]) < 0 or int(kept[-1]) >= scans.K):
            raise ValueError("CloudSDF.from_scans: keep names a view outside [0, %d)" % scans.K)
        directions = torch.from_numpy(scans.directions).to(device=scans.device, dtype=torch.float32)
        g = generator if generator is not None else torch.Generator().manual_seed(torch.initial_seed())
        parts, views = [], []
        for s in range(scans.S):
            flat = scans._covered(s)
            view_of = flat // (scans.N * scans.N)
            if kept is not None:
                chosen = torch.isin(view_of, kept)
                flat, view_of = flat[chosen], view_of[chosen]
            if max_points is not None and flat.numel() > int(max_points):
                pick = torch.randperm(flat.numel(), generator=g)[:int(max_points)].sort().values.to(scans.device)
                flat, view_of = flat[pick], view_of[pick]
            parts.append(scans._unproject(s, flat))
            views.append(torch.cat([directions[view_of], torch.zeros((flat.numel(), 1), dtype=torch.float32, device=scans.device)], dim=1))
        offsets = torch.tensor([0] + [p.shape[0] for p in parts], dtype=torch.int64).cumsum(0)
        out = cls(torch.cat(parts), offsets=offsets, view=torch.cat(views), k_normals=k_normals, device=scans.device, _view_per_point=True)
        out.single = scans.single
        return out

    @classmethod
    def from_files(cls, paths, view=None, k_normals=16, device=None):
        """The clouds of the files `paths` (load_cloud), each centred and scaled to the unit sphere as prepare.scale_to_unit_sphere does
        for a mesh — a batch, whatever the number of files.  Normals come from the files, or (when none of them has any) are estimated
        ON THE FILE'S OWN COORDINATES, before the rescaling: `view` is a scanner position (or (x, y, z, 0), a direction) in the frame
        the file was written in — a sensor at its own origin is view=(0, 0, 0) — and a normal does not change under the translation
        and the uniform scale that follow."""
        from .prepare import scale_to_unit_sphere
        loaded = [load_cloud(path) for path in paths]
        if not loaded:
            raise ValueError("CloudSDF.from_files: no file")
        oriented = [n is not None for _, n in loaded]
        if any(oriented) and not all(oriented):
            raise ValueError("CloudSDF.from_files: some clouds carry normals and some do not")
        raw = cls([torch.from_numpy(p) for p, _ in loaded], normals=[torch.from_numpy(n) for _, n in loaded] if all(oriented) else None,
                  view=view, k_normals=k_normals, device=device)
        scaled = [torch.from_numpy(scale_to_unit_sphere(p).astype(np.float32)) for p, _ in loaded]
        out = cls(scaled, normals=raw.normals, device=raw.device)
        out.variation = raw.variation
        return out

    # ---- queries --------------------------------------------------------------------------------------------------------------------------
    def _queries(self, query):
        q = L.f32c(torch.as_tensor(query).to(self.device))
        if self.single and q.dim() == 2:
            q = q.unsqueeze(0)
        if q.dim() != 3 or q.shape[0] != self.S or q.shape[2] != 3:
            raise ValueError("CloudSDF: points must be [%s, 3]" % ("Q" if self.single else "S = %d, Q" % self.S))
        return q.contiguous()

    def _out(self, t):
        return t[0] if self.single else t

    def _sdf(self, q, sample_count):
        S, Q = q.shape[0], q.shape[1]
        qo = torch.arange(S + 1, dtype=torch.int64, device=self.device) * Q
        return sdf_ragged(self.points, self.normals, self.offsets, q.reshape(S * Q, 3), qo, sample_count).reshape(S, Q)

    def get_sdf(self, query, sample_count=11):
        """sdf [S, Q]: the distance to the nearest point of the cloud, negative where more than half of the sample_count nearest points
        have the query behind their normal.  +inf for an empty cloud."""
        return self._out(self._sdf(self._queries(query), sample_count))

    def get_voxels(self, resolution, sample_count=11, check_result=False):
        """voxels [S, R, R, R] on the grid of SurfaceScans.get_voxels: voxels[s][i][j][k] = the SDF at (c_i, c_j, c_k), c = -1 + 2 i / (R - 1)."""
        from .prepare import BadMeshException, check_voxels
        R = int(resolution)
        c = torch.linspace(-1.0, 1.0, R, dtype=torch.float64)
        grid = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), dim=-1).reshape(1, R ** 3, 3).float()
        voxels = self._sdf(grid.to(self.device).expand(self.S, R ** 3, 3).contiguous(), sample_count).reshape(self.S, R, R, R)
        if not check_result:
            return self._out(voxels)
        ok = check_voxels(voxels)
        if self.single:
            if not bool(ok[0]):
                raise BadMeshException()
            return voxels[0]
        return voxels, ok

    def sample_sdf_near_surface(self, number_of_points=200000, min_size=0.015, generator=None, sample_count=11):
        """DeepSDF's mixture exactly as SurfaceScans.sample_sdf_near_surface draws it — n_s = int(n 47 / 50) // 2 random surface points plus
        N(0, 0.0025^2) noise, the same points plus N(0, 0.00025^2) noise, the rest uniform in the unit sphere — with the surface points
        drawn from the cloud's own points; (points [S, n, 3], sdf [S, n]) and, for a batch, ok [S].  A cloud is bad when it is empty or
        fewer than min_size of the uniform part is inside."""
        from .prepare import BadMeshException, _unit_sphere_points
        g = generator if generator is not None else torch.Generator().manual_seed(torch.initial_seed())
        n = int(number_of_points)
        ns = int(n * 47 / 50) // 2
        nu = n - 2 * ns
        surface = torch.zeros((self.S, ns, 3), dtype=torch.float32, device=self.device)
        has = self.sizes > 0
        for s in range(self.S):
            r = torch.rand(ns, generator=g, dtype=torch.float64)
            size = int(self.sizes[s])
            if size:
                pick = (r * size).long().clamp_(max=size - 1).to(self.device) + self.offsets[s]
                surface[s] = self.points[pick]
        coarse = torch.randn((self.S, ns, 3), generator=g) * 0.0025
        fine = torch.randn((self.S, ns, 3), generator=g) * 0.00025
        uniform = _unit_sphere_points(self.S * nu, g).reshape(self.S, nu, 3)
        points = torch.cat([surface + coarse.to(self.device), surface + fine.to(self.device), uniform.to(self.device)], dim=1).contiguous()
        sdf = self._sdf(points, sample_count)
        inside = (sdf[:, n - nu:] < 0).sum(dim=1).cpu().double() / max(nu, 1)
        ok = has & (inside >= min_size)
        if self.single:
            if not bool(ok[0]):
                raise BadMeshException()
            return points[0], sdf[0]
        return points, sdf, ok


# ---- files ------------------------------------------------------------------------------------------------------------------------------
def _read_ply(path):
    with open(path, "rb") as fh:
        if fh.readline().strip() != b"ply":
            raise ValueError("%s: not a .ply file" % path)
        fmt, count, names, element = None, 0, [], None
        while True:
            line = fh.readline()
            if not line:
                raise ValueError("%s: the header does not end" % path)
            words = line.decode("ascii", "replace").split()
            if not words:
                continue
            if words[0] == "end_header":
                break
            if words[0] == "format":
                fmt = words[1]
            elif words[0] == "element":
                element = words[1]
                if element == "vertex":
                    count = int(words[2])
            elif words[0] == "property" and element == "vertex":
                if words[1] != "float" and words[1] != "float32":
                    raise ValueError("%s: vertex properties must be float, got %s" % (path, words[1]))
                names.append(words[2])
        if fmt == "binary_little_endian":
            data = np.frombuffer(fh.read(count * len(names) * 4), dtype="<f4").reshape(count, len(names))
        elif fmt == "ascii":
            data = np.array([fh.readline().split()[:len(names)] for _ in range(count)], dtype=np.float32).reshape(count, len(names))
        else:
            raise ValueError("%s: .ply format %r is not read (binary_little_endian and ascii are)" % (path, fmt))
    if not all(c in names for c in "xyz"):
        raise ValueError("%s: no x y z vertex properties" % path)
    points = data[:, [names.index(c) for c in "xyz"]]
    normals = data[:, [names.index(c) for c in ("nx", "ny", "nz")]] if all(c in names for c in ("nx", "ny", "nz")) else None
    return points, normals


def load_cloud(path):
    """(points [P, 3] float32, normals [P, 3] float32 or None) from .npy ([P, 3] or [P, 6]), ASCII .xyz (3 or 6 numbers per line) or .ply as
    Mesh.export writes it (vertices with optional nx ny nz; the faces are not read)."""
    ext = os.path.splitext(str(path))[1].lower()
    if ext == ".npy":
        data = np.load(path)
    elif ext == ".xyz":
        rows = []
        with open(path, "r") as fh:
            for line in fh:
                words = line.split()
                if words and not words[0].startswith("#"):
                    rows.append([float(w) for w in words])
        data = np.array(rows, dtype=np.float64).reshape(len(rows), -1) if rows else np.zeros((0, 3))
    elif ext == ".ply":
        points, normals = _read_ply(path)
        return np.ascontiguousarray(points, dtype=np.float32), None if normals is None else np.ascontiguousarray(normals, dtype=np.float32)
    else:
        raise ValueError("load_cloud: unknown cloud format %r (.npy, .xyz and .ply are read)" % ext)
    if data.ndim != 2 or data.shape[1] not in (3, 6):
        raise ValueError("%s: expected [P, 3] or [P, 6], got %s" % (path, data.shape))
    data = np.ascontiguousarray(data, dtype=np.float32)
    return data[:, :3].copy(), (data[:, 3:].copy() if data.shape[1] == 6 else None)


CLOUD_EXTENSIONS = (".npy", ".xyz", ".ply")


def get_cloud_files(directory):
    found = []
    for root, _, files in os.walk(directory):
        found.extend(os.path.join(root, name) for name in files if name.lower().endswith(CLOUD_EXTENSIONS))
    return sorted(found)
