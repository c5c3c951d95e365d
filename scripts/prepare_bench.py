"""Meshes to SDF training data on the GPU (shapegan_amd/prepare.py, csrc/meshsdf.hip), from seeded synthetic meshes only; prints one JSON line.

    python scripts/prepare_bench.py                    # device-event times
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/prepare_bench.py --iters 1 --no-baseline --no-pipeline
        # per-kernel times (msdf_distance_kernel is nearly all of the distance cases)

Cases:
  distance   sg_meshsdf_distance (dist2, tri and closest) in pairs per second at Q = 64^3 queries per shape for T = 5 000 and 50 000
             triangles per shape, S = 1 and 8 shapes; and at Q = 8^3 against T = 200 000, where the grid has to split the triangles.
  pipeline   one mesh (a bumpy sphere of --pipeline-triangles triangles) through what prepare_shapenet_dataset.py does per model at the
             reference's settings: 50 scans of 1024^2 for the unit cube and again for the unit sphere, voxels at 8, 16, 32, 64, 64^3
             uniform + surface points, a 200 000-point cloud; per stage the median wall-clock time of --pipeline-repeats
             device-synchronised runs, without file I/O.
Baselines, which never run the code under test:
  eager      the same distances (dist2 and tri) by chunked eager-torch broadcasting on the device: Ericson's closest point of every
             pair, queries x triangles in blocks that fit 2 GB.
  twin       the C++ twin on the host's threads (OMP_NUM_THREADS, 16 on the bench machine) at a size it finishes in seconds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shapegan_amd import prepare as P  # noqa: E402
from shapegan_amd.rendering import raster  # noqa: E402
from eval_bench import timed  # noqa: E402


def bumpy_sphere(triangles, seed=0):
    """A closed latitude / longitude sphere with a smooth radial bump pattern: (vertices [V, 3] float64, faces [F, 3]), F ~ triangles."""
    nv = max(3, int(round((triangles / 4.0) ** 0.5)))
    nu = 2 * nv
    rng = np.random.RandomState(seed)
    a = np.arange(nu) * (2 * np.pi / nu)
    b = (np.arange(nv - 1) + 1) * (np.pi / nv)
    A, B = np.meshgrid(a, b, indexing="ij")
    phase = rng.uniform(0, 2 * np.pi, 3)
    r = 0.75 + 0.08 * np.sin(3 * A + phase[0]) * np.sin(4 * B + phase[1]) + 0.04 * np.cos(7 * A + phase[2])
    ring = np.stack([r * np.sin(B) * np.cos(A), r * np.cos(B), r * np.sin(B) * np.sin(A)], axis=-1).reshape(-1, 3)
    v = np.concatenate([ring, [[0, 0.75, 0], [0, -0.75, 0]]])
    top, bottom, m = len(ring), len(ring) + 1, nv - 1
    f = []
    for i in range(nu):
        j = (i + 1) % nu
        f.append((top, j * m, i * m))
        f.append((bottom, i * m + m - 1, j * m + m - 1))
        for k in range(m - 1):
            f += [(i * m + k, j * m + k, j * m + k + 1), (i * m + k, j * m + k + 1, i * m + k + 1)]
    return v, np.asarray(f, dtype=np.int64)


def soup_of(S, T, device):
    parts = []
    for s in range(S):
        v, f = bumpy_sphere(T, seed=s)
        parts.append(v[f][:T].astype(np.float32))
    counts = [len(p) for p in parts]
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(device)
    return raster.Soup(torch.from_numpy(np.concatenate(parts)).to(device), None, offsets), counts


def grid_points(S, R, device):
    c = torch.linspace(-1, 1, R)
    g = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), dim=-1).reshape(1, -1, 3)
    return g.expand(S, -1, -1).contiguous().to(device)


def eager_distance(tris, points, budget=2 << 30):
    """(dist2 [Q], tri [Q]) of one shape by eager torch: Ericson's closest point on a triangle for every pair, in query blocks."""
    a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
    ab, ac = b - a, c - a
    T, Q = tris.shape[0], points.shape[0]
    rows = max(1, int(budget // (T * 4 * 40)))
    best, arg = [], []
    for q0 in range(0, Q, rows):
        p = points[q0:q0 + rows, None, :]
        ap, bp, cp = p - a, p - b, p - c
        d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
        d3, d4 = (ab * bp).sum(-1), (ac * bp).sum(-1)
        d5, d6 = (ab * cp).sum(-1), (ac * cp).sum(-1)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        denom = 1.0 / (va + vb + vc)
        v, w = vb * denom, vc * denom                                      # face
        t_ab, t_ac, t_bc = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
        zero, one = torch.zeros_like(v), torch.ones_like(v)
        on_a = (d1 <= 0) & (d2 <= 0)
        on_b = (d3 >= 0) & (d4 <= d3)
        on_c = (d6 >= 0) & (d5 <= d6)
        on_ab = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        on_ac = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        on_bc = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)
        for mask, vv, ww in ((on_bc, 1 - t_bc, t_bc), (on_ac, zero, t_ac), (on_ab, t_ab, zero), (on_c, zero, one), (on_b, one, zero),
                             (on_a, zero, zero)):
            v, w = torch.where(mask, vv, v), torch.where(mask, ww, w)
        r = ap - v[..., None] * ab - w[..., None] * ac
        d = (r * r).sum(-1)
        m = d.min(dim=1)
        best.append(m.values)
        arg.append(m.indices)
    return torch.cat(best), torch.cat(arg)


def staged(fn, repeats):
    """(median wall-clock milliseconds of `repeats` device-synchronised runs, the last result)."""
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), r


def pipeline(triangles, scan_count, scan_resolution, resolutions, sample_size, cloud_size, repeats):
    """One model at the reference's settings; per stage the median milliseconds of `repeats` runs."""
    v, f = bumpy_sphere(triangles, seed=3)
    g = torch.Generator().manual_seed(0)
    stages = {}
    stages["scans_unit_cube_ms"], cube = staged(lambda: P.SurfaceScans((P.scale_to_unit_cube(v), f), 3 ** 0.5, scan_count, scan_resolution), repeats)
    for r in resolutions:
        stages["voxels_%d_ms" % r], _ = staged(lambda: cube.get_voxels(r, check_result=True), repeats)
    del cube
    stages["scans_unit_sphere_ms"], sphere = staged(lambda: P.SurfaceScans((P.scale_to_unit_sphere(v), f), 1.0, scan_count, scan_resolution), repeats)
    stages["uniform_and_surface_ms"], _ = staged(lambda: sphere.get_uniform_and_surface_points(sample_size, g), repeats)
    stages["sdf_cloud_ms"], _ = staged(lambda: sphere.sample_sdf_near_surface(cloud_size, generator=g), repeats)
    return {"triangles": int(len(f)), "scan_count": scan_count, "scan_resolution": scan_resolution, "resolutions": list(resolutions),
            "sample_size": sample_size, "cloud_size": cloud_size, "repeats": repeats, "total_ms": round(sum(stages.values()), 2),
            "stages": {k: round(x, 2) for k, x in stages.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--no-pipeline", action="store_true")
    ap.add_argument("--pipeline-repeats", type=int, default=5)
    ap.add_argument("--pipeline-triangles", type=int, default=20000)
    ap.add_argument("--twin-queries", type=int, default=32 ** 3)
    ap.add_argument("--twin-triangles", type=int, default=5000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prepare_bench needs a GPU"
    dev = torch.device("cuda")
    out = {"device": torch.cuda.get_device_properties(0).name, "distance": []}
    for R, T, S in ((64, 5000, 1), (64, 50000, 1), (64, 5000, 8), (64, 50000, 8), (8, 200000, 1)):
        soup, counts = soup_of(S, T, dev)
        points = grid_points(S, R, dev)
        ms, (dist2, tri, closest, split) = timed(lambda: P.mesh_distance(soup, points), args.iters)
        pairs = float(sum(counts)) * R ** 3
        out["distance"].append({"case": "Q = %d^3, T = %d, S = %d" % (R, counts[0], S), "ms": round(ms, 3), "split": split,
                                "pairs_per_s": round(pairs / ms * 1e3, 0)})
    if not args.no_baseline:
        soup, counts = soup_of(1, 5000, dev)
        points = grid_points(1, 64, dev)
        ms, (d_eager, i_eager) = timed(lambda: eager_distance(soup.positions, points[0]), 1)
        dist2 = P.mesh_distance(soup, points)[0][0]
        out["eager_torch"] = {"case": "Q = 64^3, T = %d, S = 1" % counts[0], "ms": round(ms, 3),
                              "pairs_per_s": round(counts[0] * 64.0 ** 3 / ms * 1e3, 0),
                              "largest_difference_of_distances": float((d_eager.sqrt() - dist2.sqrt()).abs().max())}
        cpu_soup, counts = soup_of(1, args.twin_triangles, "cpu")
        cpu_points = torch.rand((1, args.twin_queries, 3), generator=torch.Generator().manual_seed(0)) * 2 - 1
        P.mesh_distance(cpu_soup, cpu_points[:, :64])
        t0 = time.perf_counter()
        P.mesh_distance(cpu_soup, cpu_points)
        s = time.perf_counter() - t0
        out["twin"] = {"case": "Q = %d, T = %d, S = 1" % (args.twin_queries, counts[0]), "threads": int(os.environ.get("OMP_NUM_THREADS", 0)),
                       "ms": round(s * 1e3, 2), "pairs_per_s": round(counts[0] * float(args.twin_queries) / s, 0)}
    if not args.no_pipeline:
        pipeline(2000, 4, 128, (8,), 4096, 2000, 1)      # warm-up: libraries, allocator, first launches
        out["pipeline"] = pipeline(args.pipeline_triangles, 50, 1024, (8, 16, 32, 64), 64 ** 3, 200000, args.pipeline_repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
