"""The point-cloud SDF kernels on the GPU against the 1-nearest walk they are modelled on, from seeded inputs only; prints one JSON line.

    python scripts/cloud_bench.py [--iters N] [--out profiles/cloud_sdf_mi355x.json]

Two cases, both in point pairs per second (queries x cloud points of a shape, summed over the shapes, over the device-event time):
  self k-NN     8 clouds of 30 000 points, K = 16, every point against its own cloud (sg_cloud_knn, exclude_self)
  cloud SDF     8 x 64^3 grid queries against clouds of 30 000 oriented points, K = 11 (sg_cloud_sdf)
Next to each, in the same run and at the same sizes: sg_chamfer_nearest in ONE direction (the same walk with one minimum instead of a
list: the yardstick) and eager torch `cdist + topk` in chunks of queries.  Host baselines: the C++ twin and, when it can be imported,
scipy.spatial.cKDTree, both on the FIRST shape alone with a share of the queries (wall clock; their pairs per second are brute-force
equivalents: the same pair count over their time).  Nothing is asserted about speed."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from shapegan_amd import cloudsdf as C  # noqa: E402
from shapegan_amd import lib as L  # noqa: E402

S, P = 8, 30000
HOST_QUERIES = 4096


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def nearest_one_way(queries, clouds):
    """sg_chamfer_nearest from queries [S, Q, 3] to clouds [S, P, 3], one direction."""
    Sn, Q, Pn = queries.shape[0], queries.shape[1], clouds.shape[1]
    dist = torch.empty((Sn, Q), dtype=torch.float32, device=queries.device)
    idx = torch.empty((Sn, Q), dtype=torch.int32, device=queries.device)
    try:
        L.check(L.load().sg_chamfer_nearest(L.ptr(queries), L.ptr(clouds), Sn, Q, Pn, L.ptr(dist), L.ptr(idx), None, None, L.stream()),
                "chamfer_nearest")
    finally:
        L.reset_call_state()
    return dist, idx


def torch_topk(queries, clouds, k, chunk=8192):
    out = []
    for s in range(queries.shape[0]):
        for i in range(0, queries.shape[1], chunk):
            out.append(torch.cdist(queries[s, i:i + chunk], clouds[s]).topk(k, dim=1, largest=False))
    return out


def host_baselines(queries, cloud, normals, k, pairs_per_query):
    """The twin and cKDTree on one shape: {name: {"ms", "pairs_per_s"}}."""
    q, p, n = queries[:HOST_QUERIES].cpu().contiguous(), cloud.cpu().contiguous(), None if normals is None else normals.cpu().contiguous()
    co, qo = torch.tensor([0, p.shape[0]]), torch.tensor([0, q.shape[0]])
    t0 = time.perf_counter()
    if n is None:
        C.knn_ragged(p, co, q, qo, k)
    else:
        C.sdf_ragged(p, n, co, q, qo, k)
    twin = time.perf_counter() - t0
    pairs = q.shape[0] * pairs_per_query
    out = {"twin": {"queries": q.shape[0], "ms": round(twin * 1e3, 3), "pairs_per_s": pairs / twin}}
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        out["ckdtree"] = "scipy cannot be imported"
        return out
    t0 = time.perf_counter()
    tree = cKDTree(p.numpy())
    tree.query(q.numpy(), k=k)
    kd = time.perf_counter() - t0
    out["ckdtree"] = {"queries": q.shape[0], "ms_with_build": round(kd * 1e3, 3), "brute_force_equivalent_pairs_per_s": pairs / kd}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "cloud_bench needs a GPU"
    g = torch.Generator().manual_seed(0)
    direction = torch.randn((S, P, 3), generator=g)
    normals = (direction / direction.norm(dim=2, keepdim=True)).cuda().contiguous()
    clouds = (normals * (0.5 + 0.05 * torch.randn((S, P, 1), generator=g).cuda())).contiguous()      # noisy spheres
    flat, flat_normals = clouds.reshape(S * P, 3), normals.reshape(S * P, 3)
    co = torch.arange(S + 1, dtype=torch.int64, device="cuda") * P
    cases = []

    # ---- the self k-NN
    pairs = S * P * P
    knn_ms = timed(lambda: C.knn_ragged(flat, co, flat, co, 16, exclude_self=True), args.iters)
    one_ms = timed(lambda: nearest_one_way(clouds, clouds), args.iters)
    topk_ms = timed(lambda: torch_topk(clouds, clouds, 17), max(1, args.iters // 2), warmup=1)
    cases.append({"case": "self_knn", "shapes": S, "points": P, "queries_per_shape": P, "k": 16, "pairs": pairs,
                  "cloud_knn_ms": round(knn_ms, 3), "cloud_knn_pairs_per_s": pairs / knn_ms * 1e3,
                  "chamfer_nearest_ms": round(one_ms, 3), "chamfer_nearest_pairs_per_s": pairs / one_ms * 1e3,
                  "knn_over_nearest_time": round(knn_ms / one_ms, 3),
                  "torch_cdist_topk_ms": round(topk_ms, 3), "torch_cdist_topk_pairs_per_s": pairs / topk_ms * 1e3,
                  "host_first_shape": host_baselines(clouds[0], clouds[0], None, 16, P)})

    # ---- the SDF of a 64^3 grid
    R = 64
    c = torch.linspace(-1.0, 1.0, R, dtype=torch.float64)
    grid = torch.stack(torch.meshgrid(c, c, c, indexing="ij"), dim=-1).reshape(1, R ** 3, 3).float().cuda().expand(S, R ** 3, 3).contiguous()
    Q = R ** 3
    qo = torch.arange(S + 1, dtype=torch.int64, device="cuda") * Q
    pairs = S * Q * P
    sdf_ms = timed(lambda: C.sdf_ragged(flat, flat_normals, co, grid.reshape(S * Q, 3), qo, 11), args.iters)
    one_ms = timed(lambda: nearest_one_way(grid, clouds), args.iters)
    topk_ms = timed(lambda: torch_topk(grid, clouds, 11), 1, warmup=1)
    cases.append({"case": "cloud_sdf_grid", "shapes": S, "points": P, "queries_per_shape": Q, "k": 11, "pairs": pairs,
                  "cloud_sdf_ms": round(sdf_ms, 3), "cloud_sdf_pairs_per_s": pairs / sdf_ms * 1e3,
                  "chamfer_nearest_ms": round(one_ms, 3), "chamfer_nearest_pairs_per_s": pairs / one_ms * 1e3,
                  "sdf_over_nearest_time": round(sdf_ms / one_ms, 3),
                  "torch_cdist_topk_ms": round(topk_ms, 3), "torch_cdist_topk_pairs_per_s": pairs / topk_ms * 1e3,
                  "host_first_shape": host_baselines(grid[0], clouds[0], normals[0], 11, P)})

    result = {"metric": "cloud_sdf", "device": torch.cuda.get_device_name(0), "iters": args.iters, "cases": cases}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
