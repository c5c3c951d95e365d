"""The voxel zoom on the GPU against the write rate of the device, from seeded inputs only; prints one JSON line.

    python scripts/zoom_bench.py [--iters N] [--out profiles/zoom_mi355x.json]

Two workloads of voxelzoom.zoom_grids, order 3:
  32^3 -> 128^3   1000 grids (one metrics.sample_from_voxels call of the evaluation: 8.4 GB of output)
  64^3 -> 256^3   64 grids (4.3 GB of output)
For each: the prefilter and the zoom apart (device-event time), and next to them, in the same process and at the same sizes,
  a) torch.full of the output's size — the write-rate yardstick: the zoom's share of it is (fill ms) / (zoom ms);
  b) F.interpolate(mode='trilinear', align_corners=True) — the same sample positions, no prefilter, 8 taps;
  c) scipy.ndimage.zoom on the host, of the FIRST grid alone (wall clock), if scipy imports.
Then metrics.sample_from_voxels of 64 grids of 32^3 with and without upscale=4 (wall clock, host transfers included).
Nothing is asserted about speed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from shapegan_amd import metrics  # noqa: E402
from shapegan_amd import ops  # noqa: E402

WORKLOADS = ((1000, 32, 128), (64, 64, 256))


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


def workload(S, n, N, iters):
    g = torch.Generator().manual_seed(n)
    grids = torch.randn((S, n, n, n), generator=g).clamp_(-1, 1).cuda()
    size = (N, N, N)
    out_bytes = S * N ** 3 * 4
    coefficients = ops.spline_prefilter(grids)
    prefilter_ms = timed(lambda: ops.spline_prefilter(grids), iters)
    zoom_ms = timed(lambda: ops.spline_zoom(coefficients, size, 3), iters)
    linear_ms = timed(lambda: ops.spline_zoom(grids, size, 1), iters)
    fill_ms = timed(lambda: torch.full((S,) + size, 0.5, dtype=torch.float32, device="cuda"), iters)
    trilinear_ms = timed(lambda: F.interpolate(grids[:, None], size=size, mode="trilinear", align_corners=True), iters)
    total_ms = prefilter_ms + zoom_ms
    case = {"grids": S, "from": n, "to": N, "output_bytes": out_bytes, "prefilter_form": ops.spline_prefilter_form((n, n, n), grids),
            "zoom_form": ops.spline_zoom_form((n, n, n), size, grids),
            "prefilter_ms": round(prefilter_ms, 3), "zoom_ms": round(zoom_ms, 3), "total_ms": round(total_ms, 3),
            "prefilter_share_of_total": round(prefilter_ms / total_ms, 4),
            "zoom_output_GBps": round(out_bytes / zoom_ms / 1e6, 1),
            "fill_ms": round(fill_ms, 3), "fill_GBps": round(out_bytes / fill_ms / 1e6, 1),
            "zoom_share_of_fill_rate": round(fill_ms / zoom_ms, 4),
            "zoom_order1_ms": round(linear_ms, 3),
            "torch_trilinear_ms": round(trilinear_ms, 3), "speedup_over_torch_trilinear": round(trilinear_ms / total_ms, 3)}
    try:
        from scipy import ndimage
    except ImportError:
        case["scipy_host"] = "scipy cannot be imported"
    else:
        first = grids[0].cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        ndimage.zoom(first, N / n)
        one = time.perf_counter() - t0
        case["scipy_host"] = {"grids_timed": 1, "ms_per_grid": round(one * 1e3, 3), "speedup_per_grid": round(one * 1e3 / (total_ms / S), 1)}
    del coefficients, grids
    torch.cuda.empty_cache()
    return case


def sample_from_voxels_case(count=64, points=2048):
    c = (np.arange(32) + 1) * 2.0 / 32 - 1
    x, y, z = np.meshgrid(c, c, c, indexing="ij")
    rng = np.random.default_rng(0)
    voxels = np.stack([np.sqrt((x - 0.03) ** 2 + (y / a) ** 2 + z ** 2) - 0.5 for a in rng.uniform(0.6, 1.4, count)]).astype(np.float32)
    out = {"grids": count, "resolution": 32, "points": points}
    for name, upscale in (("plain_ms", None), ("upscale4_ms", 4)):
        metrics.sample_from_voxels(voxels[:4], points, upscale=upscale)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        metrics.sample_from_voxels(voxels, points, upscale=upscale)
        torch.cuda.synchronize()
        out[name] = round((time.perf_counter() - t0) * 1e3, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "zoom_bench needs a GPU"
    result = {"metric": "voxel_zoom", "device": torch.cuda.get_device_name(0), "iters": args.iters,
              "cases": [workload(S, n, N, args.iters) for S, n, N in WORKLOADS], "sample_from_voxels": sample_from_voxels_case()}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
