"""The distance transforms of voxel grids on the GPU against the write rate of the device, from seeded inputs only; prints one JSON line.

    python scripts/edt_bench.py [--repeats N] [--out profiles/edt_mi355x.json]

Four workloads:
  distance_transform   1000 x 32^3 and 64 x 64^3 occupancy grids (a noisy sphere's inside)
  redistance_grids     1000 x 32^3 and 8 x 256^3 sphere-noise grids, clamped to [-1, 1] as VoxelDataset holds them
For each (device-event time, median of the repeats after a warm-up): the transform (the site pass and the axis passes; in the LDS form
they are one launch), the finishing step and the public call; per kernel, the device time the profiler attributes to it in one call,
which splits the site pass from the axis passes in the per-axis form; and next to them, in the same process and at the same sizes,
  a) torch.full of the output — the write-rate yardstick.  The memory floor of a call is (launches that stream the grid) x 8 B per voxel
     at that rate in the per-axis form (each reads 4 B and writes 4 B per voxel) and one read plus one write in the LDS form;
  b) the twin (libshapegan_cpu.so) on a few grids, per grid (not at 256^3: the scan of the empty lines takes minutes on one core);
  c) scipy.ndimage.distance_transform_edt of the first grid's mask on the host (wall clock), if scipy imports.
Nothing is asserted about speed."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from shapegan_amd import ops  # noqa: E402
from shapegan_amd import voxeldist  # noqa: E402

# (what, grids, resolution, repeats at most, grids of the twin's run)
WORKLOADS = (("distance_transform", 1000, 32, 20, 32), ("distance_transform", 64, 64, 20, 4), ("redistance_grids", 1000, 32, 20, 32),
             ("redistance_grids", 8, 256, 3, 0))


def timed(fn, repeats, warmup=1):
    """Median device time of fn in ms."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return statistics.median(times)


def sphere_noise(S, n, seed):
    """sdf / 0.1 clamped to [-1, 1] of spheres of varying radius and centre in [-1, 1]^3, plus a little noise; built on the device."""
    g = torch.Generator().manual_seed(seed)
    ax = ((torch.arange(n, dtype=torch.float32) + 0.5) / n * 2 - 1).cuda()
    radius = (0.35 + 0.3 * torch.rand(S, generator=g)).cuda()
    centre = (0.2 * (torch.rand((S, 3), generator=g) - 0.5)).cuda()
    out = torch.empty((S, n, n, n), dtype=torch.float32, device="cuda")
    for s in range(S):
        x, y, z = ax - centre[s, 0], ax - centre[s, 1], ax - centre[s, 2]
        out[s] = torch.sqrt(x[:, None, None] ** 2 + y[None, :, None] ** 2 + z[None, None, :] ** 2) - radius[s]
    out += 0.01 * torch.randn(out.shape, generator=g).cuda()
    return (out / 0.1).clamp_(-1, 1)


def kernel_split(fn):
    """{kernel name: device ms} of one call, from the profiler; a string when it cannot tell."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            total = getattr(ev, "device_time_total", None)
            if total is None:
                total = getattr(ev, "cuda_time_total", 0)
            if "edt_" in ev.key and total:
                name = ev.key.split("(")[0].split("::")[-1]
                out[name] = round(out.get(name, 0.0) + total / 1e3, 3)
        return out or "the profiler reported no kernel of the library"
    except Exception as e:      # the split is an extra: the event times above stand without it
        return "profiler unavailable: %s" % (str(e).splitlines() or [type(e).__name__])[0]


def workload(what, S, n, repeats, twin_grids):
    grids = sphere_noise(S, n, n + S)
    spacing = 2.0 / n
    cells = S * n ** 3
    form = ops.edt_form((n, n, n), grids)
    if what == "distance_transform":
        field = (grids < 0).to(torch.float32)
        transform = lambda: ops.edt_voxels(field, 0.5, True, 1.0)            # noqa: E731
        finish_in = ops.edt_voxels(field, 0.5, True, 1.0)
        finish = lambda: ops.edt_finish(None, finish_in)                     # noqa: E731
        public = lambda: voxeldist.distance_transform(grids < 0)             # noqa: E731
        launches = 1 if form == 0 else 4
    else:
        field = grids
        transform = lambda: ops.edt_crossings(field, 0.0, spacing)           # noqa: E731
        finish_in = ops.edt_crossings(field, 0.0, spacing)
        finish = lambda: ops.edt_finish(field, finish_in, 0.0, 0.1, True)    # noqa: E731
        public = lambda: voxeldist.redistance_grids(grids)                   # noqa: E731
        launches = 1 if form == 0 else 9
    transform_ms, finish_ms, public_ms = timed(transform, repeats), timed(finish, repeats), timed(public, repeats)
    fill_ms = timed(lambda: torch.full((S, n, n, n), 0.5, dtype=torch.float32, device="cuda"), max(repeats, 10))
    fill_rate = cells * 4 / fill_ms / 1e6                                    # GB/s
    floor_ms = launches * cells * 8 / fill_rate / 1e6
    case = {"what": what, "grids": S, "resolution": n, "form": form, "repeats": repeats, "transform_ms": round(transform_ms, 3),
            "finish_ms": round(finish_ms, 3), "public_call_ms": round(public_ms, 3), "kernels_ms": kernel_split(transform),
            "fill_ms": round(fill_ms, 3), "fill_GBps": round(fill_rate, 1), "launches_that_stream_the_grid": launches,
            "memory_floor_ms": round(floor_ms, 3), "transform_over_floor": round(transform_ms / floor_ms, 2),
            "finish_over_fill": round(finish_ms / fill_ms, 2), "Mvoxels_per_s": round(cells / transform_ms / 1e3, 1)}
    if twin_grids:
        host = field[:twin_grids].cpu()
        run = (lambda: ops.edt_voxels(host, 0.5, True, 1.0)) if what == "distance_transform" else (lambda: ops.edt_crossings(host, 0.0, spacing))
        run()
        t0 = time.perf_counter()
        run()
        one = (time.perf_counter() - t0) * 1e3 / twin_grids
        case["twin"] = {"grids_timed": twin_grids, "threads": torch.get_num_threads(), "ms_per_grid": round(one, 3),
                        "speedup_per_grid": round(one / (transform_ms / S), 1)}
    else:
        case["twin"] = "not timed at this size"
    try:
        from scipy import ndimage
    except ImportError:
        case["scipy_host"] = "scipy cannot be imported"
    else:
        mask = (grids[0] < 0).cpu().numpy()
        t0 = time.perf_counter()
        ndimage.distance_transform_edt(mask)
        one = (time.perf_counter() - t0) * 1e3
        case["scipy_host"] = {"grids_timed": 1, "ms_per_grid": round(one, 3), "speedup_per_grid": round(one / (transform_ms / S), 1)}
    del grids, field, finish_in
    torch.cuda.empty_cache()
    print("done: %s" % json.dumps(case), file=sys.stderr, flush=True)
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20, help="at most; the large workload takes 3")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "edt_bench needs a GPU"
    result = {"metric": "voxel_distance_transform", "device": torch.cuda.get_device_name(0),
              "cases": [workload(what, S, n, min(args.repeats, most), twin) for what, S, n, most, twin in WORKLOADS]}
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
