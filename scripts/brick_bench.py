"""Times dense against narrow-band SDFNet.voxel_grids (csrc/brickgrid.hip, K18) on the GPU; prints ONE JSON line (kept as
profiles/narrow_band_mi355x.json).

    python scripts/brick_bench.py [--resolutions 64,128,256] [--bricks 4,8,16] [--shapes 1,8] [--rounds 3] [--frames 16]

The chairs weights of tests/golden with seeded codes (randn * 0.1, as scripts/tsne_bench.py --frames), sphere_only grids.  Per
resolution R, batch S, brick B and band (the default, lipschitz = 1, and 0: continuation only): the evaluated fraction, the rounds, the
call time, the time inside the network launches (corners / bricks) with the rest (bookkeeping kernels, allocations, the per-round
host read) as their difference, and whether marching cubes of the result equals that of the dense grid bit for bit.  Dense and
narrow-band calls alternate within a round; device events around whole calls (every call ends its rounds with a host read anyway),
median (min - max) of `--rounds`.  --frames F > 0 adds traversal_frames (128^3, 1080 px) both ways, host clock around a synchronise.
A run without a GPU fails: there is no CPU timing to report.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from shapegan_amd import brickgrid as BG  # noqa: E402
from shapegan_amd import traversal as T  # noqa: E402
from shapegan_amd.mesh import marching_cubes  # noqa: E402

LEVEL = 0.0


def summary(samples):
    s = sorted(samples)
    return {"ms": round(s[len(s) // 2], 3), "ms_min": round(s[0], 3), "ms_max": round(s[-1], 3)}


class Timed(object):
    """device events around a call"""

    def __enter__(self):
        self.start, self.end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.start.record()
        return self

    def __exit__(self, *exc):
        self.end.record()
        self.end.synchronize()
        self.ms = self.start.elapsed_time(self.end)


def narrow(net, codes, R, B, band, split=None):
    """SDFNet.voxel_grids(narrow_band=True) spelled out, so that the network launches can carry events of their own"""
    helper = net._helper(R, True)
    evaluate, S = net.point_evaluator(codes)
    if split is not None:
        inner = evaluate

        def evaluate(points, sid):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = inner(points, sid)
            b.record()
            split.append((a, b))
            return out
    with torch.no_grad():
        return BG.narrow_band_grids(evaluate, S, R, codes.device, brick=B, level=LEVEL, band=band, mask=net._mask_tensor(helper, codes.device))


def same_mesh(a, b, R):
    ma = marching_cubes(a, level=LEVEL, spacing=2.0 / R, origin=-1.0, pad=True)
    mb = marching_cubes(b, level=LEVEL, spacing=2.0 / R, origin=-1.0, pad=True)
    same = all(torch.equal(getattr(ma, n), getattr(mb, n)) for n in ("vert_offsets", "tri_offsets", "vertices", "normals", "faces"))
    return same, int(ma.faces.shape[0]), int(mb.faces.shape[0])


def bench_grid(net, codes, R, bricks, rounds):
    S = codes.shape[0]
    variants = [(B, band) for B in bricks if R % B == 0 for band in (None, 0.0)]
    out = {"resolution": R, "shapes": S, "dense_points": S * R ** 3}
    dense = net.voxel_grids(codes, R, sphere_only=True)      # warm-up of every shape the timed window uses
    rows = []
    for B, band in variants:
        res = narrow(net, codes, R, B, band)
        row = {"brick": B, "band": round(res.stats["band"], 5), "band_rule": "default" if band is None else "zero",
               "rounds": res.stats["rounds"], "evaluated_fraction": round(sum(res.stats["evaluated_points"]) / (S * R ** 3), 4),
               "active_brick_fraction": round(sum(res.stats["active_bricks"]) / (S * (R // B) ** 3), 4)}
        if S == 1:
            row["mesh_equal"], row["dense_triangles"], row["narrow_triangles"] = same_mesh(res.grid, dense, R)
        del res
        rows.append(row)
    del dense
    t_dense, t_rows = [], [[] for _ in variants]
    net_rows = [[[], []] for _ in variants]
    for _ in range(rounds):
        with Timed() as t:
            net.voxel_grids(codes, R, sphere_only=True)
        t_dense.append(t.ms)
        for i, (B, band) in enumerate(variants):
            split = []
            with Timed() as t:
                narrow(net, codes, R, B, band, split)
            t_rows[i].append(t.ms)
            net_rows[i][0].append(split[0][0].elapsed_time(split[0][1]))
            net_rows[i][1].append(sum(a.elapsed_time(b) for a, b in split[1:]))
    out["dense"] = summary(t_dense)
    for row, ts, (corner, brick) in zip(rows, t_rows, net_rows):
        row["narrow"] = summary(ts)
        row["network_corners_ms"] = summary(corner)["ms"]
        row["network_bricks_ms"] = summary(brick)["ms"]
        row["other_ms"] = round(row["narrow"]["ms"] - row["network_corners_ms"] - row["network_bricks_ms"], 3)
        row["speedup"] = round(out["dense"]["ms"] / row["narrow"]["ms"], 3)
    out["variants"] = rows
    return out


def bench_frames(net, codes, frames, rounds, bricks):
    tour = codes[torch.arange(frames) % codes.shape[0]]
    out = {"resolution": 128, "size": 1080, "frames": frames, "level": T.SURFACE_LEVEL}

    def run(narrow_band):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        images = list(T.traversal_frames(net, tour, voxel_resolution=128, size=1080, narrow_band=narrow_band))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / frames, images
    options = [False] + [dict(brick=B) for B in bricks if 128 % B == 0]
    reference = run(False)[1]
    equal = [all(a.tobytes() == b.tobytes() for a, b in zip(run(o)[1], reference)) for o in options]      # (also the warm-up)
    times = [[] for _ in options]
    for _ in range(rounds):
        for i, o in enumerate(options):
            times[i].append(run(o)[0])
    out["dense_ms_per_frame"] = summary(times[0])
    out["narrow"] = [dict(brick=o["brick"], frames_equal=e, ms_per_frame=summary(t)) for o, e, t in zip(options[1:], equal[1:], times[1:])]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", default="64,128,256")
    ap.add_argument("--bricks", default="4,8,16")
    ap.add_argument("--shapes", default="1,8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("brick_bench.py measures on the GPU; there is none here")
    import latent_fit_forms as LF
    net = LF.net_on("cuda", 5, 128, LF.chairs_state())
    table = (torch.randn(8, 128, generator=torch.Generator().manual_seed(0)) * 0.1).cuda()
    bricks = [int(b) for b in args.bricks.split(",")]
    result = {"device": torch.cuda.get_device_name(0), "level": LEVEL, "codes": "randn(8, 128, seed 0) * 0.1, chairs weights", "grids": []}
    for R in (int(r) for r in args.resolutions.split(",")):
        for S in (int(s) for s in args.shapes.split(",")):
            result["grids"].append(bench_grid(net, table[:S].contiguous(), R, bricks, args.rounds))
    if args.frames > 0:
        result["traversal"] = bench_frames(net, table, args.frames, args.rounds, bricks)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
