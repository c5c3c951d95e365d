"""Earth mover's distance on the GPU (shapegan_amd/evaluation.py, csrc/emd.hip), from seeded synthetic clouds only; prints one JSON line.

    python scripts/emd_bench.py                        # device-event times
    python scripts/emd_bench.py --sweep                # also: where to switch between the two forms of a round
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/emd_bench.py --iters 1 --no-baseline
        # per-kernel times (emd_auction_kernel is the whole of it)

Cases: emd_matrix of 50 x 50 and of 8 x 8 clouds of 2048 points for eps = 1e-3, 1e-4 and 1e-5, with the rounds per pair (median and
largest; the library leaves them in the caller's workspace), and the symmetric 50 x 50 matrix `evaluate` uses for two of its three.

Baseline: scipy.optimize.linear_sum_assignment on the float64 distances of ONE of those pairs on the host (it is exact; the auction
is within eps).  It never runs the code under test.

--sweep: sg_emd_match_impl on 64 pairs at eps = 1e-4 with the switch points "W/B" of --sweep-points (bidders of a round at or below
which a wave scans for one bidder / the whole workgroup does); the results are the same bits for every value, and that is asserted.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shapegan_amd import lib as L  # noqa: E402
from eval_bench import synthetic_clouds, timed  # noqa: E402


def matrix_call(a, b, eps, symmetric=False):
    """sg_emd_matrix with a workspace of its own: (emd [Sa, Sb], status, rounds)."""
    Sa, Sb, P = a.shape[0], b.shape[0], a.shape[1]
    lib = L.load()
    emd = torch.empty((Sa, Sb), dtype=torch.float64, device=a.device)
    status = torch.empty((Sa, Sb), dtype=torch.int32, device=a.device)
    rounds = torch.empty((Sa, Sb), dtype=torch.int32, device=a.device)
    assert lib.sg_emd_matrix_workspace_bytes(Sa, Sb, P) == rounds.numel() * 4
    try:
        L.check(lib.sg_emd_matrix(L.ptr(a), L.ptr(b), Sa, Sb, P, eps, int(symmetric), L.ptr(emd), L.ptr(status), L.ptr(rounds),
                                  rounds.numel() * 4, L.stream()), "emd_matrix")
    finally:
        L.reset_call_state()
    return emd, status, rounds


def match_impl(a, b, eps, wave_scan_at, block_scan_at):
    S, P = a.shape[0], a.shape[1]
    emd = torch.empty(S, dtype=torch.float64, device=a.device)
    match = torch.empty((S, P), dtype=torch.int32, device=a.device)
    rounds, status = (torch.empty(S, dtype=torch.int32, device=a.device) for _ in range(2))
    try:
        L.check(L.load().sg_emd_match_impl(L.ptr(a), L.ptr(b), S, P, eps, L.ptr(match), L.ptr(emd), L.ptr(rounds), L.ptr(status),
                                           wave_scan_at, block_scan_at, L.stream()), "emd_match_impl")
    finally:
        L.reset_call_state()
    return emd, match, rounds, status


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--sizes", type=int, nargs="+", default=[50, 8])
    ap.add_argument("--eps", type=float, nargs="+", default=[1e-3, 1e-4, 1e-5])
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sweep-points", nargs="+", default=["0/0", "16/0", "64/0", "160/0", "256/0", "160/1", "160/2", "160/3", "160/4",
                                                          "160/8", "64/2", "256/2"])
    ap.add_argument("--sweep-pairs", type=int, default=64)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "emd_bench needs a GPU"
    P = args.points
    out = {"device": torch.cuda.get_device_properties(0).name, "points": P, "cases": []}
    for S in args.sizes:
        gen, ref = synthetic_clouds(S, P, 11), synthetic_clouds(S, P, 12)
        for eps in args.eps:
            ms, (emd, status, rounds) = timed(lambda: matrix_call(gen, ref, eps), args.iters)
            assert not bool(status.any()), "a pair failed"
            r = rounds.flatten().cpu().numpy()
            out["cases"].append({"case": "emd_matrix %d x %d" % (S, S), "eps": eps, "ms": round(ms, 3), "pairs": S * S,
                                 "pairs_per_s": round(S * S / ms * 1e3, 1), "rounds_median": int(np.median(r)), "rounds_max": int(r.max()),
                                 "mean_emd": float(emd.mean())})
        ms, (emd, status, rounds) = timed(lambda: matrix_call(gen, gen, 1e-4, True), args.iters)
        assert not bool(status.any())
        out["cases"].append({"case": "emd_matrix %d x %d symmetric" % (S, S), "eps": 1e-4, "ms": round(ms, 3), "pairs": S * (S - 1) // 2})
    if args.sweep:
        n = args.sweep_pairs
        a, b = synthetic_clouds(n, P, 21), synthetic_clouds(n, P, 22)
        want = match_impl(a, b, 1e-4, -1, -1)
        sweep = []
        for point in args.sweep_points:
            wave_at, block_at = (int(x) for x in point.split("/"))
            ms, got = timed(lambda: match_impl(a, b, 1e-4, wave_at, block_at), args.iters)
            assert all(torch.equal(x, y) for x, y in zip(got, want)), "the switch points changed a result"
            sweep.append({"wave_scan_at": wave_at, "block_scan_at": block_at, "ms": round(ms, 3)})
        out["sweep"] = {"pairs": n, "eps": 1e-4, "rounds_median": int(want[2].median()), "points": sweep}
    if not args.no_baseline:
        from scipy.optimize import linear_sum_assignment
        a, b = (synthetic_clouds(1, P, s)[0].double().cpu().numpy() for s in (11, 12))
        t0 = time.perf_counter()
        d = np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2))
        rows, cols = linear_sum_assignment(d)
        out["host_linear_sum_assignment"] = {"pairs": 1, "s": round(time.perf_counter() - t0, 3), "emd": float(d[rows, cols].mean())}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
