"""Point-cloud evaluation on the GPU (shapegan_amd/evaluation.py), from seeded synthetic clouds only; prints one JSON line.

    python scripts/eval_bench.py                 # device-event times
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/eval_bench.py --iters 2 --no-baseline
        # per-kernel times (chamfer_rows_kernel is the whole of it)

Cases: chamfer_matrix of 1000 x 1000 and of 50 x 50 clouds of 2048 points (both directions: two sweeps of the pair table), and
evaluate(1000 generated, 1000 dataset): three matrices (four sweeps) plus the histograms and the scalar read-back.

Baseline: the same two matrices in eager torch on the same GPU, one torch.cdist per row of the matrix against a block of
columns, squared, then the two minima and means.  It is timed on a sub-block (--baseline-rows x --baseline-cols) small enough to
finish and scaled by the pair count; the factor is printed.  It never runs the code under test.

Share of the vector-pipe bound: pairs/s against  CUs x 4 SIMDs x 16 lanes x clock / (VALU instructions per pair).  The
instruction count is read off the inner loop of chamfer_rows_kernel in the compiler's .s output and passed in
--valu-per-pair; a sweep visits every pair once, so a two-direction matrix costs twice that per pair.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shapegan_amd import evaluation as E  # noqa: E402


def synthetic_clouds(S, P, seed):
    """Seeded mix of sphere surfaces, box volumes and Gaussian blobs inside the half unit sphere."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((S, P, 3), generator=g, device="cuda")
    kind = torch.arange(S, device="cuda") % 3
    radius = 0.2 + 0.3 * torch.rand((S, 1, 1), generator=g, device="cuda")
    sphere = x / x.norm(dim=2, keepdim=True) * radius
    box = (torch.rand((S, P, 3), generator=g, device="cuda") * 2 - 1) * radius * 0.55
    blob = x * radius * 0.3
    out = torch.where((kind == 0)[:, None, None], sphere, torch.where((kind == 1)[:, None, None], box, blob))
    return (out + 0.02 * torch.randn((S, 1, 3), generator=g, device="cuda")).contiguous()


def timed(fn, iters, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        r = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters, r


def eager_matrix(a, b):
    """The baseline: per row of the matrix one batched torch.cdist against the block of columns."""
    ab = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float64, device=a.device)
    ba = torch.empty_like(ab)
    for i in range(a.shape[0]):
        d = torch.cdist(a[i].unsqueeze(0).expand(b.shape[0], -1, -1), b) ** 2          # [cols, P, Q]
        ab[i] = d.min(dim=2).values.double().mean(dim=1)
        ba[i] = d.min(dim=1).values.double().mean(dim=1)
    return ab, ba


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--clouds", type=int, default=1000)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--valu-per-pair", type=float, default=3.6, help="VALU instructions per pair and sweep, from the .s file")
    ap.add_argument("--clock-mhz", type=float, default=2400.0, help="engine clock the bound is taken at (MI355X peak: 2400)")
    ap.add_argument("--baseline-rows", type=int, default=8)
    ap.add_argument("--baseline-cols", type=int, default=64)
    ap.add_argument("--no-baseline", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "eval_bench needs a GPU"
    S, P = args.clouds, args.points
    gen, ref = synthetic_clouds(S, P, 11), synthetic_clouds(S, P, 12)
    props = torch.cuda.get_device_properties(0)
    clock_hz = args.clock_mhz * 1e6
    bound = props.multi_processor_count * 4 * 16 * clock_hz / args.valu_per_pair      # pairs per second and sweep
    result = {"metric": "evaluation", "clouds": S, "points": P, "compute_units": props.multi_processor_count,
              "clock_mhz": round(clock_hz / 1e6), "valu_per_pair_per_sweep": args.valu_per_pair,
              "vector_pipe_bound_pairs_per_s_per_sweep": bound}

    for name, n in (("matrix_%dx%d" % (S, S), S), ("matrix_50x50", min(50, S))):
        ms, (ab, ba) = timed(lambda: E.chamfer_matrix(gen[:n], ref[:n]), args.iters)
        pairs = float(n) * n * P * P
        swept = 2 * pairs / (ms * 1e-3)
        result[name] = {"ms": round(ms, 3), "pairs": pairs, "pairs_per_s": pairs / (ms * 1e-3), "swept_pairs_per_s": swept,
                        "share_of_vector_pipe_bound": round(swept / bound, 4),
                        "finite": bool(torch.isfinite(ab).all() and torch.isfinite(ba).all())}

    ms, scores = timed(lambda: E.evaluate(gen, ref), max(1, args.iters // 2))
    result["evaluate_%dx%d" % (S, S)] = {"ms": round(ms, 3), "scores": scores}

    if not args.no_baseline:
        rows, cols = min(args.baseline_rows, S), min(args.baseline_cols, S)
        ms, (eab, eba) = timed(lambda: eager_matrix(gen[:rows], ref[:cols]), 2)
        ab, ba = E.chamfer_matrix(gen[:rows], ref[:cols])
        factor = float(S) * S / (rows * cols)
        result["eager_torch_baseline"] = {
            "sub_block": [rows, cols], "sub_block_ms": round(ms, 3), "scale_factor": factor, "scaled_ms": round(ms * factor, 1),
            # the two agree to float32 rounding of the expanded form (cdist may use |a|^2 + |b|^2 - 2ab): a sanity figure only
            "max_rel_difference_to_kernels": float(((eab - ab).abs() / ab).max())}
        result["speedup_over_eager_torch"] = round(ms * factor / result["matrix_%dx%d" % (S, S)]["ms"], 1)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
