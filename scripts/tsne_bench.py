"""Times exact t-SNE (csrc/tsne.hip) and the traversal built on it on the GPU; prints ONE JSON line (kept as profiles/tsne_mi355x.json).

    python scripts/tsne_bench.py [--sizes 2048,8192,32768] [--dim 128] [--rounds 5] [--sklearn] [--frames 120]

Per N: sg_tsne_affinities, one sg_tsne_step (exaggeration 12) and one eager-torch dense step on the same GPU, in alternating rounds,
device events, median with min and max; the bytes of P a step streams per second as a fraction of the 6.29 TB/s a float4 copy
reaches on this chip (MI355X_MICROARCH: HBM3E, measured), or launches per second where the step is launch-bound (N = 2048); 1000
iterations end to end through traversal.tsne.  --sklearn adds scikit-learn's TSNE on the host (Barnes-Hut at every N up to 8192, exact
at N = 2048).  --frames F > 0 adds the traversal at the reference's settings (30 stops x 60 frames, 128^3, 1080 px) on the chairs
weights of tests/golden with a seeded 4096-code table, timing the embedding, the first F frames and their panels.  A run without a GPU
fails."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from shapegan_amd import ops  # noqa: E402
from shapegan_amd import traversal as T  # noqa: E402

HBM_COPY_BYTES_PER_S = 6.29e12


def clusters(n, d, k, seed):
    r = np.random.RandomState(seed)
    c = r.randn(k, d) * 4
    return torch.from_numpy((c[r.randint(0, k, n)] + r.randn(n, d)).astype(np.float32))


def timed(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def summary(samples):
    s = sorted(samples)
    return {"ms": round(s[len(s) // 2], 4), "ms_min": round(s[0], 4), "ms_max": round(s[-1], 4)}


def eager_step(y, P, vel, gains, exaggeration, momentum, lr):
    """The same iteration in eager torch, dense [N, N] temporaries."""
    d = y.unsqueeze(1) - y.unsqueeze(0)
    w = 1.0 / (1.0 + (d * d).sum(dim=2))
    w.fill_diagonal_(0.0)
    Z = w.sum()
    pq = (exaggeration * P - w / Z) * w
    grad = 4.0 * (pq.unsqueeze(2) * d).sum(dim=1)
    inc = vel * grad < 0
    gains.copy_(torch.where(inc, gains + 0.2, gains * 0.8).clamp_(min=0.01))
    vel.mul_(momentum).sub_(lr * gains * grad)
    y.add_(vel)


def bench_size(n, dim, rounds):
    x = clusters(n, dim, 10, 0).cuda()
    out = {"N": n, "D": dim}
    P, _, plogp = ops.tsne_affinities(x, 30.0)
    y = torch.randn(n, 2, device="cuda") * 1e-4
    vel, gains, grad = torch.zeros_like(y), torch.ones_like(y), torch.empty_like(y)
    lr = T.auto_learning_rate(n, 12.0)
    ours = lambda: ops.tsne_step(y, P, vel, gains, 12.0, 0.5, lr, grad=grad)      # noqa: E731
    ye, ve, ge = y.clone(), vel.clone(), gains.clone()
    eager = lambda: eager_step(ye, P, ve, ge, 12.0, 0.5, lr)      # noqa: E731
    aff = lambda: ops.tsne_affinities(x, 30.0)      # noqa: E731
    step_reps, eager_reps = (200 if n <= 8192 else 20), (20 if n <= 8192 else 3)
    for fn in (ours, eager, aff):
        fn()
    torch.cuda.synchronize()
    t_ours, t_eager, t_aff = [], [], []
    for _ in range(rounds):
        t_ours.append(timed(ours, step_reps))
        t_eager.append(timed(eager, eager_reps))
        t_aff.append(timed(aff, 1))
    out["affinities"] = summary(t_aff)
    out["step"] = summary(t_ours)
    out["eager_step"] = summary(t_eager)
    out["step_over_eager"] = round(out["step"]["ms"] / out["eager_step"]["ms"], 4)
    rate = 4.0 * n * n / (out["step"]["ms"] * 1e-3)
    out["step_P_bytes_per_s"] = rate
    out["step_fraction_of_hbm_copy_rate"] = round(rate / HBM_COPY_BYTES_PER_S, 4)
    out["step_launches_per_s"] = round(3.0 / (out["step"]["ms"] * 1e-3))
    del ye, ve, ge
    runs = []
    for _ in range(max(1, rounds // 2)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        emb, kl = T.tsne(x, iterations=1000, init="random", return_kl=True)
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) * 1e3)
    out["tsne_1000_iterations"] = summary(runs)
    out["tsne_final_kl"] = kl
    return out, x


def bench_sklearn(x, n, exact):
    from sklearn.manifold import TSNE
    t0 = time.perf_counter()
    model = TSNE(method="exact" if exact else "barnes_hut", init="random", random_state=0, perplexity=30.0, n_jobs=16).fit(x.cpu().numpy())
    return {"N": n, "method": "exact" if exact else "barnes_hut", "s": round(time.perf_counter() - t0, 2), "kl": float(model.kl_divergence_),
            "iterations": int(model.n_iter_)}


def bench_traversal(frames):
    import latent_fit_forms as LF
    net = LF.net_on("cuda", 5, 128, LF.chairs_state())
    codes = (torch.randn(4096, 128, generator=torch.Generator().manual_seed(0)) * 0.1).cuda()
    out = {"codes": 4096, "stops": 30, "transition_frames": 60, "resolution": 128, "size": 1080, "frames_timed": frames}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plan = T.plan_traversal(codes, None, 30, 60)
    torch.cuda.synchronize()
    out["plan_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    panel = T.MapPanel(plan["embedding"], T.label_colors(None, 4096), plan["frame_positions"], plan["stops"][:-1], size=1080, device="cuda")
    torch.cuda.synchronize()
    out["panel_static_s"] = round(time.perf_counter() - t0, 3)
    t0 = time.perf_counter()
    for _ in T.traversal_frames(net, plan["frame_codes"][:frames], voxel_resolution=128, size=1080):
        pass
    torch.cuda.synchronize()
    out["frames_s"] = round(time.perf_counter() - t0, 3)
    out["ms_per_frame"] = round(out["frames_s"] * 1e3 / frames, 2)
    t0 = time.perf_counter()
    for position in plan["frame_positions"][:frames]:
        panel.image(position)
    out["panels_s"] = round(time.perf_counter() - t0, 3)
    out["ms_per_panel"] = round(out["panels_s"] * 1e3 / frames, 2)
    out["projected_1800_frames_s"] = round(out["plan_s"] + out["panel_static_s"] + 1800 * (out["ms_per_frame"] + out["ms_per_panel"]) * 1e-3, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2048,8192,32768")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sklearn", action="store_true")
    ap.add_argument("--frames", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tsne_bench.py measures on the GPU; there is none")
    result = {"device": torch.cuda.get_device_name(0), "hbm_copy_bytes_per_s": HBM_COPY_BYTES_PER_S, "cases": [], "sklearn": []}
    for n in (int(s) for s in args.sizes.split(",")):
        case, x = bench_size(n, args.dim, args.rounds)
        result["cases"].append(case)
        if args.sklearn and n <= 8192:
            result["sklearn"].append(bench_sklearn(x, n, False))
            if n <= 2048:
                result["sklearn"].append(bench_sklearn(x, n, True))
        del x
        torch.cuda.empty_cache()
    if args.frames > 0:
        result["traversal"] = bench_traversal(args.frames)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
