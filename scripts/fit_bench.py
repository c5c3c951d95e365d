"""One latent-fit iteration (shapegan_amd/reconstruct.py, csrc/latent_fit.hip) on the GPU with the seeded chairs weights; prints one JSON line.

    python scripts/fit_bench.py [--iters 100] [--rounds 3]

Per case (64 shapes x 16 384 points, 1 024 shapes x 2 048 points; random points in the unit sphere's box, targets N(0, 0.1^2)) the time of
one iteration — loss, latent gradient and the Adam step of the codes — and the peak of torch.cuda.max_memory_allocated above the inputs for
  fused     the fused step (SDFNet.latent_loss_and_grad's kernel through ops.LatentFit, weights packed once)
  composed  the same from forward_segments and autograd with respect to the latent table (fused=False)
  eager     the baseline that never runs the code under test: an nn.Linear stack in eager torch on the same device, the latent rows
            gathered per point, autograd with respect to the table, torch.optim.Adam
Device events around `--iters` iterations (a tenth of them for the eager baseline) after a warm-up of the same shapes; both project
steps keep their per-fit constants (tile table / shape index, weight pack) outside the timed step; the three are timed alternately, `--rounds` times, and
the median round is reported with the spread.  The fused and the composed gradient are compared at the sizes timed.  No profiler here."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shapegan_amd import ops  # noqa: E402
from shapegan_amd.model.sdf_net import SDFNet  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "sdfnet_chairs_weights.npz")
CUTOFF, SIGMA, LR = 0.1, 0.01, 5e-3


def chairs_net(dev):
    z = np.load(GOLDEN)
    state = {k: torch.from_numpy(z[k]) for k in z.files}
    net = SDFNet(latent_code_size=state["layers1.0.weight"].shape[1] - 3, device=dev)
    net.load_state_dict(state)
    ops.L.bump_param_epoch()
    return net


def eager_forward(sd, points, latents):
    inp = torch.cat((points, latents), dim=1)
    x = inp
    for i in (0, 2, 4, 6):
        x = F.relu(F.linear(x, sd["layers1.%d.weight" % i], sd["layers1.%d.bias" % i]))
    x = torch.cat((x, inp), dim=1)
    for i in (0, 2, 4):
        x = F.relu(F.linear(x, sd["layers2.%d.weight" % i], sd["layers2.%d.bias" % i]))
    return torch.tanh(F.linear(x, sd["layers2.6.weight"], sd["layers2.6.bias"])).reshape(-1)


def timed(fn, iters):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def case(net, S, P, iters, rounds, dev):
    g = torch.Generator().manual_seed(S)
    points = (torch.rand(S * P, 3, generator=g) * 2 - 1).to(dev)
    sdf = (torch.randn(S * P, generator=g) * 0.1).to(dev)
    seg = (torch.arange(S + 1, dtype=torch.int64) * P).to(dev)
    L = net.latent_code_size
    z0 = (torch.randn(S, L, generator=g) * 0.1).to(dev)
    off = ops.check_segments(points, sdf, z0, seg)
    params = net._params()
    lib = ops._lib()
    fit = ops.LatentFit(net._pack_shapes, params, points, sdf, seg, off, CUTOFF)
    comp = ops.LatentFitComposed(net._pack_shapes, params, points, sdf, off, CUTOFF)

    def adam(z, grad, m, v, k):
        ops.check(lib.sg_adam_step(ops.ptr(z), ops.ptr(grad), ops.ptr(m), ops.ptr(v), z.numel(), LR, 0.9, 0.999, 1e-8, k, 1.0, ops.stream()),
                  "adam_step")

    state = {}

    def start(name):
        z = z0.clone()
        state[name] = [z, torch.zeros_like(z), torch.zeros_like(z), 0]

    def fused():
        st = state["fused"]
        st[3] += 1
        adam(st[0], fit.step(st[0], 0, 0, SIGMA)[1], st[1], st[2], st[3])

    def composed():
        st = state["composed"]
        st[3] += 1
        adam(st[0], comp.step(st[0], 0, 0, SIGMA)[1], st[1], st[2], st[3])

    sd = {k: v.detach() for k, v in net.state_dict().items()}
    sid = torch.arange(S, device=dev).repeat_interleave(P)
    tgt = sdf.clamp(-CUTOFF, CUTOFF)
    ze = z0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ze], lr=LR)

    def eager():
        opt.zero_grad(set_to_none=True)
        d = (eager_forward(sd, points, ze[sid]) - tgt).abs()
        (d.view(S, P).mean(dim=1).sum() + SIGMA * (ze * ze).mean(dim=1).sum()).backward()
        opt.step()

    # the results at the sizes timed: fused against composed
    lf, gf = fit.step(z0, 0, 0, SIGMA)
    lc, gc = comp.step(z0, 0, 0, SIGMA)
    agree = {"loss_max_abs_diff": float((lf - lc).abs().max()), "grad_max_abs_diff": float((gf - gc).abs().max()),
             "grad_mean_abs": float(gc.abs().mean())}
    del lf, gf, lc, gc
    steps = {"fused": fused, "composed": composed, "eager": eager}
    out = {"shapes": S, "points_per_shape": P, "iters": iters, "rounds": rounds, "agreement": agree}
    base = torch.cuda.memory_allocated()
    ms, peak = {k: [] for k in steps}, {}
    for name, fn in steps.items():      # warm-up of every shape timed, and the memory peak of one iteration
        start(name)
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[name] = int(torch.cuda.max_memory_allocated() - base)
    for _ in range(rounds):
        for name, fn in steps.items():
            ms[name].append(timed(fn, iters if name != "eager" else max(2, iters // 10)))
    for name in steps:
        out[name] = {"ms_per_iteration": round(float(np.median(ms[name])), 4), "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                     "peak_bytes_above_inputs": peak[name]}
    out["fused_over_composed"] = round(out["fused"]["ms_per_iteration"] / out["composed"]["ms_per_iteration"], 4)
    out["fused_over_eager"] = round(out["fused"]["ms_per_iteration"] / out["eager"]["ms_per_iteration"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="64x16384,1024x2048")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "fit_bench needs a GPU"
    dev = torch.device("cuda")
    net = chairs_net(dev)
    out = {"device": torch.cuda.get_device_properties(0).name, "cutoff": CUTOFF, "sigma": SIGMA, "cases": []}
    for spec in args.cases.split(","):
        S, P = (int(x) for x in spec.split("x"))
        out["cases"].append(case(net, S, P, args.iters, args.rounds, dev))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
