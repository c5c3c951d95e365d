"""One iteration of the pose fit (shapegan_amd/reconstruct.py fit_codes_and_poses, csrc/latent_fit.hip) on the GPU with the seeded
chairs weights; prints one JSON line.

    python scripts/pose_fit_bench.py [--iters 100] [--rounds 3]

Per case (64 shapes x 16 384 points, 1 024 shapes x 2 048 points; random points in the unit sphere's box, targets N(0, 0.1^2), a
similarity pose per shape of 10 degrees, |t| = 0.05, s = 1.1) the time of one iteration — loss, the gradients with respect to the codes and
the seven pose parameters, and the Adam steps of both — and the peak of torch.cuda.max_memory_allocated above the inputs for
  fused       the fused step (ops.LatentPoseFit, weights packed once), the pose map and its backward in batched torch
  latent_fit  K7c's own iteration, the fused step of scripts/fit_bench.py without a pose: what the pose costs on top
  composed    forward_shapes on x = A q + t with autograd with respect to the points and the latent table, the pose map on top
  eager       the baseline that never runs the code under test: an nn.Linear stack in eager torch, torch.optim.Adam
The protocol is scripts/fit_bench.py's: device events around `--iters` iterations (a tenth of them for the eager baseline) after a warm-up
of the same shapes, per-fit constants outside the timed step, the forms timed alternately, `--rounds` times, the median round reported
with the range.  The fused and the composed gradients are compared at the sizes timed.  No profiler here."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fit_bench import CUTOFF, LR, SIGMA, chairs_net, eager_forward, timed  # noqa: E402
from shapegan_amd import ops  # noqa: E402
from shapegan_amd.reconstruct import pose_rows  # noqa: E402

POSE_LR = 1e-3


def posed(rows, sid, q):
    M = rows[:, :12].reshape(-1, 3, 4)[sid]
    return (M[:, :, :3] * q[:, None, :]).sum(dim=2) + M[:, :, 3], rows[:, 12][sid]


def case(net, S, P, iters, rounds, dev):
    g = torch.Generator().manual_seed(S)
    points = (torch.rand(S * P, 3, generator=g) * 2 - 1).to(dev)
    sdf = (torch.randn(S * P, generator=g) * 0.1).to(dev)
    seg = (torch.arange(S + 1, dtype=torch.int64) * P).to(dev)
    L = net.latent_code_size
    z0 = (torch.randn(S, L, generator=g) * 0.1).to(dev)
    axis = torch.randn(S, 3, generator=g)
    t = torch.randn(S, 3, generator=g)
    th0 = torch.cat([axis / axis.norm(dim=1, keepdim=True) * math.radians(10), t / t.norm(dim=1, keepdim=True) * 0.05,
                     torch.full((S, 1), math.log(1.1))], dim=1).to(dev)
    off = ops.check_segments(points, sdf, z0, seg)
    params = net._params()
    frozen = [p.detach() for p in params]
    lib = ops._lib()
    fit = ops.LatentPoseFit(net._pack_shapes, params, points, sdf, seg, off, CUTOFF)
    plain = ops.LatentFit(net._pack_shapes, params, points, sdf, seg, off, CUTOFF)
    sid = torch.arange(S, device=dev).repeat_interleave(P)

    def adam(p, grad, m, v, k, lr):
        ops.check(lib.sg_adam_step(ops.ptr(p), ops.ptr(grad), ops.ptr(m), ops.ptr(v), p.numel(), lr, 0.9, 0.999, 1e-8, k, 1.0, ops.stream()),
                  "adam_step")

    state = {}

    def start(name):
        z, th = z0.clone(), th0.clone()
        state[name] = [z, torch.zeros_like(z), torch.zeros_like(z), th, torch.zeros_like(th), torch.zeros_like(th), 0]

    def fused_grads(z, th):
        tt = th.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            rows = pose_rows(tt)
        loss, gz, grows = fit.step(z, rows.detach(), 0, 0, SIGMA)
        gth, = torch.autograd.grad(rows, tt, grows)
        return loss, gz, gth.contiguous()

    def composed_grads(z, th):
        zz = z.detach().clone().requires_grad_(True)
        tt = th.detach().clone().requires_grad_(True)
        with torch.enable_grad():
            x, ts = posed(pose_rows(tt), sid, points)
            # (forward_shapes' own Function with the weights detached, as ops.LatentFitComposed calls it: no weight gradients)
            out = ops.SDFNetShapes.apply(net._pack_shapes, x, zz, P, None, None, None, True, *frozen)
            d = (out - (ts * sdf).clamp(-CUTOFF, CUTOFF)).abs()
            loss = d.view(S, P).mean(dim=1)
            gz, gth = torch.autograd.grad(loss.sum() + SIGMA * (zz * zz).mean(dim=1).sum(), (zz, tt))
        return loss.detach(), gz.contiguous(), gth.contiguous()

    def project_step(name, grads):
        def fn():
            st = state[name]
            st[6] += 1
            _, gz, gth = grads(st[0], st[3])
            adam(st[0], gz, st[1], st[2], st[6], LR)
            adam(st[3], gth, st[4], st[5], st[6], POSE_LR)
        return fn

    def latent_fit():
        st = state["latent_fit"]
        st[6] += 1
        adam(st[0], plain.step(st[0], 0, 0, SIGMA)[1], st[1], st[2], st[6], LR)

    sd = {k: v.detach() for k, v in net.state_dict().items()}
    ze, te = z0.clone().requires_grad_(True), th0.clone().requires_grad_(True)
    opt = torch.optim.Adam([{"params": [ze], "lr": LR}, {"params": [te], "lr": POSE_LR}])

    def eager():
        opt.zero_grad(set_to_none=True)
        x, ts = posed(pose_rows(te), sid, points)
        d = (eager_forward(sd, x, ze[sid]) - (ts * sdf).clamp(-CUTOFF, CUTOFF)).abs()
        (d.view(S, P).mean(dim=1).sum() + SIGMA * (ze * ze).mean(dim=1).sum()).backward()
        opt.step()

    # the results at the sizes timed: fused against composed
    lf, gf, tf = fused_grads(z0, th0)
    lc, gc, tc = composed_grads(z0, th0)
    agree = {"loss_max_abs_diff": float((lf - lc).abs().max()), "grad_z_max_abs_diff": float((gf - gc).abs().max()),
             "grad_z_mean_abs": float(gc.abs().mean()), "grad_theta_max_abs_diff": float((tf - tc).abs().max()),
             "grad_theta_mean_abs": float(tc.abs().mean())}
    del lf, gf, tf, lc, gc, tc
    steps = {"fused": project_step("fused", fused_grads), "latent_fit": latent_fit, "composed": project_step("composed", composed_grads),
             "eager": eager}
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
    for other in ("latent_fit", "composed", "eager"):
        out["fused_over_" + other] = round(out["fused"]["ms_per_iteration"] / out[other]["ms_per_iteration"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="64x16384,1024x2048")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pose_fit_bench needs a GPU"
    dev = torch.device("cuda")
    net = chairs_net(dev)
    out = {"device": torch.cuda.get_device_properties(0).name, "cutoff": CUTOFF, "sigma": SIGMA, "cases": []}
    for spec in args.cases.split(","):
        S, P = (int(x) for x in spec.split("x"))
        out["cases"].append(case(net, S, P, args.iters, args.rounds, dev))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
