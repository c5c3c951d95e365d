"""SDFNet value + point gradient, projection onto the level set, refined meshes and the renderer's normals on the GPU with the chairs
weights (csrc/sdfnet_project.hip, shapegan_amd/surface.py); prints one JSON line.

    python scripts/surface_bench.py [--iters 10] [--rounds 3] [--skip-render]

(a) value + gradient at 8 x 131 072 points (codes 0.1 randn, L = 128, points uniform in the cube): time per evaluation and the peak of
    torch.cuda.max_memory_allocated above the inputs for
      fused     SDFNet.sdf_and_gradient's kernel through a kept ops.SurfaceProjector (weights packed and codes folded once)
      composed  forward_shapes with grad enabled and autograd with respect to the points: the code get_normals runs
      eager     the baseline that never runs the code under test: an nn.Linear stack in eager torch, autograd w.r.t. the points
(b) project_to_level_set with 5 iterations at the same size (six evaluations in one launch) against five composed rounds in a host loop
    (five evaluations, the update in torch).
(c) refine_meshes of one 128^3 and of eight 64^3 chairs (3 iterations, cell diagonal), with its stats.
(d) render_image at 800 px / ssaa 2 with normals="autograd" and normals="fused".
Device events around `--iters` calls after a warm-up of the same shapes; the forms of a measurement are timed alternately, `--rounds`
times, and the median round is reported with its minimum and maximum.  No profiler here."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shapegan_amd import ops  # noqa: E402
from shapegan_amd.model.sdf_net import SDFNet  # noqa: E402
from shapegan_amd.reconstruct import reconstruct_meshes  # noqa: E402
from shapegan_amd.rendering import raymarching  # noqa: E402
from shapegan_amd.surface import cell_diagonal, refine_meshes  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
S, P = 8, 131072
MAX_STEP = 0.1


def chairs_net(dev):
    z = np.load(os.path.join(GOLDEN, "sdfnet_chairs_weights.npz"))
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


def measure(forms, iters, rounds):
    """forms: {name: (fn, iteration divisor)} -> {name: {ms, ms_min, ms_max, peak_bytes_above_inputs}}"""
    base = torch.cuda.memory_allocated()
    ms, peak = {k: [] for k in forms}, {}
    for name, (fn, _) in forms.items():
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        peak[name] = int(torch.cuda.max_memory_allocated() - base)
    for _ in range(rounds):
        for name, (fn, div) in forms.items():
            ms[name].append(timed(fn, max(2, iters // div)))
    return {name: {"ms": round(float(np.median(ms[name])), 4), "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                   "peak_bytes_above_inputs": peak[name]} for name in forms}


def newton_update(x, f, g, level, max_step):
    n2 = (g * g).sum(dim=1)
    t = (f - level) / n2
    s = t.unsqueeze(1) * g
    length = t.abs() * n2.sqrt()
    s = s * torch.where(length > max_step, max_step / length, torch.ones_like(length)).unsqueeze(1)
    s = torch.where(((n2 > 0) & torch.isfinite(s).all(dim=1)).unsqueeze(1), s, torch.zeros_like(s))
    return x - s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-render", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "surface_bench needs a GPU"
    dev = torch.device("cuda")
    net = chairs_net(dev)
    g = torch.Generator().manual_seed(7)
    points = (torch.rand(S * P, 3, generator=g) * 2 - 1).to(dev)
    z = (torch.randn(S, net.latent_code_size, generator=g) * 0.1).to(dev)
    seg = (torch.arange(S + 1, dtype=torch.int64) * P).to(dev)
    off = seg.cpu().numpy()
    sd = {k: v.detach() for k, v in net.state_dict().items()}
    ones = torch.ones(S * P, device=dev)
    proj = net.surface_projector(z)
    out = {"device": torch.cuda.get_device_properties(0).name, "shapes": S, "points_per_shape": P, "iters": args.iters, "rounds": args.rounds}

    def composed_eval(x):
        p = x.detach().requires_grad_(True)
        with torch.enable_grad():
            sdf = net.forward_shapes(p, z, P)
            sdf.backward(ones)
        return sdf.detach(), p.grad

    def eager_eval(x):
        p = x.detach().requires_grad_(True)
        with torch.enable_grad():
            sdf = eager_forward(sd, p, z.repeat_interleave(P, dim=0))
            sdf.backward(ones)
        return sdf.detach(), p.grad

    # ---- (a) value + gradient
    fa, ga = proj.run(points, off, seg, iterations=0)[1:]
    fc, gc = composed_eval(points)
    agree = {"value_max_abs_diff": float((fa - fc).abs().max()), "grad_max_abs_diff": float((ga - gc).abs().max()),
             "grad_mean_norm": float(gc.norm(dim=1).mean())}
    del fa, ga, fc, gc
    a = measure({"fused": (lambda: proj.run(points, off, seg, iterations=0), 1), "composed": (lambda: composed_eval(points), 1),
                 "eager": (lambda: eager_eval(points), 3)}, args.iters, args.rounds)
    a["agreement"] = agree
    a["fused_over_composed_time"] = round(a["fused"]["ms"] / a["composed"]["ms"], 4)
    a["composed_round_spread_ms"] = round(a["composed"]["ms_max"] - a["composed"]["ms_min"], 4)
    a["fused_over_composed_memory"] = round(a["fused"]["peak_bytes_above_inputs"] / max(1, a["composed"]["peak_bytes_above_inputs"]), 6)
    out["value_and_gradient"] = a

    # ---- (b) five Newton iterations
    def composed_project():
        x = points
        for _ in range(5):
            f, gr = composed_eval(x)
            x = newton_update(x, f, gr, 0.0, MAX_STEP)
        return x

    b = measure({"fused": (lambda: proj.run(points, off, seg, iterations=5, max_step=MAX_STEP), 3), "composed": (composed_project, 3)},
                args.iters, args.rounds)
    xf = proj.run(points, off, seg, iterations=5, max_step=MAX_STEP)[0]
    b["positions_max_abs_diff"] = float((xf - composed_project()).abs().max())
    b["fused_over_composed_time"] = round(b["fused"]["ms"] / b["composed"]["ms"], 4)
    del xf
    out["project_5_iterations"] = b

    # ---- (c) refined meshes
    meshes = {}
    for name, codes, R in (("1x128", z[:1], 128), ("8x64", z, 64)):
        batch = reconstruct_meshes(net, codes, R)
        refine_meshes(net, codes, batch, iterations=3, max_move=cell_diagonal(R))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, stats = refine_meshes(net, codes, batch, iterations=3, max_move=cell_diagonal(R))
        torch.cuda.synchronize()
        meshes[name] = {"ms": round((time.perf_counter() - t0) * 1e3, 3), "stats": stats}
    out["refine_meshes"] = meshes

    # ---- (d) the renderer's normals
    if not args.skip_render:
        code = torch.from_numpy(np.load(os.path.join(GOLDEN, "raymarch_chairs.npz"))["latents"][0]).to(dev)
        kw = dict(radius=1.6, sdf_offset=-0.045, vertical_cutoff=1)
        d = measure({"autograd": (lambda: raymarching.render_image(net, code, normals="autograd", **kw), 5),
                     "fused": (lambda: raymarching.render_image(net, code, normals="fused", **kw), 5)}, args.iters, args.rounds)
        ia = np.asarray(raymarching.render_image(net, code, normals="autograd", **kw)).astype(np.int32)
        ib = np.asarray(raymarching.render_image(net, code, normals="fused", **kw)).astype(np.int32)
        d["max_pixel_difference"] = int(np.abs(ia - ib).max())
        out["render_800px_ssaa2"] = d
    print(json.dumps(out))


if __name__ == "__main__":
    main()
