"""Sphere-tracer benchmark: render_image at the reference default (800 px, ssaa 2) with the chairs SDFNet, one JSON line.

    python scripts/render_bench.py [--reps 3] [--skip-baseline]

images_per_s for 1 and for 8 latent codes (one render_images call), SDFNet evaluations counted on the device and their rate,
the rate of the standalone forward (sg_sdfnet_fwd through SDFNet.forward_shapes) on as many points in the same run, launches per
image, and the baseline: the reference's host-driven march (a gather, SDFNet.evaluate_in_batches, clamp, scatter and two boolean
compactions per step, raymarching.py:104-124) restated on the same GPU with the same SDFNet and camera rays; it is timed for the camera-ray march alone (the shadow marches, normals and shading are left out), so the speed-up it gives
against the whole render is a lower bound.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from shapegan_amd.model.sdf_net import SDFNet  # noqa: E402
from shapegan_amd.rendering import raymarching as rm  # noqa: E402

SETTINGS = dict(radius=1.6, sdf_offset=-0.045, vertical_cutoff=1)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps, out


def host_march(net, z, points, dirs, clamp, threshold, offset, radius, shadow, cap):
    """The host-driven loop: per step gather, evaluate, clamp, scatter, drop hits and misses; stop below 2 rays."""
    idx = torch.arange(points.shape[0], device=points.device)
    mask = torch.zeros(points.shape[0], dtype=torch.bool, device=points.device)
    for _ in range(cap):
        sdf = net.evaluate_in_batches(points[idx], z, return_cpu_tensor=False) + offset
        sdf = sdf.clamp(-clamp, clamp)
        points[idx] += dirs[idx] * sdf.unsqueeze(1)
        hit = (sdf > 0) & (sdf < threshold)
        mask[idx[hit]] = True
        idx = idx[~hit]
        out = (points[idx, 1] > radius) if shadow else (points[idx].norm(dim=1) > radius)
        idx = idx[~out]
        if idx.shape[0] < 2:
            break
    mask[idx] = True
    return mask


def host_loop_render(net, z, res, ssaa):
    """Seconds of the host-driven camera-ray march of one image, from the same camera rays as the tracer."""
    W = res * ssaa
    dirs = torch.empty((W * W, 3), device="cuda")
    pos = torch.empty((W * W, 3), device="cuda")
    from shapegan_amd.lib import check, ptr, stream
    from shapegan_amd import ops
    import ctypes
    fwd = rm.camera_position / np.linalg.norm(rm.camera_position) * -1
    right = np.cross(fwd, np.array([0, 1, 0]))
    right /= np.linalg.norm(right)
    up = np.cross(fwd, right)
    up /= np.linalg.norm(up)
    focal = 1.0 / np.tan(np.arcsin(SETTINGS["radius"] / np.linalg.norm(rm.camera_position)))
    cam = (ctypes.c_double * 13)(*[float(v) for v in list(rm.camera_position) + list(right) + list(up) + list(fwd) + [focal]])
    status = torch.empty(W * W, dtype=torch.uint8, device="cuda")
    active = torch.empty(2 * W * W, dtype=torch.int32, device="cuda")
    counts = torch.zeros(3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    check(ops._lib().sg_raymarch_rays(cam, W, 1, SETTINGS["radius"], ptr(dirs), ptr(pos), ptr(status), ptr(active), ptr(counts),
                                      stream()), "rays")
    n = int(counts[0])
    idx = active[:n].long()
    p = pos[idx].clone()
    host_march(net, z, p, dirs[idx], 0.02, 0.0005, SETTINGS["sdf_offset"], SETTINGS["radius"], False, 1000)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-baseline", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    w = np.load(os.path.join(ROOT, "tests", "golden", "sdfnet_chairs_weights.npz"))
    net = SDFNet(device="cuda")
    net.load_state_dict({k: torch.from_numpy(w[k]) for k in w.files})
    g = np.load(os.path.join(ROOT, "tests", "golden", "raymarch_chairs.npz"))
    z8 = (torch.randn(8, 128, generator=torch.Generator().manual_seed(51)) * 0.5).cuda()
    z8[0] = torch.from_numpy(g["latents"][0]).cuda()
    res = {"resolution": 800, "ssaa": 2, **SETTINGS}

    def run(z):
        return rm._render(net, z, 800, 0.0005, SETTINGS["sdf_offset"], 1000, 2, SETTINGS["radius"], (0.8, 0.1, 0.1),
                          SETTINGS["vertical_cutoff"])
    for S in (1, 8):
        t, (_, st) = timed(lambda: run(z8[:S]), args.reps)
        res["images_per_s_%d" % S] = S / t
        res["seconds_per_call_%d" % S] = t
        res["evaluations_%d" % S] = st["evaluations"]
        res["evaluations_per_s_%d" % S] = st["evaluations"] / t
        res["launches_per_image_%d" % S] = st["launches"] / S
        res["march_steps_%d" % S] = [st["iterations"], st["shadow_iterations"]]
        res["hits_%d" % S] = st["hits"]
    # the standalone forward on as many points as the single-image render evaluates
    n = res["evaluations_1"]
    pts = (torch.rand((n, 3), generator=torch.Generator().manual_seed(1)) * 2 - 1).cuda()
    with torch.no_grad():
        tf, _ = timed(lambda: net.forward_shapes(pts, z8[:1], n), args.reps)
    res["fwd_evaluations_per_s"] = n / tf
    res["march_over_fwd_rate_1"] = res["evaluations_per_s_1"] / res["fwd_evaluations_per_s"]
    res["march_over_fwd_rate_8"] = res["evaluations_per_s_8"] / res["fwd_evaluations_per_s"]
    if not args.skip_baseline:
        tb = host_loop_render(net, z8[0], 800, 2)
        res["baseline_host_loop_primary_march_s"] = tb
        res["speedup_vs_host_loop_primary_only"] = tb / res["seconds_per_call_1"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
