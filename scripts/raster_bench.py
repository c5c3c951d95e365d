"""Mesh-renderer benchmark: MeshRenderer at the reference default (800 px, ssaa 2, shadow map 1024), one JSON line.

    python scripts/raster_bench.py [--reps 5]

Three workloads: one and 64 generator-sized 32^3 SDF grids (render_voxels: one pass over the batch), and one 128^3 chair of the
SDFNet of tests/golden/sdfnet_chairs_weights.npz (the grid get_mesh meshes, drawn at set_mesh's model size).  Each reports
milliseconds per image and images per second end to end, and the split meshing / setup + bin / visibility / shade: the stages are run
one after the other with a device synchronise behind each, light and camera pass together, so the split adds up to a little more than
the end-to-end time (which synchronises once).  The same run sphere-traces the same chair with raymarching.render_images at the same
resolution.  Times are host clocks around work that ends in a synchronise, after one warm-up of every shape.
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

from shapegan_amd import mesh as M  # noqa: E402
from shapegan_amd.model.sdf_net import SDFNet  # noqa: E402
from shapegan_amd.rendering import MeshRenderer, raster  # noqa: E402
from shapegan_amd.rendering import raymarching as rm  # noqa: E402
from shapegan_amd.rendering.math import get_camera_transform  # noqa: E402

DEV = "cuda"


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps, out


def blob_grids(S, R=32):
    """Seeded stand-ins for generator samples: a ball with smooth bumps, values in (-1, 1) like the generator's tanh output."""
    g = torch.Generator().manual_seed(7)
    ax = (torch.arange(R, dtype=torch.float32) + 1) * (2.0 / R) - 1
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    out = []
    for _ in range(S):
        a = torch.rand(6, generator=g)
        r = 0.45 + 0.2 * a[0] + 0.12 * torch.sin(6 * a[1] * x + 5 * a[2]) * torch.cos(5 * a[3] * y) + 0.1 * torch.sin(7 * a[4] * z + a[5])
        out.append(torch.tanh(2 * ((x * x + 1.4 * y * y + z * z).sqrt() - r)))
    return torch.stack(out).to(DEV)


def staged(viewer, make_soup, reps):
    """Per-stage seconds of one render: meshing, setup + bin, visibility, shade (+ resolve), both passes together."""
    light_vp = get_camera_transform(6, viewer.rotation[0], 50, project=True)
    camera_vp = get_camera_transform(viewer.model_size * 2, viewer.rotation[0], viewer.rotation[1], project=True)
    params = raster.shading_params(camera_vp, light_vp, viewer.model_color, viewer.background_color)
    n, N = viewer.size * viewer.ssaa, viewer.shadow_size
    t_mesh, soup = timed(make_soup, reps)

    def bins():
        return (raster.bin_tiles(soup, raster.setup(soup, light_vp, N, N, cull_back=False)),
                raster.bin_tiles(soup, raster.setup(soup, camera_vp, n, n, cull_back=True, ground=True)))
    t_bin, (light, cam) = timed(bins, reps)
    t_vis, _ = timed(lambda: (raster.visibility(soup, light, shadow=True), raster.visibility(soup, cam)), reps)
    t_shade, _ = timed(lambda: raster.resolve(raster.shade(soup, cam, light.depth, cam.ground, params), viewer.ssaa), reps)
    return {"meshing_ms": 1e3 * t_mesh, "setup_bin_ms": 1e3 * t_bin, "visibility_ms": 1e3 * t_vis, "shade_ms": 1e3 * t_shade,
            "triangles": int(soup.positions.shape[0]), "tile_list_entries": [int(light.lists.shape[0]), int(cam.lists.shape[0])],
            "non_empty_tiles": [light.nactive, cam.nactive], "dropped": [int(light.dropped.sum()), int(cam.dropped.sum())]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"size": 800, "ssaa": 2, "shadow_size": 1024}
    viewer = MeshRenderer(size=800, ssaa=2, shadow_size=1024)
    grids = blob_grids(64)          # 64 = the trainer's batch
    for S in (1, len(grids)):
        viewer.model_size = 1.4
        t, images = timed(lambda: viewer.render_voxels(grids[:S], return_tensor=True), args.reps)
        entry = {"ms_per_image": 1e3 * t / S, "images_per_s": S / t}
        entry.update(staged(viewer, lambda: raster.pack(viewer._mesh_voxels(grids[:S], True, 0)), args.reps))
        for k in ("meshing_ms", "setup_bin_ms", "visibility_ms", "shade_ms"):
            entry[k + "_per_image"] = entry[k] / S
        entry["model_pixels_share"] = float((images[..., 0] != images[..., 1]).float().mean())
        res["voxels32_x%d" % S] = entry

    w = np.load(os.path.join(ROOT, "tests", "golden", "sdfnet_chairs_weights.npz"))
    net = SDFNet(device=DEV)
    net.load_state_dict({k: torch.from_numpy(w[k]) for k in w.files})
    z = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "raymarch_chairs.npz"))["latents"][0]).to(DEV).reshape(1, -1)

    def chair_soup():
        with torch.no_grad():
            g = net.voxel_grids(z, 128, sphere_only=True)
        return raster.pack(M.marching_cubes(g, level=0, spacing=2.0 / 128, origin=-1.0, pad=True, pad_value=1.0))

    def chair():
        viewer.model_size = 1.08
        return viewer._draw(chair_soup())
    t, image = timed(chair, args.reps)
    entry = {"ms_per_image": 1e3 * t, "images_per_s": 1 / t}
    entry.update(staged(viewer, chair_soup, args.reps))
    entry["model_pixels_share"] = float((image[..., 0] != image[..., 1]).float().mean())
    res["chair128"] = entry
    t, _ = timed(lambda: rm.render_images(net, z, resolution=800, ssaa=2, return_tensor=True), args.reps)
    res["chair_sphere_traced"] = {"ms_per_image": 1e3 * t, "images_per_s": 1 / t}
    res["rasterised_over_sphere_traced_time"] = res["chair128"]["ms_per_image"] / (1e3 * t)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
