"""Sphere-traced images of SDFNet shapes (rendering/raymarching.py), on the device.

render_image keeps the reference's signature and output.  The march is csrc/raymarch.hip: one launch per step over a compacted
list of active rays, the SDFNet forward fused with the step, no host round trip inside a step; the host reads the active counts
once per MARCH_CHUNK steps to stop.  render_images renders a batch of latent codes in one march; every image equals its render
alone, bit for bit.  One deliberate difference: where no ray hits the shape the reference fails (np.min of an empty array);
here the image is white.
"""
import ctypes
import math
import os

import numpy as np
import torch
from PIL import Image

from .. import ops
from ..lib import check, f32c, ptr, stream
from ..util import crop_image, ensure_directory
from .math import get_camera_transform

BATCH_SIZE = 100000
MARCH_CHUNK = 16      # march steps enqueued between two reads of the active counts


def get_default_coordinates():
    camera_transform = get_camera_transform(2.2, 147, 20)
    camera_position = np.matmul(np.linalg.inv(camera_transform), np.array([0, 0, 0, 1]))[:3]
    light_matrix = get_camera_transform(6, 164, 50)
    light_position = np.matmul(np.linalg.inv(light_matrix), np.array([0, 0, 0, 1]))[:3]
    return camera_position, light_position


camera_position, light_position = get_default_coordinates()


def get_normals(sdf_net, points, latent_code):
    """Normalised SDF gradients at points [N,3] (raymarching.py:25-34)."""
    result = torch.zeros((points.shape[0], 3), device=points.device)
    for begin in range(0, points.shape[0], BATCH_SIZE):
        result[begin:begin + BATCH_SIZE, :] = sdf_net.get_normals(latent_code, points[begin:begin + BATCH_SIZE, :])
    return result


def _doubles(values):
    values = [float(v) for v in values]
    return (ctypes.c_double * len(values))(*values)


def _march(lib, packed, zb1, zb5, pos, dir, dir_period, status, active, counts, seg_off, nseg, nshapes, cap, clamp, threshold,
           sdf_offset, radius0, radius1, shadow, evals, stats):
    """Steps until every segment is finished or `cap` steps ran, then marks the rays left as hits.  Returns the step count."""
    nrays = status.numel()
    it, bound = 0, nrays
    counts3 = counts.view(3, nseg)
    while it < cap and bound > 0:
        k = min(MARCH_CHUNK, cap - it)
        check(lib.sg_raymarch_steps(ptr(packed), ptr(zb1), ptr(zb5), ptr(pos), ptr(dir), dir_period, ptr(status), ptr(active), nrays,
                                    ptr(counts), ptr(seg_off), nseg, nshapes, bound, it, k, clamp, threshold, sdf_offset, radius0,
                                    radius1, shadow, ptr(evals), stream()), "raymarch_steps")
        it += k
        stats["launches"] += k
        c = counts3[it % 3].cpu()
        bound = int(c.sum())        # the counts only fall: a bound for the launches of the next chunk
        if bool((c < 2).all()):
            break
    check(lib.sg_raymarch_finish(ptr(status), ptr(active), nrays, ptr(counts), ptr(seg_off), nseg, it, stream()), "raymarch_finish")
    stats["launches"] += 1
    return it


NORMALS = ("autograd", "fused")


def _render(sdf_net, latent_codes, resolution, threshold, sdf_offset, iterations, ssaa, radius, color, vertical_cutoff,
            normals="autograd"):
    """Device uint8 images [S, W, W, 3] (W = resolution * ssaa) before crop and resize, and a dict of counters."""
    if normals not in NORMALS:
        raise ValueError("normals must be one of %s, got %r" % (NORMALS, normals))
    z = f32c(latent_codes.detach().reshape(-1, sdf_net.latent_code_size))
    S = z.shape[0]
    if S > 128:
        raise ValueError("render_images: at most 128 latent codes per call")
    dev = z.device
    W = resolution * ssaa
    M = W * W
    lib = ops._lib()
    stats = {"launches": 0, "iterations": 0, "shadow_iterations": 0}
    packed, zb1, zb5 = sdf_net._pack_shapes.get_with_fold(sdf_net._params(), z)
    stats["launches"] += 1
    evals = torch.zeros(1, dtype=torch.int64, device=dev)

    # camera rays (raymarching.py:65-102), float64 camera basis as the reference computes it
    camera_forward = camera_position / np.linalg.norm(camera_position) * -1
    camera_distance = np.linalg.norm(camera_position).item()
    up = np.array([0, 1, 0])
    camera_right = np.cross(camera_forward, up)
    camera_right /= np.linalg.norm(camera_right)
    camera_up = np.cross(camera_forward, camera_right)
    camera_up /= np.linalg.norm(camera_up)
    focal_distance = 1.0 / math.tan(math.asin(radius / camera_distance))
    cam = _doubles(list(camera_position) + list(camera_right) + list(camera_up) + list(camera_forward) + [focal_distance])
    dirs = torch.empty((M, 3), dtype=torch.float32, device=dev)
    pos = torch.empty((S * M, 3), dtype=torch.float32, device=dev)
    status = torch.empty(S * M, dtype=torch.uint8, device=dev)
    active = torch.empty(2 * S * M, dtype=torch.int32, device=dev)
    counts = torch.zeros(3 * S, dtype=torch.int32, device=dev)
    seg = torch.arange(S + 1, dtype=torch.int64, device=dev) * M
    check(lib.sg_raymarch_rays(cam, W, S, float(radius), ptr(dirs), ptr(pos), ptr(status), ptr(active), ptr(counts), stream()),
          "raymarch_rays")
    stats["launches"] += 1
    stats["iterations"] = _march(lib, packed, zb1, zb5, pos, dirs, M, status, active, counts, seg, S, S, iterations, 0.02,
                                 float(threshold), float(sdf_offset), float(radius), float(radius), 0, evals, stats)

    # hits, ground plane, ground rays (raymarching.py:126-130, :155-163)
    ws = torch.empty(max(1, lib.sg_raymarch_workspace_bytes(M, S)), dtype=torch.uint8, device=dev)
    ground = torch.empty(S, dtype=torch.float32, device=dev)
    offs = torch.empty((2, S + 1), dtype=torch.int64, device=dev)
    use_cut = vertical_cutoff is not None
    check(lib.sg_raymarch_classify(ptr(status), ptr(pos), ptr(dirs), M, S, int(use_cut), float(vertical_cutoff if use_cut else 0.0),
                                   ptr(ground), ptr(offs[0]), ptr(offs[1]), ptr(ws), ws.numel(), stream()), "raymarch_classify")
    stats["launches"] += 4
    offs_h = offs.cpu()
    H, G = int(offs_h[0, S]), int(offs_h[1, S])
    NS = max(H + G, 1)
    hit_pos = torch.empty((max(H, 1), 3), dtype=torch.float32, device=dev)
    hit_sid = torch.empty(max(H, 1), dtype=torch.int32, device=dev)
    slot = torch.empty(S * M, dtype=torch.int32, device=dev)
    spos = torch.empty((NS, 3), dtype=torch.float32, device=dev)
    sdir = torch.empty((NS, 3), dtype=torch.float32, device=dev)
    sstatus = torch.zeros(NS, dtype=torch.uint8, device=dev)
    sactive = torch.empty(2 * NS, dtype=torch.int32, device=dev)
    scounts = torch.empty(6 * S, dtype=torch.int32, device=dev)
    sseg = torch.empty(2 * S + 1, dtype=torch.int64, device=dev)
    light = _doubles(light_position)
    check(lib.sg_raymarch_emit(ptr(status), ptr(pos), ptr(dirs), M, S, ptr(ground), ptr(offs[0]), ptr(offs[1]), light, ptr(hit_pos),
                               ptr(hit_sid), ptr(slot), ptr(spos), ptr(sdir), ptr(sactive), ptr(scounts), ptr(sseg), ptr(ws),
                               ws.numel(), stream()), "raymarch_emit")
    stats["launches"] += 1

    # normals: d sdf / d p of every hit in one forward_segments + backward (raymarching.py:130, model/sdf_net.py:118-128)
    # ("fused": the same gradient from sg_sdfnet_project, which keeps no activation image: 28 B per hit instead of 14.8 KB)
    grad = torch.zeros((max(H, 1), 3), dtype=torch.float32, device=dev)
    if H > 0 and normals == "fused":
        proj = ops.SurfaceProjector(sdf_net._pack_shapes, sdf_net._params(), z)
        _, _, grad = proj.run(hit_pos[:H], offs_h[0].numpy(), offs[0], iterations=0)
        stats["launches"] += 1
    elif H > 0:
        pts = hit_pos[:H].detach().clone().requires_grad_(True)
        with torch.enable_grad():
            sdf = sdf_net.forward_segments(pts, z, hit_sid[:H], offs[0])
            sdf.backward(torch.ones_like(sdf))
        grad = pts.grad

    # both get_shadows calls in one march (raymarching.py:136, :165): hits with the caller's radius, ground points with 1.0
    if H + G > 0:
        stats["shadow_iterations"] = _march(lib, packed, zb1, zb5, spos, sdir, 0, sstatus, sactive, scounts, sseg, 2 * S, S, 200, 0.1,
                                            0.001, float(sdf_offset), float(radius), 1.0, 1, evals, stats)

    image = torch.empty((S, W, W, 3), dtype=torch.uint8, device=dev)
    check(lib.sg_raymarch_shade(ptr(slot), ptr(hit_pos), ptr(grad), ptr(sstatus), ptr(dirs), M, S, H, light, _doubles(color),
                                ptr(image), stream()), "raymarch_shade")
    stats["launches"] += 1
    stats.update(hits=H, ground_rays=G, evaluations=int(evals.item()), status=status, pos=pos, hit_pos=hit_pos[:H],
                 hit_offsets=offs_h[0], ground=ground, shadows=sstatus[:H + G])
    return image, stats


def _to_pil(pixels, resolution, ssaa, crop):
    pixels = pixels.cpu().numpy()
    if crop:
        pixels = crop_image(pixels, background=255)   # (255 exactly where the reference's float image is 1)
    image = Image.fromarray(np.ascontiguousarray(pixels), 'RGB')
    if ssaa != 1:
        image = image.resize((resolution, resolution), Image.LANCZOS)
    return image


def render_images(sdf_net, latent_codes, resolution=800, threshold=0.0005, sdf_offset=0, iterations=1000, ssaa=2, radius=1.0,
                  crop=False, color=(0.8, 0.1, 0.1), vertical_cutoff=None, return_tensor=False, normals="autograd"):
    """render_image for every row of latent_codes [S,L] (S <= 128) in one march: a list of PIL images, or with return_tensor the
    device uint8 images [S, R ssaa, R ssaa, 3] before crop and resize.  normals: "autograd" — the hits' normals through
    forward_segments and its backward, as the reference takes them — or "fused": SDFNet.sdf_and_gradient's kernel, the same gradient
    without the activation images of the training path."""
    image, _ = _render(sdf_net, latent_codes, resolution, threshold, sdf_offset, iterations, ssaa, radius, color, vertical_cutoff,
                       normals=normals)
    if return_tensor:
        return image
    return [_to_pil(image[s], resolution, ssaa, crop) for s in range(image.shape[0])]


def render_image(sdf_net, latent_code, resolution=800, threshold=0.0005, sdf_offset=0, iterations=1000, ssaa=2, radius=1.0,
                 crop=False, color=(0.8, 0.1, 0.1), vertical_cutoff=None, normals="autograd"):
    """raymarching.py:63-182: a PIL image of resolution x resolution (ssaa x ssaa supersampled, LANCZOS-downsampled)."""
    return render_images(sdf_net, latent_code.reshape(1, -1), resolution=resolution, threshold=threshold, sdf_offset=sdf_offset,
                         iterations=iterations, ssaa=ssaa, radius=radius, crop=crop, color=color,
                         vertical_cutoff=vertical_cutoff, normals=normals)[0]


def get_shadows(sdf_net, points, light_position, latent_code, threshold=0.001, sdf_offset=0, radius=1.0):
    """1 where the ray from points [N,3] (numpy) toward light_position is blocked, else 0 (raymarching.py:37-61): float32 numpy."""
    ray_directions = light_position[np.newaxis, :] - points
    ray_directions /= np.linalg.norm(ray_directions, axis=1)[:, np.newaxis]
    n = points.shape[0]
    dev = sdf_net.device
    if n == 0:
        return np.zeros(0, dtype=np.float32)
    d = torch.tensor(ray_directions, device=dev, dtype=torch.float32)
    p = torch.tensor(points, device=dev, dtype=torch.float32)
    p += d * 0.1
    z = f32c(latent_code.detach().reshape(1, -1))
    packed, zb1, zb5 = sdf_net._pack_shapes.get_with_fold(sdf_net._params(), z)
    status = torch.zeros(n, dtype=torch.uint8, device=dev)
    active = torch.empty(2 * n, dtype=torch.int32, device=dev)
    active[:n] = torch.arange(n, dtype=torch.int32, device=dev)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    counts[0] = n
    seg = torch.tensor([0, n], dtype=torch.int64, device=dev)
    evals = torch.zeros(1, dtype=torch.int64, device=dev)
    stats = {"launches": 0}
    _march(ops._lib(), packed, zb1, zb5, p.contiguous(), d.contiguous(), 0, status, active, counts, seg, 1, 1, 200, 0.1,
           float(threshold), float(sdf_offset), float(radius), float(radius), 1, evals, stats)
    return status.cpu().numpy().astype(np.float32)


def render_image_for_index(sdf_net, latent_codes, index, crop=False, resolution=800):
    ensure_directory('screenshots')
    FILENAME = 'screenshots/raymarching-examples/image-{:d}-{:d}.png'
    filename = FILENAME.format(index, resolution)
    if os.path.isfile(filename):
        return Image.open(filename)
    img = render_image(sdf_net, latent_codes[index], resolution=resolution, crop=crop)
    img.save(filename)
    return img
