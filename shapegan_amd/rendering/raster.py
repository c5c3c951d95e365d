"""The stages of the tiled rasteriser (csrc/raster.hip, K14 of include/shapegan_hip.h), one function per entry point.

    soup = pack(batch, smooth)                        # vertices[faces] of a MeshBatch: plumbing, done with torch
    light = draw_view(soup, light_vp, N, N, cull_back=False, shadow=True)
    cam = draw_view(soup, camera_vp, W, H, cull_back=True, ground=True)
    image = shade(soup, cam, light.depth, cam.ground, shading_params(camera_vp, light_vp, albedo, background))

GPU tensors run the HIP kernels, CPU tensors the twin.  Integer scratch (tile counts, offsets, lists, cursors) is `torch.empty` of an
integer dtype, never `lib.workspace`.  draw_view reads two totals back from the device once per view, between the scan and the fill,
to size the triangle lists and the visibility launch (like marching_cubes): rendering is not meant for graph capture.
"""
import ctypes

import numpy as np
import torch

from .. import lib as L
from ..lib import check, ptr, stream
from .math import PROJECTION_MATRIX

TILE = 16                     # SG_RS_TILE
CHUNK = 256                   # SG_RS_CHUNK: records per LDS stage of the visibility kernel
DROPPED = 15                  # flags & DROPPED: the triangle was dropped (near distance, guard box, zero area, back face)
# the near distance of the projection every view here uses: P[2][3] / (P[2][2] - 1) = 2fn/(f-n) / (2f/(f-n))
NEAR = float(PROJECTION_MATRIX[2, 3] / (PROJECTION_MATRIX[2, 2] - 1.0))


def _doubles(values):
    values = [float(v) for v in np.asarray(values, dtype=np.float64).reshape(-1)]
    return (ctypes.c_double * len(values))(*values)


class Soup(object):
    """S triangle soups packed on one device: positions [T,3,3] fp32, normals [T,3,3] fp32 or None (flat), tri_offsets [S+1] int64."""

    def __init__(self, positions, normals, tri_offsets):
        self.positions = L.f32c(positions).reshape(-1, 3, 3)
        self.normals = None if normals is None else L.f32c(normals).reshape(-1, 3, 3)
        self.tri_offsets = tri_offsets.to(torch.int64).contiguous()
        if self.normals is not None and self.normals.shape != self.positions.shape:
            raise ValueError("Soup: normals %s do not match positions %s" % (tuple(self.normals.shape), tuple(self.positions.shape)))

    def __len__(self):
        return self.tri_offsets.shape[0] - 1

    @property
    def device(self):
        return self.positions.device


def pack(batch, smooth=False):
    """MeshBatch -> Soup.  K12 meshes face outward and carry outward vertex normals: they are used as they are (the reference's `* -1`
    on smooth normals undoes skimage's inward convention, which this project does not have)."""
    S = len(batch)
    counts = batch.triangle_counts()
    shape_of = torch.repeat_interleave(torch.arange(S, device=counts.device), counts)
    faces = batch.faces + batch.vert_offsets[shape_of].unsqueeze(1)
    normals = batch.normals[faces] if smooth else None
    return Soup(batch.vertices[faces], normals, batch.tri_offsets)


class View(object):
    """Everything one pass leaves behind, stage by stage."""
    __slots__ = ("width", "height", "ntx", "nty", "recs", "flags", "clip", "dropped", "ground", "tile_counts", "tile_offsets",
                 "active", "nactive", "lists", "id", "depth")


def setup(soup, vp, width, height, cull_back, ground=False, clip=False):
    S, T, dev = len(soup), soup.positions.shape[0], soup.device
    v = View()
    v.width, v.height = int(width), int(height)
    v.ntx, v.nty = (v.width + TILE - 1) // TILE, (v.height + TILE - 1) // TILE
    v.recs = torch.empty((T, 16), dtype=torch.int32, device=dev)
    v.flags = torch.empty(T, dtype=torch.int32, device=dev)
    v.clip = torch.empty((T, 3, 4), dtype=torch.float32, device=dev) if clip else None
    v.dropped = torch.empty(S, dtype=torch.int32, device=dev)
    v.ground = torch.empty(S, dtype=torch.float32, device=dev) if ground else None
    v.tile_counts = torch.empty((S, v.nty, v.ntx), dtype=torch.int32, device=dev)
    lib = L.load()
    try:
        check(lib.sg_raster_setup(ptr(soup.positions) if T else None, ptr(soup.tri_offsets), S, T, _doubles(vp), v.width, v.height,
                                  int(bool(cull_back)), NEAR, ptr(v.recs) if T else None, ptr(v.flags) if T else None, ptr(v.clip) if T else None,
                                  ptr(v.dropped), ptr(v.ground), ptr(v.tile_counts), stream()), "raster_setup")
    finally:
        L.reset_call_state()
    return v


def bin_tiles(soup, v):
    S, T, dev = len(soup), soup.positions.shape[0], soup.device
    n = S * v.nty * v.ntx
    v.tile_offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    cursor = torch.empty(n, dtype=torch.int32, device=dev)
    v.active = torch.empty(n, dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    lib = L.load()
    try:
        check(lib.sg_raster_scan(ptr(v.tile_counts), n, ptr(v.tile_offsets), ptr(cursor), ptr(v.active), ptr(totals), stream()),
              "raster_scan")
    finally:
        L.reset_call_state()
    total, v.nactive = (int(x) for x in totals.cpu())      # the one device -> host read of a view
    v.lists = torch.empty(total, dtype=torch.int32, device=dev)
    if T and total:
        try:
            check(lib.sg_raster_fill(ptr(v.recs), ptr(v.flags), ptr(soup.tri_offsets), S, T, v.width, v.height, ptr(v.tile_offsets),
                                     ptr(cursor), ptr(v.lists), total, stream()), "raster_fill")
        finally:
            L.reset_call_state()
    return v


def visibility(soup, v, shadow=False):
    S, dev = len(soup), soup.device
    v.id = None if shadow else torch.empty((S, v.height, v.width), dtype=torch.int32, device=dev)
    v.depth = torch.empty((S, v.height, v.width), dtype=torch.float32, device=dev)
    lib = L.load()
    try:
        check(lib.sg_raster_visibility(ptr(v.recs) if v.nactive else None, ptr(soup.tri_offsets), S, v.width, v.height,
                                       ptr(v.tile_offsets), ptr(v.lists) if v.nactive else None, v.lists.shape[0],
                                       ptr(v.active) if v.nactive else None, v.nactive, ptr(v.id), ptr(v.depth), int(bool(shadow)), stream()),
              "raster_visibility")
    finally:
        L.reset_call_state()
    return v


def draw_view(soup, vp, width, height, cull_back, shadow=False, ground=False, clip=False):
    return visibility(soup, bin_tiles(soup, setup(soup, vp, width, height, cull_back, ground=ground, clip=clip)), shadow=shadow)


def shading_params(camera_vp, light_vp, albedo, background):
    """The 60 doubles of sg_raster_shade, computed in float64: VP, lightVP, VP^-1, the camera position, lightPosition =
    (VP lightVP^-1 (0, 0, -1, 1)).xyz, albedo, background."""
    camera_vp, light_vp = np.asarray(camera_vp, dtype=np.float64), np.asarray(light_vp, dtype=np.float64)
    inverse = np.linalg.inv(camera_vp)
    a, b = inverse @ np.array([0.0, 0.0, -1.0, 1.0]), inverse @ np.array([0.0, 0.0, 1.0, 1.0])
    a, b = a[:3] / a[3], b[:3] / b[3]
    # the centre ray's near (NDC z = -1) and far points lie at eye distances n and f along one line: eye = a - (b - a) n / (f - n)
    near = NEAR
    far = float(PROJECTION_MATRIX[2, 3] / (PROJECTION_MATRIX[2, 2] + 1.0))
    camera = a - (b - a) * near / (far - near)
    light = (camera_vp @ np.linalg.inv(light_vp) @ np.array([0.0, 0.0, -1.0, 1.0]))[:3]
    return np.concatenate([camera_vp.reshape(-1), light_vp.reshape(-1), inverse.reshape(-1), camera, light,
                           np.asarray(albedo, dtype=np.float64)[:3], np.asarray(background, dtype=np.float64)[:3]])


def shade(soup, cam, shadow_map, ground, params):
    S, T, dev = len(soup), soup.positions.shape[0], soup.device
    image = torch.empty((S, cam.height, cam.width, 3), dtype=torch.uint8, device=dev)
    lib = L.load()
    try:
        check(lib.sg_raster_shade(ptr(soup.positions) if T else None, ptr(soup.normals) if T else None, T, ptr(cam.recs) if T else None,
                                  ptr(cam.id), ptr(cam.depth), ptr(shadow_map), shadow_map.shape[-1], ptr(ground), _doubles(params), S,
                                  cam.width, cam.height, ptr(image), stream()), "raster_shade")
    finally:
        L.reset_call_state()
    return image


def resolve(samples, ssaa):
    """[S, H ssaa, W ssaa, 3] uint8 -> [S, H, W, 3]: the rounded mean of every ssaa x ssaa block."""
    if ssaa == 1:
        return samples
    S, Hs, Ws, _ = samples.shape
    image = torch.empty((S, Hs // ssaa, Ws // ssaa, 3), dtype=torch.uint8, device=samples.device)
    lib = L.load()
    try:
        check(lib.sg_raster_resolve(ptr(samples), S, Ws // ssaa, Hs // ssaa, int(ssaa), ptr(image), stream()), "raster_resolve")
    finally:
        L.reset_call_state()
    return image
