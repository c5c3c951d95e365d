"""Float64 / exact-integer restatement of the rasteriser's rules (include/shapegan_hip.h, K14), written from the header, in numpy.

Each function is the reference of ONE stage and starts from the previous stage's kernel output (fp32 records, ids, depths, shadow
map), so that a one-ulp difference upstream cannot show up as an error downstream.  Nothing here calls the library.
"""
import numpy as np

U = 2.0 ** -24                 # unit roundoff of fp32
SUB, HALF, GUARD, TILE = 256, 128, 1 << 22, 16
NEAR, GUARDED, ZERO_AREA, BACK, OFFSCREEN = 1, 2, 4, 8, 16


def f32_matrix(vp):
    """The view as the kernels see it: rounded once to fp32 (returned as float64)."""
    return np.asarray(vp, dtype=np.float64).astype(np.float32).astype(np.float64)


# ---- setup ------------------------------------------------------------------------------------------------------------------------
def setup(positions, vp, width, height, cull_back, near):
    """positions [T,3,3] fp32.  Returns clip [T,3,4] float64, its fp32 error bound [T,3,4] = 8 u sum_k |M[i][k] v[k]| (four products,
    three additions), the float64 window coordinates before rounding X, Y [T,3], and the flags (from float64 arithmetic)."""
    M = f32_matrix(vp)
    v = np.concatenate([positions.astype(np.float64), np.ones(positions.shape[:2] + (1,))], axis=2)          # [T,3,4]
    terms = v[:, :, None, :] * M[None, None, :, :]                                                          # [T,3,i,k]
    clip = terms.sum(axis=3)
    bound = 8 * U * np.abs(terms).sum(axis=3)
    w = clip[:, :, 3]
    near_flag = (w <= near).any(axis=1)
    with np.errstate(all="ignore"):
        X = (clip[:, :, 0] / w) * (HALF * width) + HALF * width
        Y = (clip[:, :, 1] / w) * (-HALF * height) + HALF * height
    guard_flag = ~near_flag & ((np.abs(X) > GUARD) | (np.abs(Y) > GUARD)).any(axis=1)
    return clip, bound, X, Y, near_flag, guard_flag


def flags_from_snapped(x, y, near_flag, guard_flag, cull_back, width, height):
    """The remaining flags are integer decisions on the kernel's own snapped coordinates x, y [T,3] (int64)."""
    a2 = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
    flags = np.where(near_flag, NEAR, np.where(guard_flag, GUARDED, 0))
    flags = np.where((flags == 0) & (a2 == 0), ZERO_AREA, flags)
    if cull_back:
        flags = np.where((flags == 0) & (a2 > 0), BACK, flags)
    px0, px1 = np.maximum(-((-(x.min(1) - HALF)) // SUB), 0), np.minimum((x.max(1) - HALF) // SUB, width - 1)
    py0, py1 = np.maximum(-((-(y.min(1) - HALF)) // SUB), 0), np.minimum((y.max(1) - HALF) // SUB, height - 1)
    empty = (px0 > px1) | (py0 > py1)
    flags = np.where((flags == 0) & empty, OFFSCREEN, flags)
    box = np.stack([px0, py0, px1, py1], axis=1)
    box[flags != 0] = (1, 1, 0, 0)
    return flags, box


def unpack_records(recs):
    """recs [T,16] int32 -> x, y [T,3] int64, z, iw [T,3] float64 (the fp32 values), box [T,4]."""
    recs = np.ascontiguousarray(recs)
    f = recs.view(np.float32)
    return (recs[:, 0:3].astype(np.int64), recs[:, 3:6].astype(np.int64), f[:, 6:9].astype(np.float64), f[:, 9:12].astype(np.float64),
            recs[:, 12:16].astype(np.int64))


def tile_sets(flags, box, tri_offsets, ntx, nty):
    """{(shape, ty, tx): set of triangle indices} of the kept triangles."""
    out = {}
    for s in range(len(tri_offsets) - 1):
        for t in range(int(tri_offsets[s]), int(tri_offsets[s + 1])):
            if flags[t]:
                continue
            for ty in range(box[t, 1] // TILE, box[t, 3] // TILE + 1):
                for tx in range(box[t, 0] // TILE, box[t, 2] // TILE + 1):
                    out.setdefault((s, ty, tx), set()).add(t)
    return out


# ---- visibility ---------------------------------------------------------------------------------------------------------------------
def edge_functions(x, y, width, height):
    """x, y [n,3] int64 -> e [n,3,H,W] int64 signed so that the inside is positive, inside [n,H,W] bool (top-left rule), |2 area| [n]."""
    sx = (np.arange(width, dtype=np.int64) * SUB + HALF)[None, None, :]
    sy = (np.arange(height, dtype=np.int64) * SUB + HALF)[None, :, None]
    a2 = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
    s = np.where(a2 < 0, -1, 1)
    e = np.empty((x.shape[0], 3, height, width), dtype=np.int64)
    inside = np.ones((x.shape[0], height, width), dtype=bool)
    for i in range(3):
        a, b = (i + 1) % 3, (i + 2) % 3
        dx, dy = ((x[:, b] - x[:, a]) * s)[:, None, None], ((y[:, b] - y[:, a]) * s)[:, None, None]
        e[:, i] = dx * (sy - y[:, a, None, None]) - dy * (sx - x[:, a, None, None])
        top_left = (dy < 0) | ((dy == 0) & (dx > 0))
        inside &= (e[:, i] > 0) | ((e[:, i] == 0) & top_left)
    return e, inside, np.abs(a2)


def visibility(recs, flags, t0, t1, width, height, chunk=256):
    """Brute force over the kept triangles [t0, t1) of one shape: every triangle against every sample.
    Returns count [H,W] (size of the covering set), id1 / z1 (nearest, ties to the lowest index), z2 (second nearest, inf if none),
    tau [H,W] = the fp32 error bound of the two depths compared (see depth_tau), cover = {triangle: bool [H,W]} when small."""
    x, y, z, _, _ = unpack_records(recs)
    count = np.zeros((height, width), dtype=np.int64)
    z1 = np.full((height, width), np.inf)
    z2 = np.full((height, width), np.inf)
    zm1 = np.zeros((height, width))
    zm2 = np.zeros((height, width))
    id1 = np.full((height, width), -1, dtype=np.int64)
    kept = [t for t in range(t0, t1) if flags[t] == 0]
    for c0 in range(0, len(kept), chunk):
        idx = np.array(kept[c0:c0 + chunk], dtype=np.int64)
        e, inside, a2 = edge_functions(x[idx], y[idx], width, height)
        l1, l2 = e[:, 1] / a2[:, None, None], e[:, 2] / a2[:, None, None]
        zz = z[idx, 0, None, None] + l1 * (z[idx, 1] - z[idx, 0])[:, None, None] + l2 * (z[idx, 2] - z[idx, 0])[:, None, None]
        zz = np.where(inside, zz, np.inf)
        zmax = np.abs(z[idx]).max(axis=1)
        count += inside.sum(axis=0)
        for k in range(len(idx)):          # increasing index: strict < keeps the lowest index of a tie
            d, m = zz[k], zmax[k]
            first = d < z1
            second = ~first & (d < z2)
            z2 = np.where(first, z1, np.where(second, d, z2))
            zm2 = np.where(first, zm1, np.where(second, m, zm2))
            z1 = np.where(first, d, z1)
            zm1 = np.where(first, m, zm1)
            id1 = np.where(first, idx[k], id1)
    return count, id1, z1, z2, depth_tau(zm1) + depth_tau(zm2)


def depth_tau(zmax):
    """Bound of |z_fp32 - z_exact| for z = fmaf(l2, z2 - z0, fmaf(l1, z1 - z0, z0)), l_i = (float)e_i * (1 / (float)A), Z = max |z_k|:
    (float)e_i, (float)A, the division and the product are one rounding each: l_i carries 4u; z_i - z0 one more: each product
    l_i (z_i - z0) is off by 5u |l_i| |z_i - z0| <= 5u * 2Z (0 <= l_i <= 1 inside the triangle); the two fused steps round results of
    magnitude <= 3Z: 2 * 3uZ.  Total 2 * 10uZ + 6uZ = 26 u Z."""
    return 26 * U * zmax


def coverage_single(recs, flags, t, width, height):
    x, y, _, _, _ = unpack_records(recs[t:t + 1])
    if flags[t]:
        return np.zeros((height, width), dtype=bool)
    return edge_functions(x, y, width, height)[1][0]


# ---- shading ------------------------------------------------------------------------------------------------------------------------
def _normalize(v):
    with np.errstate(all="ignore"):
        return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def _shadow(sp, d, smap, tau):
    """sp [...,4], d [...] -> shadow [...], fragile [...] (a comparison within tau of flipping)."""
    N = smap.shape[0]
    with np.errstate(all="ignore"):
        c = sp[..., :3] / sp[..., 3:4] * 0.5 + 0.5
        ref = c[..., 2] - np.maximum(0.002 * (1 - d), 0.001) / sp[..., 3]
    total = np.zeros(d.shape)
    fragile = np.zeros(d.shape, dtype=bool)
    flipped = smap[::-1]                       # texel row v counts from NDC y = -1
    for ox in (-1, 0, 1):
        for oy in (-1, 0, 1):
            tx, ty = (c[..., 0] + ox / N) * N + 0.5, (c[..., 1] + oy / N) * N + 0.5
            tx, ty = np.nan_to_num(tx, nan=-1.0, posinf=N, neginf=-1.0), np.nan_to_num(ty, nan=-1.0, posinf=N, neginf=-1.0)
            bx, by = np.floor(tx), np.floor(ty)
            fx, fy = tx - bx, ty - by
            ix, iy = np.clip(bx, -1, N).astype(np.int64), np.clip(by, -1, N).astype(np.int64)
            taps = {}
            for a in (0, 1):
                for b in (0, 1):
                    m = flipped[np.clip(iy + b, 0, N - 1), np.clip(ix + a, 0, N - 1)].astype(np.float64)
                    taps[a, b] = (ref > m).astype(np.float64)
                    fragile |= np.abs(ref - m) <= tau
            lo = taps[0, 0] + (taps[0, 1] - taps[0, 0]) * fy
            hi = taps[1, 0] + (taps[1, 1] - taps[1, 0]) * fy
            total += lo + (hi - lo) * fx
    shadow = np.clip(total / 9.0, 0.0, 1.0)
    dead = ~(c[..., 2] <= 1.0)
    return np.where(dead, 0.0, shadow), fragile & ~dead


def _rows(M, p, w):
    """M [4,4] times (p, w) for p [...,3] -> [...,4]"""
    return p @ M[:, :3].T + w * M[:, 3]


def shadow_tau(L, perr, p, sp):
    """fp32 bound of the shadow reference depth of a sample at world position p [...,3] whose fp32 position is off by at most
    u * perr [...,3] (mesh_perr / floor_perr).  A row of lightVP times (p, 1) is four fused steps on top of that:
    |d row_i| <= u (sum_k |L[i][k]| (perr_k + 4 |p_k|) + 4 |L[i][3]|) =: u A_i.  c.z = 0.5 z / w + 0.5, so
    |dc.z| <= 0.5 u (A_2 + |z / w| A_3) / |w|; the division, the scale-and-bias, the bias term and the subtraction add at most
    6u (|c.z| + 1) <= 6u (0.5 |z / w| + 1.5)."""
    A = (perr + 4 * np.abs(p)) @ np.abs(L[:, :3]).T + 4 * np.abs(L[:, 3])
    with np.errstate(all="ignore"):
        zw = np.abs(sp[..., 2] / sp[..., 3])
        return 0.5 * U * (A[..., 2] + zw * A[..., 3]) / np.abs(sp[..., 3]) + 6 * U * (0.5 * zw + 1.5)


def mesh_perr(v):
    """v [n,3,3]: the corners of each sample's triangle.  b_i = q_i / ((q0 + q1) + q2), q_i = l_i * iw_i: l_i carries 4u (depth_tau),
    the product 1u (iw_i comes from the kernel: upstream); the sum of three positive terms 2u, the division 1u: b_i is off by <= 9u
    relative.  p = sum b_i v_i in three roundings of partial sums no larger than max_i |v_i|: |dp_k| <= 12 u max_i |v_ik|."""
    return 12 * np.abs(v).max(axis=1)


def floor_perr(cam, p, d):
    """The floor point cam + t d: d = h.xyz / h.w - cam with h = a row product of four fused steps (4u on magnitudes <= |h| ~ |far
    point|), one division and one subtraction: |dd_k| <= 8u (|d_k| + |cam_k|) generously; t = (ground - cam_y) / d_y: 2u + the error of
    d_y, relative <= 10u (|d_y| + |cam_y|) / |d_y|; the last fused step 1u.  With |t d_k| = |p_k - cam_k| <= |p_k| + |cam_k| and
    (|d_y| + |cam_y|) / |d_y| <= 2 for a ray that reaches the plane from above the far points of this scene (|d_y| >= |cam_y|),
    |dp_k| <= (8 * 2 + 20 + 1) u (|p_k| + |cam_k|) <= 40 u (|p_k| + |cam_k|); the y coordinate is the ground level itself."""
    e = 40 * (np.abs(p) + np.abs(cam))
    e[..., 1] = 0.0
    return e


def shade(positions, normals, recs, ids, depth, smap, ground, params, width, height):
    """One shape.  positions / normals [T,3,3] fp32 (indices as in `ids`), recs the camera records, ids / depth [H,W] the kernel's
    visibility output, smap [N,N] the kernel's shadow map, params the 60 doubles.  Returns colour [H,W,3] float64 in [0,1] before the
    conversion to bytes, and fragile [H,W]."""
    P = np.asarray(params, dtype=np.float64).astype(np.float32).astype(np.float64)
    VP, LVP, IVP = P[0:16].reshape(4, 4), P[16:32].reshape(4, 4), P[32:48].reshape(4, 4)
    cam, light, albedo, background = P[48:51], P[51:54], P[54:57], P[57:60]
    colour = np.empty((height, width, 3))
    colour[:] = background
    fragile = np.zeros((height, width), dtype=bool)
    py, px = np.mgrid[0:height, 0:width]

    hit = ids >= 0
    if hit.any():
        t = ids[hit]
        x, y, _, iw, _ = unpack_records(recs[t])
        sx, sy = px[hit] * SUB + HALF, py[hit] * SUB + HALF
        a2 = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
        s = np.where(a2 < 0, -1, 1)
        e = np.empty((t.shape[0], 3))
        for i in range(3):
            a, b = (i + 1) % 3, (i + 2) % 3
            e[:, i] = ((x[:, b] - x[:, a]) * (sy - y[:, a]) - (y[:, b] - y[:, a]) * (sx - x[:, a])) * s
        q = e / np.abs(a2)[:, None] * iw
        bary = q / q.sum(axis=1, keepdims=True)
        v = positions[t].astype(np.float64)
        p = (bary[:, :, None] * v).sum(axis=1)
        if normals is not None:
            n = (bary[:, :, None] * normals[t].astype(np.float64)).sum(axis=1)
        else:
            n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
        pos = _rows(VP, p, 1.0)[:, :3]
        sp = _rows(LVP, p, 1.0)
        nv = _normalize(_rows(VP, n, 0.0)[:, :3])
        L = _normalize(light - pos)
        V = _normalize(-pos)
        nl = (nv * L).sum(-1)
        R = -_normalize(L - 2 * nl[:, None] * nv)
        d = np.clip(nl, 0, 1)
        sh, fr = _shadow(sp, d, smap, shadow_tau(LVP, mesh_perr(v), p, sp))
        lit = 1 - sh
        spec = np.maximum(0, (R * V).sum(-1)) ** 20
        rim = (1 - np.clip(-nv[:, 2], 0, 1)) ** 4
        c = albedo[None, :] * 0.5 + albedo[None, :] * 0.5 * (d * lit)[:, None] + (0.3 * spec * lit)[:, None] + (0.3 * rim)[:, None]
        colour[hit] = c
        fragile[hit] = fr
    # the floor wins wherever it is nearer than the mesh (depth is 1.0 where there is none)
    if cam[1] > ground:
        nx, ny = (px + 0.5) * (2.0 / width) - 1.0, (py + 0.5) * (-2.0 / height) + 1.0
        h = _rows(IVP, np.stack([nx, ny, np.ones_like(nx)], axis=-1), 1.0)
        with np.errstate(all="ignore"):
            d = h[..., :3] / h[..., 3:4] - cam
            t = (ground - cam[1]) / d[..., 1]
            fx, fz = cam[0] + t * d[..., 0], cam[2] + t * d[..., 2]
            p = np.stack([fx, np.full_like(fx, ground), fz], axis=-1)
            pos = _rows(VP, p, 1.0)
            zf = pos[..., 2] / pos[..., 3]
            ok = (t > 0) & (np.abs(fx) <= 6) & (np.abs(fz) <= 6) & (pos[..., 3] > 0) & (zf >= -1) & (zf <= 1) & (zf < depth)
        sp = _rows(LVP, p, 1.0)
        up = _normalize(VP[:3, 1])
        L = _normalize(light - pos[..., :3])
        dd = np.clip((up * L).sum(-1), 0, 1)
        sh, fr = _shadow(sp, dd, smap, shadow_tau(LVP, floor_perr(cam, p, d), p, sp))
        ok = np.nan_to_num(ok, nan=False).astype(bool)
        colour[ok] = (1.0 + sh * (0.4 - 1.0))[ok][:, None]
        fragile = np.where(ok, fr, fragile)

    return np.clip(np.nan_to_num(colour, nan=0.0), 0, 1), fragile
