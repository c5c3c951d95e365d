// shapegan_amd/csrc/meshsdf_core.h — the per-pair arithmetic of the mesh-to-SDF conversion (K16): the squared distance from a point to a
// triangle with its closest point, and the visibility of a point in one orthographic scan.
//
// Included by csrc/meshsdf.hip and the twin (core_fn.h has the conventions).  What each library keeps: the walk over the triangles,
// the running minimum (strict <, increasing index: the lowest index of a tie) and the loop over the scans.
#pragma once
#include "core_fn.h"
#include "../../include/shapegan_hip.h"      // SG_MESHSDF_*

// What the distance needs of a triangle, made once per call by sg_msdf_record: 32 floats, eight 16-byte reads.
struct alignas(16) SgMsdfRec {
    float a[3], iab;      // corner a, 1 / |ab|^2
    float b[3], ibc;
    float c[3], ica;
    float ab[3], pad0;    // b - a
    float bc[3], pad1;    // c - b
    float ca[3], pad2;    // a - c
    float gv[3], pad3;    // (ac x n) / |n|^2: the barycentric weight of b of a point p is (p - a) . gv   (n = ab x ac)
    float gw[3], pad4;    // (n x ab) / |n|^2: the weight of c is (p - a) . gw
};

SG_CORE_FN float sg_msdf_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx));
}

// 1 / x for a divisor that is never 0: a squared length below 1e-30 (an edge shorter than 1e-15, a collapsed triangle, NaN) gives 0,
// which parks the parameter it scales at the start of the edge / at corner a — still a point of the triangle.
SG_CORE_FN float sg_msdf_inv(float x) { return x >= 1e-30f ? 1.0f / x : 0.0f; }

SG_CORE_FN void sg_msdf_record(const float* tri, SgMsdfRec* r) {
    SG_CORE_UNROLL
    for (int i = 0; i < 3; ++i) {
        r->a[i] = tri[i];
        r->b[i] = tri[3 + i];
        r->c[i] = tri[6 + i];
        r->ab[i] = tri[3 + i] - tri[i];
        r->bc[i] = tri[6 + i] - tri[3 + i];
        r->ca[i] = tri[i] - tri[6 + i];
    }
    const float acx = -r->ca[0], acy = -r->ca[1], acz = -r->ca[2];
    r->iab = sg_msdf_inv(sg_msdf_dot(r->ab[0], r->ab[1], r->ab[2], r->ab[0], r->ab[1], r->ab[2]));
    r->ibc = sg_msdf_inv(sg_msdf_dot(r->bc[0], r->bc[1], r->bc[2], r->bc[0], r->bc[1], r->bc[2]));
    r->ica = sg_msdf_inv(sg_msdf_dot(r->ca[0], r->ca[1], r->ca[2], r->ca[0], r->ca[1], r->ca[2]));
    // n = ab x ac, each component fmaf(a, b, -(c d))
    const float nx = __builtin_fmaf(r->ab[1], acz, -(r->ab[2] * acy)), ny = __builtin_fmaf(r->ab[2], acx, -(r->ab[0] * acz)),
                nz = __builtin_fmaf(r->ab[0], acy, -(r->ab[1] * acx));
    const float inn = sg_msdf_inv(sg_msdf_dot(nx, ny, nz, nx, ny, nz));
    r->gv[0] = __builtin_fmaf(acy, nz, -(acz * ny)) * inn;
    r->gv[1] = __builtin_fmaf(acz, nx, -(acx * nz)) * inn;
    r->gv[2] = __builtin_fmaf(acx, ny, -(acy * nx)) * inn;
    r->gw[0] = __builtin_fmaf(ny, r->ab[2], -(nz * r->ab[1])) * inn;
    r->gw[1] = __builtin_fmaf(nz, r->ab[0], -(nx * r->ab[2])) * inn;
    r->gw[2] = __builtin_fmaf(nx, r->ab[1], -(ny * r->ab[0])) * inn;
    r->pad0 = r->pad1 = r->pad2 = r->pad3 = r->pad4 = 0.0f;
}

// the residual p - (o + t e) of the closest point of the segment o + t e, t in [0, 1], from q = p - o; returns its squared length
SG_CORE_FN float sg_msdf_edge(float qx, float qy, float qz, const float* e, float inv, float* t_out) {
    float t = sg_msdf_dot(qx, qy, qz, e[0], e[1], e[2]) * inv;
    t = t > 0.0f ? t : 0.0f;      // comparisons, not fmaxf: -0 and NaN both give +0 in either library
    t = t < 1.0f ? t : 1.0f;
    const float rx = __builtin_fmaf(-t, e[0], qx), ry = __builtin_fmaf(-t, e[1], qy), rz = __builtin_fmaf(-t, e[2], qz);
    *t_out = t;
    return sg_msdf_dot(rx, ry, rz, rx, ry, rz);
}

// The squared distance from p to the triangle of r: the smallest of four candidates, each the squared length of p - c for a point c
// of the triangle, so the value is a distance to the triangle whatever the rounding did to the choice:
//   the three edges, each from its own start corner (p on a corner gives exactly 0);
//   the face, only when the weights v, w of b and c satisfy v >= 0, w >= 0, v + w <= 1:  c = a + v ab + w ac.
// A triangle without area has gv = gw = 0 or weights without meaning; the face candidate is then a point of its segment at best
// and never below the edges' by more than rounding.  No division, no branch.  closest (may be NULL): the point c of the winner,
// the first of edge ab, bc, ca, face on a tie.
SG_CORE_FN float sg_msdf_d2(float px, float py, float pz, const SgMsdfRec& r, float* closest) {
    const float ax = px - r.a[0], ay = py - r.a[1], az = pz - r.a[2];
    const float bx = px - r.b[0], by = py - r.b[1], bz = pz - r.b[2];
    const float cx = px - r.c[0], cy = py - r.c[1], cz = pz - r.c[2];
    float t0, t1, t2;
    const float d0 = sg_msdf_edge(ax, ay, az, r.ab, r.iab, &t0);
    const float d1 = sg_msdf_edge(bx, by, bz, r.bc, r.ibc, &t1);
    const float d2 = sg_msdf_edge(cx, cy, cz, r.ca, r.ica, &t2);
    const float v = sg_msdf_dot(ax, ay, az, r.gv[0], r.gv[1], r.gv[2]), w = sg_msdf_dot(ax, ay, az, r.gw[0], r.gw[1], r.gw[2]);
    // ac = -ca
    const float fx = __builtin_fmaf(w, r.ca[0], __builtin_fmaf(-v, r.ab[0], ax)), fy = __builtin_fmaf(w, r.ca[1], __builtin_fmaf(-v, r.ab[1], ay)),
                fz = __builtin_fmaf(w, r.ca[2], __builtin_fmaf(-v, r.ab[2], az));
    const float df = sg_msdf_dot(fx, fy, fz, fx, fy, fz);
    const bool inside = v >= 0.0f && w >= 0.0f && v + w <= 1.0f;      // false for NaN
    float best = d0;
    int which = 0;
    if (d1 < best) best = d1, which = 1;
    if (d2 < best) best = d2, which = 2;
    if (inside && df < best) best = df, which = 3;
    if (closest) {
        SG_CORE_UNROLL
        for (int i = 0; i < 3; ++i)
            closest[i] = which == 0   ? __builtin_fmaf(t0, r.ab[i], r.a[i])
                         : which == 1 ? __builtin_fmaf(t1, r.bc[i], r.b[i])
                         : which == 2 ? __builtin_fmaf(t2, r.ca[i], r.c[i])
                                      : __builtin_fmaf(-w, r.ca[i], __builtin_fmaf(v, r.ab[i], r.a[i]));
    }
    return best;
}

// ---- the sign: is the point seen by the scan with rows M[0..12) (rows 0..2 of its view matrix, f32) and depth map `depth` [N][N]? ----
SG_CORE_FN bool sg_msdf_visible(const float* M, float x, float y, float z, const float* depth, int N, float bias) {
    const float c0 = __builtin_fmaf(M[2], z, __builtin_fmaf(M[1], y, __builtin_fmaf(M[0], x, M[3])));
    const float c1 = __builtin_fmaf(M[6], z, __builtin_fmaf(M[5], y, __builtin_fmaf(M[4], x, M[7])));
    const float c2 = __builtin_fmaf(M[10], z, __builtin_fmaf(M[9], y, __builtin_fmaf(M[8], x, M[11])));
    const float h = 0.5f * (float)N;
    const float fx = __builtin_fmaf(c0, h, h), fy = __builtin_fmaf(c1, -h, h);
    const bool in_window = fx >= 0.0f && fx < (float)N && fy >= 0.0f && fy < (float)N;      // false for NaN
    if (!in_window) return true;
    const float t = depth[(long)(int)fy * N + (int)fx];
    return t == 1.0f || c2 < t - bias;
}

// what the entry points refuse, in the library and the twin alike
SG_CORE_FN bool sg_msdf_sizes_ok(long S, long T, long Q) {
    return S >= 1 && S <= 65535 && T >= 0 && T <= SG_MESHSDF_MAX_TRIANGLES && Q >= 1 && Q <= SG_MESHSDF_MAX_POINTS && S * Q <= SG_MESHSDF_MAX_TOTAL_POINTS;
}
// K scans of N x N texels with an orthographic view each: row 3 of every vp is (0, 0, 0, 1)
SG_CORE_FN bool sg_msdf_scans_ok(const double* vps, int K, int N, float bias) {
    if (!vps || K < 1 || K > SG_MESHSDF_MAX_SCANS || N < 1 || N > 16384 || !(bias >= 0.0f) || !(bias < INFINITY)) return false;
    for (int k = 0; k < K; ++k)
        if (vps[k * 16 + 12] != 0.0 || vps[k * 16 + 13] != 0.0 || vps[k * 16 + 14] != 0.0 || vps[k * 16 + 15] != 1.0) return false;
    return true;
}
