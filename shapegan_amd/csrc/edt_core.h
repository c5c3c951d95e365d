// shapegan_amd/csrc/edt_core.h — the arithmetic of the distance transforms of voxel grids (K21): which voxels and which edge crossings are
// sites, the candidate of one pass, the exact minimum of a line, the order of the passes, the finishing step, and which kernel form a
// shape takes.
//
// Included by csrc/edt.hip and the twin (core_fn.h has the conventions).  T(p) = min over the sites q of f(q) + |p - q|^2 is separable:
// one pass per axis, each the minimum over the candidates of a line.  Every pass returns the EXACT minimum of its candidates, so the
// result does not depend on which lane looked at which candidate, and ties are broken by the smaller index along the line: the GPU in
// both of its forms and the twin agree bit for bit.  What each library keeps: where a line lives and which lane computes which output.
#pragma once
#include "core_fn.h"

#define SG_EDT_MAX_AXIS 512
// the floats of LDS the one-workgroup form holds: a whole grid, 128 KiB of the CU's 160 KiB (32^3 fits exactly)
#define SG_EDT_LDS_FLOATS 32768
#define SG_EDT_LDS_LANES 1024

// 0: one workgroup holds the grid in LDS and runs every pass there; 1: one launch per pass through global memory
SG_CORE_FN int sg_edt_form_of(long D, long H, long W) { return D * H * W <= SG_EDT_LDS_FLOATS ? 0 : 1; }

// ---- sites -----------------------------------------------------------------------------------------------------------------------------
// `voxels`: a voxel is a site when it is background: !(v < level), or v < level with `inside` set (NaN is never below the level)
SG_CORE_FN bool sg_edt_is_site(float v, float level, int inside) { return (v < level) == (inside != 0); }

// the candidate of a pass: d = (p - q) spacing in fp32 (one rounding), then one fused multiply-add onto the offset g >= 0
SG_CORE_FN float sg_edt_candidate(int p, int q, float spacing, float g) {
    const float d = (float)(p - q) * spacing;
    return __builtin_fmaf(d, d, g);
}

// `crossings`: the edge from voxel q to q + 1 of a line crosses the level when exactly one end is below it (mesh_core.h's inside rule);
// the crossing lies at the index coordinate u = q + t, t = (level - va) / (vb - va) as in sg_mc_vertex: 0 <= t <= 1 in fp32 too
SG_CORE_FN bool sg_edt_crosses(float va, float vb, float level) { return (va < level) != (vb < level); }
SG_CORE_FN float sg_edt_crossing_coord(int q, float va, float vb, float level) {
    const float t = (level - va) / (vb - va);
    return (float)q + t;
}
// the candidate of a crossing at u for voxel p of the same line: d = (p - u) spacing (two roundings), offset 0
SG_CORE_FN float sg_edt_crossing_candidate(int p, float u, float spacing) {
    const float d = ((float)p - u) * spacing;
    return __builtin_fmaf(d, d, 0.f);
}

// ---- one output of an axis pass --------------------------------------------------------------------------------------------------------
// min over q = 0 .. n - 1 of sg_edt_candidate(p, q, spacing, g[q stride]); *arg = the smallest q that attains it (on a line whose g
// are all +inf every q attains +inf and the scan never stops early: 0).  The scan goes outward from p and stops once the offset-free term alone exceeds the best: g >= 0 and rounding is monotone, so
// no candidate further out can be smaller or equal.
SG_CORE_FN float sg_edt_axis(const float* g, long stride, int n, int p, float spacing, int* arg) {
    float best = g[(long)p * stride];
    int bq = p;
    for (int k = 1; k < n; ++k) {
        const float d = (float)k * spacing;      // |d| of both candidates of this step
        if (d * d > best) break;
        const int lo = p - k, hi = p + k;
        if (lo < 0 && hi >= n) break;
        if (lo >= 0) {
            const float c = sg_edt_candidate(p, lo, spacing, g[(long)lo * stride]);
            if (c <= best) best = c, bq = lo;      // lo is below every index seen so far
        }
        if (hi < n) {
            const float c = sg_edt_candidate(p, hi, spacing, g[(long)hi * stride]);
            if (c < best) best = c, bq = hi;
        }
    }
    *arg = bq;
    return best;
}

// ---- one output of a crossing pass -----------------------------------------------------------------------------------------------------
// min over the crossing edges q = 0 .. n - 2 of the line v[0], v[stride], ... of sg_edt_crossing_candidate(p, u_q, spacing); *arg = the
// smallest such q, -1 and +inf when the line has no crossing.  Step k looks at the edges p - 1 - k and p + k, both at least k spacing
// away.
SG_CORE_FN float sg_edt_cross(const float* v, long stride, int n, int p, float level, float spacing, int* arg) {
    float best = INFINITY;
    int bq = -1;
    for (int k = 0; k < n; ++k) {
        const float d = (float)k * spacing;
        if (d * d > best) break;
        const int lo = p - 1 - k, hi = p + k;
        if (lo < 0 && hi + 1 >= n) break;
        if (lo >= 0) {
            const float va = v[(long)lo * stride], vb = v[(long)(lo + 1) * stride];
            if (sg_edt_crosses(va, vb, level)) {
                const float c = sg_edt_crossing_candidate(p, sg_edt_crossing_coord(lo, va, vb, level), spacing);
                if (c <= best) best = c, bq = lo;
            }
        }
        if (hi + 1 < n) {
            const float va = v[(long)hi * stride], vb = v[(long)(hi + 1) * stride];
            if (sg_edt_crosses(va, vb, level)) {
                const float c = sg_edt_crossing_candidate(p, sg_edt_crossing_coord(hi, va, vb, level), spacing);
                if (c < best) best = c, bq = hi;
            }
        }
    }
    *arg = bq;
    return best;
}

// ---- the order of the passes -----------------------------------------------------------------------------------------------------------
// `voxels`: W, then H, then D.  `crossings`: the families of the edges along D, H, W in this order, each its crossing pass and then the
// two other axes in increasing order; where two families tie the earlier one keeps the voxel.
SG_CORE_FN int sg_edt_other_axis(int axis, int which) { return which == 0 ? (axis == 0 ? 1 : 0) : (axis == 2 ? 1 : 2); }

// a line view [outer][n][inner] of a grid [D][H][W] along `axis`
SG_CORE_FN void sg_edt_view(int axis, int D, int H, int W, int* outer, int* n, int* inner) {
    *outer = axis == 0 ? 1 : axis == 1 ? D : D * H;
    *n = axis == 0 ? D : axis == 1 ? H : W;
    *inner = axis == 0 ? H * W : axis == 1 ? W : 1;
}

// the code of a crossing: the linear index of the edge's lower voxel (< 2^27) and the edge's axis; -1: none
SG_CORE_FN int sg_edt_code(int voxel, int axis) { return voxel * 4 + axis; }

// the world position of a coded crossing of grid g [D][H][W], as sg_mc_vertex places it with origin 0; NaN for code -1
SG_CORE_FN void sg_edt_decode(const float* g, int H, int W, int code, float level, const float spacing[3], float pos[3]) {
    if (code < 0) {
        pos[0] = pos[1] = pos[2] = NAN;
        return;
    }
    const int voxel = code >> 2, axis = code & 3;
    const int d = voxel / (H * W), h = voxel / W % H, w = voxel % W;
    const float va = g[voxel], vb = g[voxel + (axis == 0 ? H * W : axis == 1 ? W : 1)];
    const float u = sg_edt_crossing_coord(axis == 0 ? d : axis == 1 ? h : w, va, vb, level);
    pos[0] = (axis == 0 ? u : (float)d) * spacing[0];
    pos[1] = (axis == 1 ? u : (float)h) * spacing[1];
    pos[2] = (axis == 2 ? u : (float)w) * spacing[2];
}

// ---- finishing -------------------------------------------------------------------------------------------------------------------------
// s sqrt(T), s = -1 where v < level else +1 (sqrt is IEEE); with keep_band a voxel that has a 6-neighbour on the other side of the level
// keeps (v - level) value_scale
SG_CORE_FN float sg_edt_root(float squared) { return sqrtf(squared); }
SG_CORE_FN float sg_edt_finish_value(const float* g, int D, int H, int W, int d, int h, int w, float squared, float level, float value_scale,
                                     int keep_band) {
    const long i = ((long)d * H + h) * W + w;
    const float v = g[i];
    const bool in = v < level;
    if (keep_band) {
        bool band = false;
        if (d > 0) band |= (g[i - (long)H * W] < level) != in;
        if (d + 1 < D) band |= (g[i + (long)H * W] < level) != in;
        if (h > 0) band |= (g[i - W] < level) != in;
        if (h + 1 < H) band |= (g[i + W] < level) != in;
        if (w > 0) band |= (g[i - 1] < level) != in;
        if (w + 1 < W) band |= (g[i + 1] < level) != in;
        if (band) return (v - level) * value_scale;
    }
    const float r = sg_edt_root(squared);
    return in ? -r : r;
}
