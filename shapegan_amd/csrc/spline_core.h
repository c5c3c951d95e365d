// shapegan_amd/csrc/spline_core.h — the arithmetic of cubic B-spline resampling of voxel grids (K20): the prefilter of one line, the
// coordinate and the tap weights of an output index, the mirror fold, the order of the 64-tap sum, and which kernel form a shape takes.
//
// Included by csrc/spline.hip and the twin (core_fn.h has the conventions).  This is scipy.ndimage.zoom / map_coordinates at their
// defaults (order 3, mode 'constant', grid_mode False): the prefilter with the mirror (whole-sample symmetric) boundary, the
// coordinate o (n - 1) / (N - 1).  What each library keeps: which line a lane filters and where a tap's value is read from.
#pragma once
#include "core_fn.h"

#define SG_SPLINE_TILE_D 8
#define SG_SPLINE_TILE_H 8
#define SG_SPLINE_TILE_W 64
#define SG_SPLINE_MAX_AXIS 4096
// the floats of LDS one workgroup may hold: 136 KiB of the CU's 160 KiB
#define SG_SPLINE_LDS_FLOATS 34816
// the floats a zoom tile (coefficient box and the two intermediates of the separable evaluation) may hold: 112 KiB
#define SG_SPLINE_ZOOM_LDS_FLOATS 28672

// the pole of the cubic B-spline, (float)(sqrt(3) - 2)
#define SG_SPLINE_POLE (-0.26794919243112270647f)

// ---- the prefilter of one line c[0], c[stride], ..., c[(n - 1) stride], in place -----------------------------------------------------
// Every fused step is written out; everything else is a single rounded operation, in this order.
SG_CORE_FN void sg_spline_line(float* c, long stride, int n) {
    if (n <= 1) return;
    const float z = SG_SPLINE_POLE;
    float zn = 1.f;                                        // z^(n - 1) by n - 1 products
    for (int i = 1; i < n; ++i) zn = zn * z;
    const float last = 6.f * c[(long)(n - 1) * stride];
    // the causal start: c0 = sum_i z^i (c[i] + z^(n-1) c[n-1-i]), i = 0 .. n - 2, over the line scaled by 6
    float c0 = __builtin_fmaf(zn, last, 6.f * c[0]);
    float zi = z;
    for (int i = 1; i <= n - 2; ++i) {
        c0 = __builtin_fmaf(zi, __builtin_fmaf(zn, 6.f * c[(long)(n - 1 - i) * stride], 6.f * c[(long)i * stride]), c0);
        zi = zi * z;
    }
    float prev = c0 / (1.f - zn * zn);
    c[0] = prev;
    for (int i = 1; i < n; ++i) {                          // the causal pass
        prev = __builtin_fmaf(z, prev, 6.f * c[(long)i * stride]);
        c[(long)i * stride] = prev;
    }
    // the anticausal start: prev is c[n - 1] of the causal pass; c[n - 2] is in memory
    prev = __builtin_fmaf(z, c[(long)(n - 2) * stride], prev) * (z / (z * z - 1.f));
    c[(long)(n - 1) * stride] = prev;
    for (int i = n - 2; i >= 0; --i) {                     // the anticausal pass
        prev = z * (prev - c[(long)i * stride]);
        c[(long)i * stride] = prev;
    }
}

// ---- coordinates -----------------------------------------------------------------------------------------------------------------------
// output index o of N along an axis of n: the position o (n - 1) / (N - 1) as its floor f and its fraction t, in integers
// (n, N <= SG_SPLINE_MAX_AXIS: the product stays below 2^24)
SG_CORE_FN void sg_spline_coord(int o, int n, int N, int* f, float* t) {
    if (N <= 1) {
        *f = 0;
        *t = 0.f;
        return;
    }
    const int num = o * (n - 1);
    *f = num / (N - 1);
    *t = (float)(num % (N - 1)) / (float)(N - 1);
}

// the periodic mirror of period 2 (n - 1): ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ...; i may be any integer
SG_CORE_FN int sg_spline_mirror(int i, int n) {
    if (i >= 0 && i < n) return i;
    if (n <= 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

// the weights of the taps f - 1 .. f + 2 at fraction t.  order 3: the cubic B-spline; order 1: (0, 1 - t, t, 0), so that both orders
// run the same four-tap sum (a zero weight leaves the sum of finite values as it is)
SG_CORE_FN void sg_spline_weights(float t, int order, float* w) {
    const float u = 1.f - t;
    if (order == 1) {
        w[0] = 0.f, w[1] = u, w[2] = t, w[3] = 0.f;
        return;
    }
    w[0] = ((u * u) * u) / 6.f;
    w[1] = __builtin_fmaf(t * t, __builtin_fmaf(3.f, t, -6.f), 4.f) / 6.f;
    w[2] = __builtin_fmaf(t, __builtin_fmaf(t, __builtin_fmaf(-3.f, t, 3.f), 3.f), 1.f) / 6.f;
    w[3] = ((t * t) * t) / 6.f;
}

// their derivatives with respect to t (order 3)
SG_CORE_FN void sg_spline_dweights(float t, float* w) {
    const float u = 1.f - t;
    w[0] = -0.5f * (u * u);
    w[1] = t * __builtin_fmaf(1.5f, t, -2.f);
    w[2] = __builtin_fmaf(t, __builtin_fmaf(-1.5f, t, 1.f), 0.5f);
    w[3] = 0.5f * (t * t);
}

// THE sum of four taps.  The 64-tap sum of a point is dot4 along D of (dot4 along H of (dot4 along W of the coefficients)): the W
// sums first, for each of the 16 (d, h) tap pairs; then the H sums, for each of the 4 d taps; then the D sum.
SG_CORE_FN float sg_spline_dot4(const float* w, float v0, float v1, float v2, float v3) {
    return __builtin_fmaf(w[3], v3, __builtin_fmaf(w[2], v2, __builtin_fmaf(w[1], v1, w[0] * v0)));
}

// a sample position x along an axis of n: inside [0, n - 1] (NaN is outside) it gives f = floor(x), at most n - 2, and t = x - f
SG_CORE_FN bool sg_spline_locate(float x, int n, int* f, float* t) {
    if (!(x >= 0.f && x <= (float)(n - 1))) return false;
    int i = (int)floorf(x);
    if (i > n - 2) i = n - 2;
    if (i < 0) i = 0;                                      // n == 1: x == 0
    *f = i;
    *t = x - (float)i;
    return true;
}

// value (and, with grad != NULL, the gradient [3] in index units) at (fd + td, fh + th, fw + tw) of the coefficients c [D][H][W]
SG_CORE_FN float sg_spline_point(const float* c, int D, int H, int W, int fd, float td, int fh, float th, int fw, float tw, int order,
                                 float* grad) {
    float wd[4], wh[4], ww[4], dd[4] = {0.f, 0.f, 0.f, 0.f}, dh[4] = {0.f, 0.f, 0.f, 0.f}, dw[4] = {0.f, 0.f, 0.f, 0.f};
    sg_spline_weights(td, order, wd);
    sg_spline_weights(th, order, wh);
    sg_spline_weights(tw, order, ww);
    if (grad) {
        sg_spline_dweights(td, dd);
        sg_spline_dweights(th, dh);
        sg_spline_dweights(tw, dw);
    }
    long od[4], oh[4];
    int ow[4];
    SG_CORE_UNROLL
    for (int k = 0; k < 4; ++k) {
        od[k] = (long)sg_spline_mirror(fd - 1 + k, D) * H * W;
        oh[k] = (long)sg_spline_mirror(fh - 1 + k, H) * W;
        ow[k] = sg_spline_mirror(fw - 1 + k, W);
    }
    float a[4], a_h[4] = {0.f, 0.f, 0.f, 0.f}, a_w[4] = {0.f, 0.f, 0.f, 0.f};      // per d tap: the (h, w) sum, with dh for wh, with dw for ww
    SG_CORE_UNROLL
    for (int i = 0; i < 4; ++i) {
        float b[4], b_w[4];
        SG_CORE_UNROLL
        for (int j = 0; j < 4; ++j) {
            const float* p = c + od[i] + oh[j];
            const float v0 = p[ow[0]], v1 = p[ow[1]], v2 = p[ow[2]], v3 = p[ow[3]];
            b[j] = sg_spline_dot4(ww, v0, v1, v2, v3);
            b_w[j] = grad ? sg_spline_dot4(dw, v0, v1, v2, v3) : 0.f;
        }
        a[i] = sg_spline_dot4(wh, b[0], b[1], b[2], b[3]);
        if (grad) {
            a_h[i] = sg_spline_dot4(dh, b[0], b[1], b[2], b[3]);
            a_w[i] = sg_spline_dot4(wh, b_w[0], b_w[1], b_w[2], b_w[3]);
        }
    }
    if (grad) {
        grad[0] = sg_spline_dot4(dd, a[0], a[1], a[2], a[3]);
        grad[1] = sg_spline_dot4(wd, a_h[0], a_h[1], a_h[2], a_h[3]);
        grad[2] = sg_spline_dot4(wd, a_w[0], a_w[1], a_w[2], a_w[3]);
    }
    return sg_spline_dot4(wd, a[0], a[1], a[2], a[3]);
}

// ---- kernel forms (host arithmetic; the twin answers the same) ------------------------------------------------------------------------
// the row stride of a grid held in LDS: odd, so that lanes that each walk a row of their own hit different banks
SG_CORE_FN long sg_spline_row_stride(long W) { return W | 1; }

// prefilter: 0 = the whole grid in the LDS of one workgroup, 1 = one pass per axis through global memory
SG_CORE_FN int sg_spline_prefilter_form_of(long D, long H, long W) {
    return D * H * sg_spline_row_stride(W) <= SG_SPLINE_LDS_FLOATS ? 0 : 1;
}

// the longest run of coefficients f(o_last) - f(o_first) + 4 that a tile of T outputs needs along an axis
SG_CORE_FN long sg_spline_span(long n, long N, long T) {
    long span = 0;
    for (long o0 = 0; o0 < N; o0 += T) {
        const long o1 = (o0 + T < N ? o0 + T : N) - 1;
        int f0, f1;
        float t;
        sg_spline_coord((int)o0, (int)n, (int)N, &f0, &t);
        sg_spline_coord((int)o1, (int)n, (int)N, &f1, &t);
        if (f1 - f0 + 4 > span) span = f1 - f0 + 4;
    }
    return span;
}

// the LDS floats of the tiled zoom: the coefficient box [sd][sh][sw], the W sums [sd][sh][TILE_W], the H sums [sd][TILE_H][TILE_W]
SG_CORE_FN long sg_spline_zoom_lds_floats(long D, long H, long W, long D2, long H2, long W2) {
    const long sd = sg_spline_span(D, D2, SG_SPLINE_TILE_D), sh = sg_spline_span(H, H2, SG_SPLINE_TILE_H),
               sw = sg_spline_span(W, W2, SG_SPLINE_TILE_W);
    return sd * sh * sw + sd * sh * SG_SPLINE_TILE_W + sd * SG_SPLINE_TILE_H * SG_SPLINE_TILE_W;
}

// zoom: 0 = tiles of the output evaluated separably from a coefficient box in LDS, 1 = one lane per output, 64 taps from global memory
SG_CORE_FN int sg_spline_zoom_form_of(long D, long H, long W, long D2, long H2, long W2) {
    return sg_spline_zoom_lds_floats(D, H, W, D2, H2, W2) <= SG_SPLINE_ZOOM_LDS_FLOATS ? 0 : 1;
}
