// shapegan_amd/csrc/spline.hip — cubic B-spline resampling of voxel grids (K20): prefilter, zoom, sampling at points.
//
// scipy.ndimage.zoom(voxels_32, 4) of create_plot.py:826-828 on the device (include/shapegan_hip.h has the contract, csrc/spline_core.h
// every formula).  The kernels decide only which lane does what and where a value lives:
//   prefilter_lds    form 0: ONE workgroup of 1024 lanes holds a whole grid in LDS (row stride W | 1: lanes that each walk a row of
//                    their own hit different banks), filters along W, H and D there, one lane per line, and writes the
//                    coefficients once.  A 32^3 grid is 132 KiB with the padding.
//   prefilter_rows   form 1, the W pass: 64 rows of a grid pass through LDS (the same odd stride), so that the loads and the stores are
//                    coalesced although every lane walks along a row; one lane per row.
//   prefilter_axis   form 1, the H and D passes, in place in global memory: one lane per line, neighbouring lanes on neighbouring w,
//                    so every step of the walk is one coalesced access.
//   zoom_tile        form 0: a workgroup makes an 8 x 8 x 64 tile of the output.  It copies the box of coefficients the tile needs
//                    (its extent divided by the zoom factor, plus 3; mirror-folded while it is copied) into LDS and evaluates
//                    separably in the order of sg_spline_dot4: the W sums of the box, the H sums of those, and the D sums.  After the
//                    copy a lane IS an output column: every stage reads and writes rows of 64 consecutive floats, the weights of the
//                    H and D stages are the same for a whole wave, and a wave stores one row of the output at a time.
//   zoom_direct      form 1 (a box that does not fit: downscaling by a large factor): one lane per output, 64 taps from global memory.
//   sample           one lane per point, 64 taps from global memory, value and gradient.
// Plain vector loads and stores only: no atomics, no scratch buffers, no inline assembly.
#include <algorithm>

#include "common.h"
#include "../../include/shapegan_hip.h"

// every value is compared bit for bit with the twin: the only fused steps are the explicit fmaf
#pragma clang fp contract(off)
#include "spline_core.h"

namespace sg {

constexpr int kSpTD = SG_SPLINE_TILE_D, kSpTH = SG_SPLINE_TILE_H, kSpTW = SG_SPLINE_TILE_W;
constexpr int kSpRows = 64;          // rows of the staged W pass per workgroup
static_assert(kSpTW == 64 && kSpTD * kSpTH * kSpTW == 4096, "a wave stores one row of a tile; 256 lanes make 16 outputs each");

// ---- prefilter -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) spline_prefilter_lds_kernel(const float* __restrict__ grids, int D, int H, int W,
                                                                    float* __restrict__ coefficients) {
    extern __shared__ float sp_lds[];
    const int Wp = (int)sg_spline_row_stride(W), rows = D * H, n = rows * W, tid = threadIdx.x, bs = blockDim.x;
    const float* src = grids + (long)blockIdx.x * n;
    float* dst = coefficients + (long)blockIdx.x * n;
    for (int i = tid; i < n; i += bs) sp_lds[(i / W) * Wp + i % W] = src[i];
    __syncthreads();
    if (W > 1)
        for (int line = tid; line < rows; line += bs) sg_spline_line(sp_lds + line * Wp, 1, W);
    __syncthreads();
    if (H > 1)
        for (int line = tid; line < D * W; line += bs) sg_spline_line(sp_lds + (line / W) * H * Wp + line % W, Wp, H);
    __syncthreads();
    if (D > 1)
        for (int line = tid; line < H * W; line += bs) sg_spline_line(sp_lds + (line / W) * Wp + line % W, (long)H * Wp, D);
    __syncthreads();
    for (int i = tid; i < n; i += bs) dst[i] = sp_lds[(i / W) * Wp + i % W];
}

// rows [rows][W] of `src` -> filtered rows of `dst`; rows_per workgroup rows at a time
__global__ void __launch_bounds__(256) spline_prefilter_rows_kernel(const float* __restrict__ src, long rows, int W, int rows_per,
                                                                    float* __restrict__ dst) {
    extern __shared__ float sp_lds[];
    const int Wp = (int)sg_spline_row_stride(W), tid = threadIdx.x;
    const long row0 = (long)blockIdx.x * rows_per;
    const int count = (int)(rows - row0 < rows_per ? rows - row0 : rows_per), n = count * W;
    for (int i = tid; i < n; i += 256) sp_lds[(i / W) * Wp + i % W] = src[row0 * W + i];
    __syncthreads();
    if (tid < count) sg_spline_line(sp_lds + tid * Wp, 1, W);
    __syncthreads();
    for (int i = tid; i < n; i += 256) dst[row0 * W + i] = sp_lds[(i / W) * Wp + i % W];
}

// c viewed as [outer][n][inner]: every line along n, in place
__global__ void __launch_bounds__(256) spline_prefilter_axis_kernel(float* __restrict__ c, long outer, int n, long inner) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= outer * inner) return;
    sg_spline_line(c + (gid / inner) * n * inner + gid % inner, inner, n);
}

// ---- zoom ------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) spline_zoom_tile_kernel(const float* __restrict__ coefficients, long s0, int D, int H, int W, int D2,
                                                               int H2, int W2, int order, float* __restrict__ out) {
    extern __shared__ float sp_lds[];
    __shared__ float tab_w[kSpTD + kSpTH + kSpTW][4];
    __shared__ int tab_f[kSpTD + kSpTH + kSpTW];
    constexpr int kH = kSpTD, kW = kSpTD + kSpTH;      // where the H and the W entries of the tables begin
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles_w = (W2 + kSpTW - 1) / kSpTW, tiles_h = (H2 + kSpTH - 1) / kSpTH, tiles_d = (D2 + kSpTD - 1) / kSpTD;
    const int tiles = tiles_w * tiles_h * tiles_d;
    const long s = s0 + blockIdx.x / tiles;
    int tile = blockIdx.x % tiles;
    const int ow0 = (tile % tiles_w) * kSpTW;
    tile /= tiles_w;
    const int oh0 = (tile % tiles_h) * kSpTH, od0 = (tile / tiles_h) * kSpTD;
    const int cd = min(kSpTD, D2 - od0), ch = min(kSpTH, H2 - oh0), cw = min(kSpTW, W2 - ow0);

    if (tid < kSpTD + kSpTH + kSpTW) {            // the taps of every output index of the tile: floor of the position, weights
        int i = tid, n = D, N = D2, o0 = od0, count = cd;
        if (tid >= kW) i = tid - kW, n = W, N = W2, o0 = ow0, count = cw;
        else if (tid >= kH) i = tid - kH, n = H, N = H2, o0 = oh0, count = ch;
        if (i < count) {
            int f;
            float t, w[4];
            sg_spline_coord(o0 + i, n, N, &f, &t);
            sg_spline_weights(t, order, w);
            tab_w[tid][0] = w[0], tab_w[tid][1] = w[1], tab_w[tid][2] = w[2], tab_w[tid][3] = w[3];
            tab_f[tid] = f;
        }
    }
    __syncthreads();
    // the box: unfolded indices lo .. lo + extent - 1 along every axis, lo = the first tap of the tile's first output
    const int lo_d = tab_f[0] - 1, sd = tab_f[cd - 1] - tab_f[0] + 4;
    const int lo_h = tab_f[kH] - 1, sh = tab_f[kH + ch - 1] - tab_f[kH] + 4;
    const int lo_w = tab_f[kW] - 1, sw = tab_f[kW + cw - 1] - tab_f[kW] + 4;
    const int plane = sh * sw;
    float* box = sp_lds;                          // [sd][sh][sw]
    float* sum_w = box + sd * plane;              // [sd][sh][64]
    float* sum_h = sum_w + sd * sh * kSpTW;       // [sd][ch][64]

    const float* src = coefficients + s * ((long)D * H * W);
    for (int r = tid; r < plane; r += 256) {
        const int j = r / sw, k = r - j * sw;
        const float* col = src + (long)sg_spline_mirror(lo_h + j, H) * W + sg_spline_mirror(lo_w + k, W);
        for (int i = 0; i < sd; ++i) box[i * plane + r] = col[(long)sg_spline_mirror(lo_d + i, D) * H * W];
    }
    __syncthreads();
    // from here on lane = ow: a wave makes one row of 64 at a time, and every LDS access is lane-consecutive or a broadcast
    const int ow = lane < cw ? lane : cw - 1;     // lanes beyond the tile compute on its last column and store nothing
    {
        const float w[4] = {tab_w[kW + ow][0], tab_w[kW + ow][1], tab_w[kW + ow][2], tab_w[kW + ow][3]};
        const float* p = box + (tab_f[kW + ow] - 1 - lo_w);
        for (int row = wave; row < sd * sh; row += 4)
            sum_w[row * kSpTW + lane] = sg_spline_dot4(w, p[row * sw], p[row * sw + 1], p[row * sw + 2], p[row * sw + 3]);
    }
    __syncthreads();
    for (int oh = wave; oh < ch; oh += 4) {
        const float w[4] = {tab_w[kH + oh][0], tab_w[kH + oh][1], tab_w[kH + oh][2], tab_w[kH + oh][3]};
        const float* p = sum_w + (tab_f[kH + oh] - 1 - lo_h) * kSpTW + lane;
        for (int i = 0; i < sd; ++i, p += sh * kSpTW)
            sum_h[(i * ch + oh) * kSpTW + lane] = sg_spline_dot4(w, p[0], p[kSpTW], p[2 * kSpTW], p[3 * kSpTW]);
    }
    __syncthreads();
    float* dst = out + s * ((long)D2 * H2 * W2) + ow0 + lane;
    const int step = ch * kSpTW;
    for (int od = 0; od < cd; ++od) {
        const float w[4] = {tab_w[od][0], tab_w[od][1], tab_w[od][2], tab_w[od][3]};
        const float* p = sum_h + (tab_f[od] - 1 - lo_d) * step + lane;
        for (int oh = wave; oh < ch; oh += 4) {
            const float v = sg_spline_dot4(w, p[oh * kSpTW], p[oh * kSpTW + step], p[oh * kSpTW + 2 * step], p[oh * kSpTW + 3 * step]);
            if (lane < cw) dst[((long)(od0 + od) * H2 + oh0 + oh) * W2] = v;
        }
    }
}

__global__ void __launch_bounds__(256) spline_zoom_direct_kernel(const float* __restrict__ coefficients, long total, int D, int H, int W,
                                                                 int D2, int H2, int W2, int order, float* __restrict__ out) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int ow = (int)(gid % W2);
    long r = gid / W2;
    const int oh = (int)(r % H2);
    r /= H2;
    const int od = (int)(r % D2);
    const long s = r / D2;
    int fd, fh, fw;
    float td, th, tw;
    sg_spline_coord(od, D, D2, &fd, &td);
    sg_spline_coord(oh, H, H2, &fh, &th);
    sg_spline_coord(ow, W, W2, &fw, &tw);
    out[gid] = sg_spline_point(coefficients + s * ((long)D * H * W), D, H, W, fd, td, fh, th, fw, tw, order, nullptr);
}

// ---- sample ----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) spline_sample_kernel(const float* __restrict__ coefficients, long total, int D, int H, int W,
                                                            const float* __restrict__ points, long P, float outside,
                                                            float* __restrict__ values, float* __restrict__ gradient) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const float x = points[gid * 3], y = points[gid * 3 + 1], z = points[gid * 3 + 2];
    int fd, fh, fw;
    float td, th, tw;
    float g[3] = {0.f, 0.f, 0.f};
    float v = outside;
    const bool in_d = sg_spline_locate(x, D, &fd, &td), in_h = sg_spline_locate(y, H, &fh, &th), in_w = sg_spline_locate(z, W, &fw, &tw);
    if (in_d && in_h && in_w)
        v = sg_spline_point(coefficients + (gid / P) * ((long)D * H * W), D, H, W, fd, td, fh, th, fw, tw, 3, gradient ? g : nullptr);
    values[gid] = v;
    if (gradient) gradient[gid * 3] = g[0], gradient[gid * 3 + 1] = g[1], gradient[gid * 3 + 2] = g[2];
}

static bool spline_axes_ok(long D, long H, long W) {
    return D >= 1 && H >= 1 && W >= 1 && D <= SG_SPLINE_MAX_AXIS && H <= SG_SPLINE_MAX_AXIS && W <= SG_SPLINE_MAX_AXIS;
}

constexpr long kSpMaxElements = 1L << 36;      // of one call: every kernel's block count stays below 2^31

}  // namespace sg

extern "C" {

int sg_spline_prefilter_form(long D, long H, long W) {
    SG_CHECK_ARG(sg::spline_axes_ok(D, H, W));
    return sg_spline_prefilter_form_of(D, H, W);
}

int sg_spline_zoom_form(long D, long H, long W, long D2, long H2, long W2) {
    SG_CHECK_ARG(sg::spline_axes_ok(D, H, W) && sg::spline_axes_ok(D2, H2, W2));
    return sg_spline_zoom_form_of(D, H, W, D2, H2, W2);
}

int sg_spline_prefilter(const float* grids, long S, long D, long H, long W, float* coefficients, hipStream_t stream) {
    SG_CHECK_ARG(S >= 0 && sg::spline_axes_ok(D, H, W) && S <= sg::kSpMaxElements / (D * H * W));
    SG_CHECK_ARG((grids && coefficients && grids != coefficients) || S == 0);
    if (S == 0) return SG_OK;
    if (sg_spline_prefilter_form_of(D, H, W) == 0) {
        SG_CHECK_ARG(S <= 2147483647L);
        static SgPerDeviceOnce once;
        const int rc = sg_reserve_lds(once, sg::spline_prefilter_lds_kernel, SG_SPLINE_LDS_FLOATS * sizeof(float), __func__);
        if (rc != SG_OK) return rc;
        hipLaunchKernelGGL(sg::spline_prefilter_lds_kernel, dim3((unsigned)S), dim3(1024), (size_t)(D * H * sg_spline_row_stride(W)) * sizeof(float),
                           stream, grids, (int)D, (int)H, (int)W, coefficients);
        SG_CHECK_LAUNCH();
        return SG_OK;
    }
    static SgPerDeviceOnce once_rows;
    const int rc = sg_reserve_lds(once_rows, sg::spline_prefilter_rows_kernel, SG_SPLINE_LDS_FLOATS * sizeof(float), __func__);
    if (rc != SG_OK) return rc;
    const long Wp = sg_spline_row_stride(W), rows = S * D * H;
    const int rows_per = (int)std::min<long>(sg::kSpRows, SG_SPLINE_LDS_FLOATS / Wp);
    hipLaunchKernelGGL(sg::spline_prefilter_rows_kernel, dim3((unsigned)((rows + rows_per - 1) / rows_per)), dim3(256),
                       (size_t)(rows_per * Wp) * sizeof(float), stream, grids, rows, (int)W, rows_per, coefficients);
    SG_CHECK_LAUNCH();
    if (H > 1) {
        hipLaunchKernelGGL(sg::spline_prefilter_axis_kernel, dim3((unsigned)((S * D * W + 255) / 256)), dim3(256), 0, stream, coefficients, S * D,
                           (int)H, W);
        SG_CHECK_LAUNCH();
    }
    if (D > 1) {
        hipLaunchKernelGGL(sg::spline_prefilter_axis_kernel, dim3((unsigned)((S * H * W + 255) / 256)), dim3(256), 0, stream, coefficients, S,
                           (int)D, H * W);
        SG_CHECK_LAUNCH();
    }
    return SG_OK;
}

int sg_spline_zoom(const float* coefficients, long S, long D, long H, long W, long D2, long H2, long W2, int order, float* out,
                   hipStream_t stream) {
    SG_CHECK_ARG(S >= 0 && sg::spline_axes_ok(D, H, W) && sg::spline_axes_ok(D2, H2, W2) && (order == 1 || order == 3));
    SG_CHECK_ARG(S <= sg::kSpMaxElements / (D * H * W) && S <= sg::kSpMaxElements / (D2 * H2 * W2));
    SG_CHECK_ARG((coefficients && out && coefficients != out) || S == 0);
    if (S == 0) return SG_OK;
    const long lds_floats = sg_spline_zoom_lds_floats(D, H, W, D2, H2, W2);
    if (lds_floats > SG_SPLINE_ZOOM_LDS_FLOATS) {
        const long total = S * D2 * H2 * W2;
        hipLaunchKernelGGL(sg::spline_zoom_direct_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, coefficients, total, (int)D,
                           (int)H, (int)W, (int)D2, (int)H2, (int)W2, order, out);
        SG_CHECK_LAUNCH();
        return SG_OK;
    }
    static SgPerDeviceOnce once;
    const int rc = sg_reserve_lds(once, sg::spline_zoom_tile_kernel, SG_SPLINE_ZOOM_LDS_FLOATS * sizeof(float), __func__);
    if (rc != SG_OK) return rc;
    const long tiles = sg_cdiv(D2, SG_SPLINE_TILE_D) * (long)sg_cdiv(H2, SG_SPLINE_TILE_H) * sg_cdiv(W2, SG_SPLINE_TILE_W);
    const long per_launch = 2147483647L / tiles;          // grids of one launch: the block count is an int
    for (long s0 = 0; s0 < S; s0 += per_launch) {
        const long count = std::min(per_launch, S - s0);
        hipLaunchKernelGGL(sg::spline_zoom_tile_kernel, dim3((unsigned)(count * tiles)), dim3(256), (size_t)lds_floats * sizeof(float), stream,
                           coefficients, s0, (int)D, (int)H, (int)W, (int)D2, (int)H2, (int)W2, order, out);
        SG_CHECK_LAUNCH();
    }
    return SG_OK;
}

int sg_spline_sample(const float* coefficients, long S, long D, long H, long W, const float* points, long P, float outside, float* values,
                     float* gradient, hipStream_t stream) {
    SG_CHECK_ARG(S >= 0 && P >= 0 && sg::spline_axes_ok(D, H, W) && S <= sg::kSpMaxElements / (D * H * W));
    SG_CHECK_ARG(S == 0 || P == 0 || S <= sg::kSpMaxElements / (3 * P));
    SG_CHECK_ARG((coefficients && points && values) || S == 0 || P == 0);
    if (S == 0 || P == 0) return SG_OK;
    const long total = S * P;
    hipLaunchKernelGGL(sg::spline_sample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, coefficients, total, (int)D, (int)H,
                       (int)W, points, P, outside, values, gradient);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

}  // extern "C"
