// shapegan_amd/csrc/edt.hip — distance transforms of voxel grids (K21): exact Euclidean distance transform and redistancing.
//
// scipy.ndimage.distance_transform_edt and the redistancing of the truncated grids of datasets.py:7-40 on the device
// (include/shapegan_hip.h has the contract, csrc/edt_core.h every formula).  Every pass is the exact minimum of a line's candidates, one
// lane per output; the kernels decide only where a line lives:
//   edt_*_lds      form 0: ONE workgroup of 1024 lanes holds a whole grid in LDS (32^3 fp32 = 128 KiB) and runs every pass there, in
//                  place: a round computes the outputs of as many COMPLETE lines as the lanes cover, one output per lane, and stores
//                  them after a barrier, so no lane reads a value of this pass.  Along W the lanes of a wave walk one line
//                  (consecutive banks); along H and D neighbouring lanes hold neighbouring w of neighbouring lines (consecutive
//                  banks again).  The crossing passes read the grid itself from global memory (L2-resident: each value is read by
//                  the few lanes around it) and the running minimum over the three edge families is kept in the output.
//   edt_*_kernel   form 1: one launch per pass from one global array to another, one lane per output, neighbouring lanes on
//                  neighbouring w: a workgroup owns a slab of 256 adjacent columns of the D and H passes, and every step of the scan is
//                  one coalesced access; along W the lanes of a wave walk one line and read their neighbours' values.
// The nearest-site arrays travel through global memory in both forms (they are optional).  Plain vector loads and stores only.
#include "common.h"
#include "../../include/shapegan_hip.h"

// every value is compared bit for bit with the twin: the only fused steps are the explicit fmaf
#pragma clang fp contract(off)
#include "edt_core.h"

namespace sg {

constexpr int kEdtLanes = SG_EDT_LDS_LANES;
static_assert(SG_EDT_MAX_AXIS <= kEdtLanes / 2, "a round covers at least two complete lines");

__device__ __forceinline__ float edt_pick(int axis, float d, float h, float w) { return axis == 0 ? d : axis == 1 ? h : w; }

// ---- form 0 ----------------------------------------------------------------------------------------------------------------------------
// T viewed [outer][n][inner], in place; ids (global, [outer n inner]) follow the attaining index when IDS
template <bool IDS>
__device__ __forceinline__ void edt_lds_axis(float* T, int* ids, int outer, int n, int inner, float spacing) {
    if (n == 1) return;      // the only candidate is the voxel itself
    const int tid = threadIdx.x, lines = outer * inner, per = kEdtLanes / n;
    for (int l0 = 0; l0 < lines; l0 += per) {
        int line, p;
        if (inner == 1) line = l0 + tid / n, p = tid % n;
        else line = l0 + tid % per, p = tid / per;
        const bool active = p < n && line < l0 + per && line < lines;
        float r = 0.f;
        int id = -1;
        long at = 0;
        if (active) {
            const long base = (long)(line / inner) * n * inner + line % inner;
            int q;
            r = sg_edt_axis(T + base, inner, n, p, spacing, &q);
            if (IDS) id = ids[base + (long)q * inner];
            at = base + (long)p * inner;
        }
        __syncthreads();
        if (active) {
            T[at] = r;
            if (IDS) ids[at] = id;
        }
        __syncthreads();
    }
}

template <bool IDS>
__global__ void __launch_bounds__(kEdtLanes) edt_voxels_lds_kernel(const float* __restrict__ grids, int D, int H, int W, float level, int inside,
                                                                   float sd, float sh, float sw, float* __restrict__ squared, int* nearest) {
    extern __shared__ float edt_lds[];
    const int n = D * H * W, tid = threadIdx.x;
    const float* src = grids + (long)blockIdx.x * n;
    int* ids = IDS ? nearest + (long)blockIdx.x * n : nullptr;
    for (int i = tid; i < n; i += kEdtLanes) {
        const bool site = sg_edt_is_site(src[i], level, inside);
        edt_lds[i] = site ? 0.f : INFINITY;
        if (IDS) ids[i] = site ? i : -1;
    }
    __syncthreads();
    edt_lds_axis<IDS>(edt_lds, ids, D * H, W, 1, sw);
    edt_lds_axis<IDS>(edt_lds, ids, D, H, W, sh);
    edt_lds_axis<IDS>(edt_lds, ids, 1, D, H * W, sd);
    float* dst = squared + (long)blockIdx.x * n;
    for (int i = tid; i < n; i += kEdtLanes) dst[i] = edt_lds[i];
}

template <bool IDS>
__global__ void __launch_bounds__(kEdtLanes) edt_crossings_lds_kernel(const float* __restrict__ grids, int D, int H, int W, float level, float sd,
                                                                      float sh, float sw, float* squared, float* __restrict__ closest,
                                                                      int* codes, int* best_codes) {
    extern __shared__ float edt_lds[];
    const int n = D * H * W, tid = threadIdx.x;
    const float* src = grids + (long)blockIdx.x * n;
    int* ids = IDS ? codes + (long)blockIdx.x * n : nullptr;
    // the running minimum over the families lives in the output itself: element i is read and written by one lane only
    float* dst = squared + (long)blockIdx.x * n;
    int* best = IDS ? best_codes + (long)blockIdx.x * n : nullptr;
    for (int axis = 0; axis < 3; ++axis) {
        int outer, len, inner;
        sg_edt_view(axis, D, H, W, &outer, &len, &inner);
        for (int i = tid; i < n; i += kEdtLanes) {
            const int o = i / (len * inner), p = i / inner % len, in = i % inner;
            const long base = (long)o * len * inner + in;
            int q;
            edt_lds[i] = sg_edt_cross(src + base, inner, len, p, level, edt_pick(axis, sd, sh, sw), &q);
            if (IDS) ids[i] = q < 0 ? -1 : sg_edt_code((int)(base + (long)q * inner), axis);
        }
        __syncthreads();
        for (int which = 0; which < 2; ++which) {
            const int other = sg_edt_other_axis(axis, which);
            int o2, n2, i2;
            sg_edt_view(other, D, H, W, &o2, &n2, &i2);
            edt_lds_axis<IDS>(edt_lds, ids, o2, n2, i2, edt_pick(other, sd, sh, sw));
        }
        for (int i = tid; i < n; i += kEdtLanes) {
            const float c = edt_lds[i];
            if (axis == 0 || c < dst[i]) {      // the earlier family keeps a tie
                dst[i] = c;
                if (IDS) best[i] = ids[i];
            }
        }
        __syncthreads();      // the next family overwrites the grid in LDS and the codes
    }
    if (IDS)
        for (int i = tid; i < n; i += kEdtLanes) {      // best[i] is this lane's own store
            const float sp[3] = {sd, sh, sw};
            float pos[3];
            sg_edt_decode(src, H, W, best[i], level, sp, pos);
            float* c = closest + ((long)blockIdx.x * n + i) * 3;
            c[0] = pos[0], c[1] = pos[1], c[2] = pos[2];
        }
}

// ---- form 1 ----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) edt_site_voxels_kernel(const float* __restrict__ grids, long total, long n, float level, int inside,
                                                              float* __restrict__ T, int* __restrict__ ids) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const bool site = sg_edt_is_site(grids[gid], level, inside);
    T[gid] = site ? 0.f : INFINITY;
    if (ids) ids[gid] = site ? (int)(gid % n) : -1;
}

// the grids viewed [outer][len][inner] (outer spans the batch); grid_n = D H W
__global__ void __launch_bounds__(256) edt_site_cross_kernel(const float* __restrict__ grids, long total, int len, long inner, long grid_n,
                                                             int axis, float level, float spacing, float* __restrict__ T,
                                                             int* __restrict__ ids) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const long base = gid / (len * inner) * (len * inner) + gid % inner;
    const int p = (int)(gid / inner % len);
    int q;
    T[gid] = sg_edt_cross(grids + base, inner, len, p, level, spacing, &q);
    if (ids) ids[gid] = q < 0 ? -1 : sg_edt_code((int)((base + (long)q * inner) % grid_n), axis);
}

// merge: the output keeps what it holds unless this pass's result is smaller (the earlier family wins a tie)
__global__ void __launch_bounds__(256) edt_axis_kernel(const float* __restrict__ Tin, const int* __restrict__ id_in, long total, int len,
                                                       long inner, float spacing, int merge, float* __restrict__ Tout,
                                                       int* __restrict__ id_out) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const long base = gid / (len * inner) * (len * inner) + gid % inner;
    const int p = (int)(gid / inner % len);
    int q;
    const float r = sg_edt_axis(Tin + base, inner, len, p, spacing, &q);
    if (merge && !(r < Tout[gid])) return;
    Tout[gid] = r;
    if (id_out) id_out[gid] = id_in[base + (long)q * inner];
}

__global__ void __launch_bounds__(256) edt_decode_kernel(const float* __restrict__ grids, const int* __restrict__ codes, long total, int H, int W,
                                                         long grid_n, float level, float sd, float sh, float sw,
                                                         float* __restrict__ closest) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const float sp[3] = {sd, sh, sw};
    float pos[3];
    sg_edt_decode(grids + gid / grid_n * grid_n, H, W, codes[gid], level, sp, pos);
    closest[gid * 3] = pos[0], closest[gid * 3 + 1] = pos[1], closest[gid * 3 + 2] = pos[2];
}

__global__ void __launch_bounds__(256) edt_finish_kernel(const float* __restrict__ grids, const float* squared, long total, int D, int H, int W,
                                                         float level, float value_scale, int keep_band, float* out) {
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    if (!grids) {      // the plain root: no sign, no band
        out[gid] = sg_edt_root(squared[gid]);
        return;
    }
    const long grid_n = (long)D * H * W, i = gid % grid_n;
    out[gid] = sg_edt_finish_value(grids + (gid - i), D, H, W, (int)(i / ((long)H * W)), (int)(i / W % H), (int)(i % W), squared[gid], level,
                                   value_scale, keep_band);
}

static bool edt_axes_ok(long D, long H, long W) {
    return D >= 1 && H >= 1 && W >= 1 && D <= SG_EDT_MAX_AXIS && H <= SG_EDT_MAX_AXIS && W <= SG_EDT_MAX_AXIS;
}

constexpr long kEdtMaxElements = 1L << 36;      // of one call: every kernel's block count stays below 2^31

static size_t edt_workspace_bytes(int sites, long S, long D, long H, long W, int nearest) {
    const size_t cells = (size_t)S * D * H * W * sizeof(float);
    if (sg_edt_form_of(D, H, W) == 0) return sites == SG_EDT_CROSSINGS && nearest ? 2 * cells : 0;      // the codes and the best of them
    return cells * (2 + (nearest ? (sites == SG_EDT_CROSSINGS ? 3 : 2) : 0));
}

static unsigned edt_blocks(long total) { return (unsigned)((total + 255) / 256); }

}  // namespace sg

extern "C" {

int sg_edt_form(long D, long H, long W) {
    SG_CHECK_ARG(sg::edt_axes_ok(D, H, W));
    return sg_edt_form_of(D, H, W);
}

size_t sg_edt_workspace_bytes(int sites, long S, long D, long H, long W, int nearest) {
    if (S < 0 || !sg::edt_axes_ok(D, H, W) || S > sg::kEdtMaxElements / (D * H * W)) return 0;
    return sg::edt_workspace_bytes(sites, S, D, H, W, nearest);
}

int sg_edt_voxels(const float* grids, long S, long D, long H, long W, float level, int inside, float spacing_d, float spacing_h,
                  float spacing_w, float* squared, int* nearest, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    SG_CHECK_ARG(S >= 0 && sg::edt_axes_ok(D, H, W) && S <= sg::kEdtMaxElements / (D * H * W));
    SG_CHECK_ARG(spacing_d > 0.f && spacing_h > 0.f && spacing_w > 0.f && spacing_d < INFINITY && spacing_h < INFINITY && spacing_w < INFINITY);
    SG_CHECK_ARG(level == level);
    SG_CHECK_ARG((grids && squared && grids != squared) || S == 0);
    if (S == 0) return SG_OK;
    const size_t need = sg::edt_workspace_bytes(SG_EDT_VOXELS, S, D, H, W, nearest != nullptr);
    if (need && (!workspace || workspace_bytes < need)) SG_FAIL(SG_ERR_WORKSPACE, "%s: workspace of %zu B, %zu B needed", __func__, workspace_bytes, need);
    const long n = D * H * W, total = S * n;
    if (sg_edt_form_of(D, H, W) == 0) {
        SG_CHECK_ARG(S <= 2147483647L);
        static SgPerDeviceOnce once, once_ids;
        const int rc = nearest ? sg_reserve_lds(once_ids, sg::edt_voxels_lds_kernel<true>, SG_EDT_LDS_FLOATS * sizeof(float), __func__)
                               : sg_reserve_lds(once, sg::edt_voxels_lds_kernel<false>, SG_EDT_LDS_FLOATS * sizeof(float), __func__);
        if (rc != SG_OK) return rc;
        if (nearest)
            hipLaunchKernelGGL(sg::edt_voxels_lds_kernel<true>, dim3((unsigned)S), dim3(sg::kEdtLanes), (size_t)n * sizeof(float), stream, grids,
                               (int)D, (int)H, (int)W, level, inside, spacing_d, spacing_h, spacing_w, squared, nearest);
        else
            hipLaunchKernelGGL(sg::edt_voxels_lds_kernel<false>, dim3((unsigned)S), dim3(sg::kEdtLanes), (size_t)n * sizeof(float), stream, grids,
                               (int)D, (int)H, (int)W, level, inside, spacing_d, spacing_h, spacing_w, squared, nearest);
        SG_CHECK_LAUNCH();
        return SG_OK;
    }
    float* A = (float*)workspace;
    float* B = A + total;
    int* IA = nearest ? (int*)(B + total) : nullptr;
    int* IB = nearest ? IA + total : nullptr;
    const unsigned blocks = sg::edt_blocks(total);
    hipLaunchKernelGGL(sg::edt_site_voxels_kernel, dim3(blocks), dim3(256), 0, stream, grids, total, n, level, inside, A, IA);
    SG_CHECK_LAUNCH();
    hipLaunchKernelGGL(sg::edt_axis_kernel, dim3(blocks), dim3(256), 0, stream, A, IA, total, (int)W, 1L, spacing_w, 0, B, IB);
    SG_CHECK_LAUNCH();
    hipLaunchKernelGGL(sg::edt_axis_kernel, dim3(blocks), dim3(256), 0, stream, B, IB, total, (int)H, W, spacing_h, 0, A, IA);
    SG_CHECK_LAUNCH();
    hipLaunchKernelGGL(sg::edt_axis_kernel, dim3(blocks), dim3(256), 0, stream, A, IA, total, (int)D, H * W, spacing_d, 0, squared, nearest);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_edt_crossings(const float* grids, long S, long D, long H, long W, float level, float spacing_d, float spacing_h, float spacing_w,
                     float* squared, float* closest, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    SG_CHECK_ARG(S >= 0 && sg::edt_axes_ok(D, H, W) && S <= sg::kEdtMaxElements / (D * H * W));
    SG_CHECK_ARG(spacing_d > 0.f && spacing_h > 0.f && spacing_w > 0.f && spacing_d < INFINITY && spacing_h < INFINITY && spacing_w < INFINITY);
    SG_CHECK_ARG(level == level);
    SG_CHECK_ARG((grids && squared && grids != squared && grids != closest && squared != closest) || S == 0);
    if (S == 0) return SG_OK;
    const size_t need = sg::edt_workspace_bytes(SG_EDT_CROSSINGS, S, D, H, W, closest != nullptr);
    if (need && (!workspace || workspace_bytes < need)) SG_FAIL(SG_ERR_WORKSPACE, "%s: workspace of %zu B, %zu B needed", __func__, workspace_bytes, need);
    const long n = D * H * W, total = S * n;
    if (sg_edt_form_of(D, H, W) == 0) {
        SG_CHECK_ARG(S <= 2147483647L);
        static SgPerDeviceOnce once, once_ids;
        const int rc = closest ? sg_reserve_lds(once_ids, sg::edt_crossings_lds_kernel<true>, SG_EDT_LDS_FLOATS * sizeof(float), __func__)
                               : sg_reserve_lds(once, sg::edt_crossings_lds_kernel<false>, SG_EDT_LDS_FLOATS * sizeof(float), __func__);
        if (rc != SG_OK) return rc;
        if (closest)
            hipLaunchKernelGGL(sg::edt_crossings_lds_kernel<true>, dim3((unsigned)S), dim3(sg::kEdtLanes), (size_t)n * sizeof(float), stream, grids,
                               (int)D, (int)H, (int)W, level, spacing_d, spacing_h, spacing_w, squared, closest, (int*)workspace, (int*)workspace + total);
        else
            hipLaunchKernelGGL(sg::edt_crossings_lds_kernel<false>, dim3((unsigned)S), dim3(sg::kEdtLanes), (size_t)n * sizeof(float), stream, grids,
                               (int)D, (int)H, (int)W, level, spacing_d, spacing_h, spacing_w, squared, closest, (int*)nullptr, (int*)nullptr);
        SG_CHECK_LAUNCH();
        return SG_OK;
    }
    float* A = (float*)workspace;
    float* B = A + total;
    int* IA = closest ? (int*)(B + total) : nullptr;
    int* IB = closest ? IA + total : nullptr;
    int* IC = closest ? IB + total : nullptr;
    const unsigned blocks = sg::edt_blocks(total);
    const float sp[3] = {spacing_d, spacing_h, spacing_w};
    const long len[3] = {D, H, W}, inner[3] = {H * W, W, 1};
    for (int axis = 0; axis < 3; ++axis) {
        const int b = sg_edt_other_axis(axis, 0), c = sg_edt_other_axis(axis, 1);
        hipLaunchKernelGGL(sg::edt_site_cross_kernel, dim3(blocks), dim3(256), 0, stream, grids, total, (int)len[axis], inner[axis], n, axis, level,
                           sp[axis], A, IA);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(sg::edt_axis_kernel, dim3(blocks), dim3(256), 0, stream, A, IA, total, (int)len[b], inner[b], sp[b], 0, B, IB);
        SG_CHECK_LAUNCH();
        hipLaunchKernelGGL(sg::edt_axis_kernel, dim3(blocks), dim3(256), 0, stream, B, IB, total, (int)len[c], inner[c], sp[c], axis > 0 ? 1 : 0,
                           squared, IC);
        SG_CHECK_LAUNCH();
    }
    if (closest) {
        hipLaunchKernelGGL(sg::edt_decode_kernel, dim3(blocks), dim3(256), 0, stream, grids, IC, total, (int)H, (int)W, n, level, spacing_d,
                           spacing_h, spacing_w, closest);
        SG_CHECK_LAUNCH();
    }
    return SG_OK;
}

int sg_edt_finish(const float* grids, const float* squared, long S, long D, long H, long W, float level, float value_scale, int keep_band,
                  float* out, hipStream_t stream) {
    SG_CHECK_ARG(S >= 0 && sg::edt_axes_ok(D, H, W) && S <= sg::kEdtMaxElements / (D * H * W));
    SG_CHECK_ARG((squared && out && (grids ? grids != out && grids != squared : keep_band == 0)) || S == 0);
    if (S == 0) return SG_OK;
    const long total = S * D * H * W;
    hipLaunchKernelGGL(sg::edt_finish_kernel, dim3(sg::edt_blocks(total)), dim3(256), 0, stream, grids, squared, total, (int)D, (int)H, (int)W,
                       level, value_scale, keep_band, out);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

}  // extern "C"
