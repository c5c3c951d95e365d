// shapegan_amd/csrc/raster.hip — tiled triangle rasteriser with shadow map and analytic floor (K14): the headless MeshRenderer.
//
// The consumer of K12: S triangle soups (vertices[faces] of a MeshBatch) drawn in a handful of launches, twice each — from the light
// (depth only, nothing culled) and from the camera — through ONE code path:
//   setup        one lane per triangle: clip coordinates, snapped window coordinates, flags, sample box; integer atomics count the
//                triangle into every tile its box touches, count the dropped ones per shape and lower the shape's ground level
//                (the order-preserving integer image of min y).
//   scan         one workgroup: exclusive sum of the tile counts, the compact list of non-empty tiles, the fill cursors zeroed.
//   fill         one lane per triangle: its index into the list of every tile it touches.  The slot comes from an atomic cursor, so
//                the ORDER inside a list is not fixed — the winner rule of visibility is a minimum with an index tie-break and does
//                not depend on it.
//   visibility   clears the buffers, then one 256-lane workgroup per NON-EMPTY (shape, tile), one sample per lane.  Records are staged
//                through LDS 256 at a time (16 KB: ten workgroups fit a CU's 160 KB, more than its 32 waves admit); every lane reads
//                the same record (a broadcast, no bank conflict); a wave skips a record whose sample box misses its own 16 x 4
//                rectangle.  Edge functions are int64 on the snapped coordinates; nearest depth and triangle stay in registers; the only
//                global traffic is the record loads and one store per sample.
//   shade        one lane per sample: the fragment rules of the header, the floor as a ray against the ground plane, the background.
//   resolve      box average of ssaa x ssaa samples, in integers.
// The arithmetic lives in raster_core.h, shared with the twin.
#include "common.h"
#include "../../include/shapegan_hip.h"

// results are compared bit for bit with the twin: the only fused steps are the explicit fmaf of raster_core.h
#pragma clang fp contract(off)
#include "raster_core.h"

namespace sg {

constexpr int kRsBlock = 256;
static_assert(SG_RS_TILE * SG_RS_TILE == kRsBlock && SG_RS_CHUNK == kRsBlock, "one sample and one staged record per lane");

// shape of triangle t: the s with tri_offsets[s] <= t < tri_offsets[s + 1] (offsets non-decreasing; -1 if none)
__device__ __forceinline__ long rs_shape_of(const int64_t* __restrict__ tri_offsets, long S, long t) {
    long lo = 0, hi = S;      // invariant: the answer, if any, is in [lo, hi)
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if (tri_offsets[mid] <= t) lo = mid;
        else hi = mid;
    }
    return (tri_offsets[lo] <= t && t < tri_offsets[lo + 1]) ? lo : -1;
}

__global__ void __launch_bounds__(256) rs_init_kernel(int* __restrict__ dropped, int* __restrict__ ground_key, long S,
                                                      int* __restrict__ tile_counts, long ntile_all) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < S) {
        dropped[i] = 0;
        if (ground_key) ground_key[i] = 0x7fffffff;
    }
    if (i < ntile_all) tile_counts[i] = 0;
}

__global__ void __launch_bounds__(256) rs_setup_kernel(const float* __restrict__ positions, const int64_t* __restrict__ tri_offsets,
                                                       long S, long T, SgRasterParams M, int W, int H, int cull_back, float near_w,
                                                       SgRasterRec* __restrict__ recs, int* __restrict__ flags, float* __restrict__ clip,
                                                       int* __restrict__ dropped, int* __restrict__ ground_key,
                                                       int* __restrict__ tile_counts, int ntx, int nty) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    float p[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) p[k] = positions[t * 9 + k];
    SgRasterRec r;
    float c[12];
    const int f = sg_rs_setup(p, M.vp, W, H, cull_back, near_w, &r, c);
    recs[t] = r;
    flags[t] = f;
    if (clip)
#pragma unroll
        for (int k = 0; k < 12; ++k) clip[t * 12 + k] = c[k];
    const long s = rs_shape_of(tri_offsets, S, t);
    if (s < 0) return;
    if (ground_key) atomicMin(&ground_key[s], sg_float_key(fminf(fminf(p[1], p[4]), p[7])));
    if (f & SG_RS_DROPPED) atomicAdd(&dropped[s], 1);
    if (f) return;
    int* __restrict__ counts = tile_counts + s * (long)ntx * nty;
    for (int ty = r.py0 >> SG_RS_TILE_SHIFT; ty <= r.py1 >> SG_RS_TILE_SHIFT; ++ty)
        for (int tx = r.px0 >> SG_RS_TILE_SHIFT; tx <= r.px1 >> SG_RS_TILE_SHIFT; ++tx) atomicAdd(&counts[ty * ntx + tx], 1);
}

__global__ void __launch_bounds__(256) rs_ground_kernel(float* __restrict__ ground, long S) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= S) return;
    const int k = ((const int*)ground)[i];
    ground[i] = k == 0x7fffffff ? -1.0f : sg_key_float(k);
}

// One workgroup of 1024: lane l owns the contiguous run [l * per, (l + 1) * per) of the n tiles.
__global__ void __launch_bounds__(1024) rs_scan_kernel(const int* __restrict__ counts, long n, int64_t* __restrict__ offsets,
                                                       int* __restrict__ cursor, int* __restrict__ active, int64_t* __restrict__ totals) {
    __shared__ int64_t s_sum[1024];
    __shared__ int s_act[1024];
    const int l = threadIdx.x;
    const long per = (n + 1023) / 1024, i0 = l * per, i1 = i0 + per < n ? i0 + per : n;
    int64_t sum = 0;
    int act = 0;
    for (long i = i0; i < i1; ++i) {
        const int c = counts[i] > 0 ? counts[i] : 0;
        sum += c;
        act += c > 0;
    }
    s_sum[l] = sum;
    s_act[l] = act;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {      // inclusive scan, both at once
        const int64_t a = l >= off ? s_sum[l - off] : 0;
        const int b = l >= off ? s_act[l - off] : 0;
        __syncthreads();
        s_sum[l] += a;
        s_act[l] += b;
        __syncthreads();
    }
    int64_t run = s_sum[l] - sum;
    int slot = s_act[l] - act;
    for (long i = i0; i < i1; ++i) {
        const int c = counts[i] > 0 ? counts[i] : 0;
        offsets[i] = run;
        cursor[i] = 0;
        if (c > 0) active[slot++] = (int)i;
        run += c;
    }
    if (l == 1023) {
        offsets[n] = s_sum[1023];
        totals[0] = s_sum[1023];
        totals[1] = s_act[1023];
    }
}

__global__ void __launch_bounds__(256) rs_fill_kernel(const SgRasterRec* __restrict__ recs, const int* __restrict__ flags,
                                                      const int64_t* __restrict__ tri_offsets, long S, long T, int ntx, int nty,
                                                      const int64_t* __restrict__ offsets, int* __restrict__ cursor,
                                                      int* __restrict__ lists, long capacity) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= T || flags[t]) return;
    const long s = rs_shape_of(tri_offsets, S, t);
    if (s < 0) return;
    const int px0 = recs[t].px0, py0 = recs[t].py0, px1 = recs[t].px1, py1 = recs[t].py1;
    if (px0 < 0 || py0 < 0 || (px1 >> SG_RS_TILE_SHIFT) >= ntx || (py1 >> SG_RS_TILE_SHIFT) >= nty) return;
    const long base = s * (long)ntx * nty;
    for (int ty = py0 >> SG_RS_TILE_SHIFT; ty <= py1 >> SG_RS_TILE_SHIFT; ++ty)
        for (int tx = px0 >> SG_RS_TILE_SHIFT; tx <= px1 >> SG_RS_TILE_SHIFT; ++tx) {
            const long g = base + ty * ntx + tx;
            const long at = offsets[g] + atomicAdd(&cursor[g], 1);
            if (at >= offsets[g] && at < offsets[g + 1] && at < capacity) lists[at] = (int)t;
        }
}

__global__ void __launch_bounds__(256) rs_clear_kernel(int* __restrict__ id, float* __restrict__ depth, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (id) id[i] = -1;
    depth[i] = 1.0f;
}

struct RsStaged {      // 16 words: four ds_read_b128 per record
    int x[3], y[3];
    float z0, dz1, dz2, inv;
    int px0, py0, px1, py1, id, pad;
};

__global__ void __launch_bounds__(kRsBlock) rs_visibility_kernel(const SgRasterRec* __restrict__ recs,
                                                                 const int64_t* __restrict__ tri_offsets, long S, int W, int H, int ntx,
                                                                 int nty, const int64_t* __restrict__ offsets, const int* __restrict__ lists,
                                                                 long capacity, const int* __restrict__ active, long nactive,
                                                                 int* __restrict__ id_out, float* __restrict__ depth_out, int shadow) {
    __shared__ __attribute__((aligned(16))) RsStaged stage[SG_RS_CHUNK];
    const int tid = threadIdx.x;
    const long ntiles = (long)ntx * nty;
    const long g = active[blockIdx.x];
    if (g < 0 || g >= S * ntiles) return;      // an unwritten entry names no tile
    const long s = g / ntiles;
    const int tile = (int)(g - s * ntiles), tx = tile % ntx, ty = tile / ntx;
    const int px = tx * SG_RS_TILE + (tid & 15), py = ty * SG_RS_TILE + (tid >> 4);
    const int wy0 = ty * SG_RS_TILE + (tid >> 6) * 4, wx0 = tx * SG_RS_TILE;      // this wave's 16 x 4 samples
    const long t_lo = tri_offsets[s], t_hi = tri_offsets[s + 1];
    long begin = offsets[g], end = offsets[g + 1];
    begin = begin < 0 ? 0 : begin;
    end = end > capacity ? capacity : end;
    float best = __builtin_inff();
    int best_id = -1;
    for (long c0 = begin; c0 < end; c0 += SG_RS_CHUNK) {
        const int n = (int)(end - c0 < SG_RS_CHUNK ? end - c0 : SG_RS_CHUNK);
        __syncthreads();      // the previous chunk has been consumed
        if (tid < n) {
            const long t = lists[c0 + tid];
            RsStaged q;
            if (t >= t_lo && t < t_hi) {
                const SgRasterRec r = recs[t];
                const int64_t a2 = sg_rs_area2(r);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    q.x[k] = r.x[k];
                    q.y[k] = r.y[k];
                }
                q.z0 = r.z[0];
                q.dz1 = r.z[1] - r.z[0];
                q.dz2 = r.z[2] - r.z[0];
                q.inv = 1.0f / (float)(a2 < 0 ? -a2 : a2);
                q.px0 = r.px0, q.py0 = r.py0, q.px1 = r.px1, q.py1 = r.py1;
                q.id = (int)t;
            } else {      // not a triangle of this shape: an empty box, skipped by every wave
                q = RsStaged{};
                q.px0 = q.py0 = 1;
                q.px1 = q.py1 = 0;
                q.id = -1;
            }
            q.pad = 0;
            stage[tid] = q;
        }
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            const RsStaged& q = stage[k];
            if (q.px0 > q.px1 || q.px1 < wx0 || q.px0 > wx0 + 15 || q.py1 < wy0 || q.py0 > wy0 + 3) continue;      // the same in every lane
            int64_t e[3], a2;
            if (sg_rs_cover(q.x, q.y, px, py, e, &a2)) {
                const float z = sg_rs_depth(e, q.inv, q.z0, q.dz1, q.dz2);
                if (z < best || (z == best && q.id < best_id)) {
                    best = z;
                    best_id = q.id;
                }
            }
        }
    }
    if (px < W && py < H) {
        const long o = (s * H + py) * W + px;
        if (id_out) id_out[o] = best_id;
        depth_out[o] = best_id < 0 ? 1.0f : (shadow ? __builtin_fmaf(0.5f, best, 0.5f) : best);
    }
}

__global__ void __launch_bounds__(256) rs_shade_kernel(const float* __restrict__ positions, const float* __restrict__ normals, long T,
                                                       const SgRasterRec* __restrict__ recs, const int* __restrict__ id,
                                                       const float* __restrict__ depth, const float* __restrict__ smap, int N,
                                                       const float* __restrict__ ground, SgRasterParams P, long S, int W, int H,
                                                       unsigned char* __restrict__ image) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= S * H * W) return;
    const long s = i / ((long)H * W);
    const int rem = (int)(i - s * H * W), py = rem / W, px = rem - py * W;
    unsigned char rgb[3];
    sg_rs_shade(px, py, W, H, id[i], depth[i], T, recs, positions, normals, smap + s * (long)N * N, N, ground[s], P, rgb);
    image[i * 3] = rgb[0];
    image[i * 3 + 1] = rgb[1];
    image[i * 3 + 2] = rgb[2];
}

__global__ void __launch_bounds__(256) rs_resolve_kernel(const unsigned char* __restrict__ in, long S, int W, int H, int ss,
                                                         unsigned char* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= S * H * W * 3) return;
    const int c = (int)(i % 3);
    const long q = i / 3, s = q / ((long)H * W);
    const int rem = (int)(q - s * H * W), y = rem / W, x = rem - y * W;
    const long Wi = (long)W * ss;
    const unsigned char* __restrict__ src = in + ((s * H * ss + (long)y * ss) * Wi + (long)x * ss) * 3 + c;
    int sum = 0;
    for (int a = 0; a < ss; ++a)
        for (int b = 0; b < ss; ++b) sum += src[(a * Wi + b) * 3];
    const int n = ss * ss;
    out[i] = (unsigned char)((2 * sum + n) / (2 * n));
}

static inline bool rs_view_ok(long S, long T, int W, int H) {
    return S >= 1 && S <= 65535 && T >= 0 && T <= 2147483647L && W >= 1 && H >= 1 && W <= 16384 && H <= 16384 &&
           S * (long)sg_cdiv(W, SG_RS_TILE) * sg_cdiv(H, SG_RS_TILE) <= 2147483647L;
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_raster_setup(const float* positions, const int64_t* tri_offsets, long S, long T, const double* vp, int width, int height,
                    int cull_back, double near_w, int* recs, int* flags, float* clip, int* dropped, float* ground, int* tile_counts,
                    hipStream_t stream) {
    SG_CHECK_ARG(rs_view_ok(S, T, width, height) && tri_offsets && vp && dropped && tile_counts);
    SG_CHECK_ARG(T == 0 || (positions && recs && flags));
    SgRasterParams M;
    for (int i = 0; i < 16; ++i) M.vp[i] = (float)vp[i];
    const int ntx = sg_cdiv(width, SG_RS_TILE), nty = sg_cdiv(height, SG_RS_TILE);
    const long ntile_all = S * (long)ntx * nty, ninit = ntile_all > S ? ntile_all : S;
    hipLaunchKernelGGL(rs_init_kernel, dim3((unsigned)((ninit + 255) / 256)), dim3(256), 0, stream, dropped, (int*)ground, S, tile_counts,
                       ntile_all);
    if (T > 0)
        hipLaunchKernelGGL(rs_setup_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, stream, positions, tri_offsets, S, T, M,
                           width, height, cull_back, (float)near_w, (SgRasterRec*)recs, flags, clip, dropped, (int*)ground, tile_counts,
                           ntx, nty);
    if (ground) hipLaunchKernelGGL(rs_ground_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, stream, ground, S);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_raster_scan(const int* tile_counts, long ntiles, int64_t* tile_offsets, int* cursor, int* active, int64_t* totals,
                   hipStream_t stream) {
    SG_CHECK_ARG(tile_counts && tile_offsets && cursor && active && totals && ntiles >= 1 && ntiles <= 2147483647L);
    hipLaunchKernelGGL(rs_scan_kernel, dim3(1), dim3(1024), 0, stream, tile_counts, ntiles, tile_offsets, cursor, active, totals);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_raster_fill(const int* recs, const int* flags, const int64_t* tri_offsets, long S, long T, int width, int height,
                   const int64_t* tile_offsets, int* cursor, int* lists, long capacity, hipStream_t stream) {
    SG_CHECK_ARG(rs_view_ok(S, T, width, height) && tri_offsets && tile_offsets && cursor && capacity >= 0);
    if (T == 0 || capacity == 0) return SG_OK;
    SG_CHECK_ARG(recs && flags && lists);
    hipLaunchKernelGGL(rs_fill_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, stream, (const SgRasterRec*)recs, flags,
                       tri_offsets, S, T, sg_cdiv(width, SG_RS_TILE), sg_cdiv(height, SG_RS_TILE), tile_offsets, cursor, lists, capacity);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_raster_visibility(const int* recs, const int64_t* tri_offsets, long S, int width, int height, const int64_t* tile_offsets,
                         const int* lists, long capacity, const int* active, long nactive, int* id, float* depth, int shadow,
                         hipStream_t stream) {
    SG_CHECK_ARG(rs_view_ok(S, 0, width, height) && tri_offsets && tile_offsets && depth && capacity >= 0 && nactive >= 0);
    const int ntx = sg_cdiv(width, SG_RS_TILE), nty = sg_cdiv(height, SG_RS_TILE);
    SG_CHECK_ARG(nactive <= S * (long)ntx * nty && (nactive == 0 || (recs && lists && active)));
    const long n = S * (long)height * width;
    hipLaunchKernelGGL(rs_clear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, id, depth, n);
    if (nactive > 0)
        hipLaunchKernelGGL(rs_visibility_kernel, dim3((unsigned)nactive), dim3(kRsBlock), 0, stream, (const SgRasterRec*)recs,
                           tri_offsets, S, width, height, ntx, nty, tile_offsets, lists, capacity, active, nactive, id, depth, shadow);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_raster_shade(const float* positions, const float* normals, long T, const int* recs, const int* id, const float* depth,
                    const float* shadow_map, int shadow_size, const float* ground, const double* params, long S, int width, int height,
                    unsigned char* image, hipStream_t stream) {
    SG_CHECK_ARG(rs_view_ok(S, T, width, height) && id && depth && shadow_map && shadow_size >= 1 && shadow_size <= 16384 && ground &&
                 params && image);
    SG_CHECK_ARG(T == 0 || (positions && recs));
    SgRasterParams P;
    sg_rs_params_from_host(params, &P);
    const long n = S * (long)height * width;
    hipLaunchKernelGGL(rs_shade_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, positions, normals, T,
                       (const SgRasterRec*)recs, id, depth, shadow_map, shadow_size, ground, P, S, width, height, image);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_raster_resolve(const unsigned char* samples, long S, int width, int height, int ssaa, unsigned char* image, hipStream_t stream) {
    SG_CHECK_ARG(samples && image && S >= 1 && width >= 1 && height >= 1 && ssaa >= 1 && ssaa <= 16 &&
                 (long)width * ssaa <= 16384 && (long)height * ssaa <= 16384);
    const long n = S * (long)height * width * 3;
    hipLaunchKernelGGL(rs_resolve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, samples, S, width, height, ssaa, image);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

}  // extern "C"
