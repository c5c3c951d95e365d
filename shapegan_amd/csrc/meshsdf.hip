// shapegan_amd/csrc/meshsdf.hip — meshes to signed distances (K16): brute-force point-triangle distances and the sign from depth scans.
//
// Distance, three launches and one fill:
//   records   one lane per triangle: the 32-float record of csrc/meshsdf_core.h (corners, edges, reciprocal squared lengths, the two
//             gradient vectors of the face weights), written once per call into the workspace;
//   distance  grid (blocks of queries) x (split) x S, 256 lanes, QPL = 1, 2 or 4 queries per lane in registers.  A workgroup walks its run of the
//             shape's triangles in chunks of SG_MESHSDF_CHUNK records staged in LDS (32 KB); every lane reads the SAME record, a
//             broadcast, so a record costs eight wide LDS reads per wave whatever the lanes hold, shared by the lane's queries.  The
//             running minimum and its index stay in registers; at the end each query meets the other runs of its shape in ONE 64-bit
//             atomicMin on (bits(d2) << 32 | index).
//   finish    one lane per query: unpacks the word and re-evaluates the winning triangle through the same core function for its
//             closest point.
// The packed words are set to all ones by the entry point itself (hipMemsetAsync), so nothing depends on what the workspace held.
// Sizes: 4 queries per lane keep the LDS reads at 0.3 of the VALU issue time; the split is chosen so that the grid has at
// least kTargetBlocks workgroups (4 per CU, 4 waves per SIMD) wherever the triangles allow it.
// Sign: one lane per point, a loop over the scans with an early exit at the first that sees the point; gather-bound and small.
#include "common.h"
#include "../../include/shapegan_hip.h"

#pragma clang fp contract(off)
#include "meshsdf_core.h"

namespace sg {

constexpr int kMsdfBlock = 256;
constexpr int kMsdfChunk = SG_MESHSDF_CHUNK;
constexpr int kMsdfTargetBlocks = 1024;
constexpr int kMsdfRecVec = sizeof(SgMsdfRec) / sizeof(f32x4);
static_assert(sizeof(SgMsdfRec) == 128 && kMsdfRecVec == 8, "eight 16-byte rows per record");
constexpr unsigned long long kMsdfNone = ~0ull;

__global__ void __launch_bounds__(kMsdfBlock) msdf_records_kernel(const float* __restrict__ positions, long T, SgMsdfRec* __restrict__ recs) {
    const long t = (long)blockIdx.x * kMsdfBlock + threadIdx.x;
    if (t >= T) return;
    float tri[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) tri[i] = positions[t * 9 + i];
    SgMsdfRec r;
    sg_msdf_record(tri, &r);
    recs[t] = r;
}

template <int QPL>
__global__ void __launch_bounds__(kMsdfBlock) msdf_distance_kernel(const SgMsdfRec* __restrict__ recs, const int64_t* __restrict__ tri_offsets,
                                                                  long T, const float* __restrict__ points, long Q,
                                                                  unsigned long long* __restrict__ packed) {
    __shared__ SgMsdfRec sh[kMsdfChunk];
    const int tid = threadIdx.x;
    const long s = blockIdx.z;
    long t0 = tri_offsets[s], t1 = tri_offsets[s + 1];
    t0 = t0 < 0 ? 0 : t0;
    t1 = t1 > T ? T : t1;
    const long n = t1 - t0;
    if (n <= 0) return;                                 // uniform: the words of an empty shape stay all ones
    const long nchunks = (n + kMsdfChunk - 1) / kMsdfChunk, per = (nchunks + gridDim.y - 1) / gridDim.y;
    const long c0 = (long)blockIdx.y * per, c1 = c0 + per < nchunks ? c0 + per : nchunks;
    if (c0 >= c1) return;

    const long q0 = (long)blockIdx.x * (kMsdfBlock * QPL) + tid;
    float px[QPL], py[QPL], pz[QPL], best[QPL];
    int arg[QPL];
#pragma unroll
    for (int j = 0; j < QPL; ++j) {
        long q = q0 + (long)j * kMsdfBlock;
        q = q < Q ? q : Q - 1;                          // a slot beyond the points computes on the last one and stores nothing
        const float* p = points + (s * Q + q) * 3;
        px[j] = p[0], py[j] = p[1], pz[j] = p[2];
        best[j] = INFINITY;
        arg[j] = -1;
    }

    for (long c = c0; c < c1; ++c) {
        const long first = c * kMsdfChunk;
        const int cnt = (int)(n - first < kMsdfChunk ? n - first : kMsdfChunk);
        __syncthreads();                                // the previous chunk has been read by every lane
        const f32x4* src = (const f32x4*)(recs + t0 + first);
        f32x4* dst = (f32x4*)sh;
        for (int i = tid; i < cnt * kMsdfRecVec; i += kMsdfBlock) dst[i] = src[i];
        __syncthreads();
        const int base = (int)first;
#pragma unroll 2
        for (int i = 0; i < cnt; ++i) {
            const SgMsdfRec& r = sh[i];
#pragma unroll
            for (int j = 0; j < QPL; ++j) {
                const float d2 = sg_msdf_d2(px[j], py[j], pz[j], r, nullptr);
                const bool lt = d2 < best[j];           // strict, increasing index: the lowest index of a tie stays
                best[j] = lt ? d2 : best[j];
                arg[j] = lt ? base + i : arg[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < QPL; ++j) {
        const long q = q0 + (long)j * kMsdfBlock;
        if (q < Q && arg[j] >= 0)
            atomicMin(&packed[s * Q + q], ((unsigned long long)__builtin_bit_cast(unsigned, best[j]) << 32) | (unsigned)arg[j]);
    }
}

__global__ void __launch_bounds__(kMsdfBlock) msdf_finish_kernel(const SgMsdfRec* __restrict__ recs, const int64_t* __restrict__ tri_offsets,
                                                                long T, const float* __restrict__ points, long Q, long SQ,
                                                                const unsigned long long* __restrict__ packed, float* __restrict__ dist2,
                                                                int* __restrict__ tri, float* __restrict__ closest) {
    const long i = (long)blockIdx.x * kMsdfBlock + threadIdx.x;
    if (i >= SQ) return;
    const unsigned long long word = packed[i];
    float d2 = INFINITY, c[3] = {0.f, 0.f, 0.f};
    int t = -1;
    if (word != kMsdfNone) {
        const long s = i / Q;
        long t0 = tri_offsets[s], t1 = tri_offsets[s + 1];
        t0 = t0 < 0 ? 0 : t0;
        t1 = t1 > T ? T : t1;
        const long local = (long)(unsigned)word;
        if (local < t1 - t0) {                          // always, for a word this call's distance kernel wrote
            d2 = __builtin_bit_cast(float, (unsigned)(word >> 32));
            t = (int)local;
            if (closest) sg_msdf_d2(points[i * 3], points[i * 3 + 1], points[i * 3 + 2], recs[t0 + local], c);
        }
    }
    dist2[i] = d2;
    if (tri) tri[i] = t;
    if (closest) closest[i * 3] = c[0], closest[i * 3 + 1] = c[1], closest[i * 3 + 2] = c[2];
}

struct MsdfViews {
    float m[SG_MESHSDF_MAX_SCANS][12];
};

__global__ void __launch_bounds__(kMsdfBlock) msdf_sign_kernel(const float* __restrict__ points, long S, long Q, const float* __restrict__ depth,
                                                              MsdfViews views, int K, int N, float bias, const float* __restrict__ dist2,
                                                              float* __restrict__ sdf, unsigned char* __restrict__ outside) {
    const long i = (long)blockIdx.x * kMsdfBlock + threadIdx.x;
    if (i >= S * Q) return;
    const long s = i / Q;
    const float x = points[i * 3], y = points[i * 3 + 1], z = points[i * 3 + 2];
    bool seen = false;
    for (int k = 0; k < K && !seen; ++k) seen = sg_msdf_visible(views.m[k], x, y, z, depth + ((long)k * S + s) * N * N, N, bias);
    if (outside) outside[i] = seen ? 1 : 0;
    if (sdf) {
        const float d = sqrtf(dist2[i]);
        sdf[i] = seen ? d : -d;
    }
}

static size_t msdf_recs_bytes(long T) { return ((size_t)T * sizeof(SgMsdfRec) + 255) & ~(size_t)255; }

static int msdf_split(long S, long T, long Q, int qpl, int requested) {
    const long chunks = T > 0 ? (T + kMsdfChunk - 1) / kMsdfChunk : 1;
    long split = requested;
    if (split <= 0) {
        const long blocks = S * ((Q + kMsdfBlock * qpl - 1) / (kMsdfBlock * qpl));
        split = (kMsdfTargetBlocks + blocks - 1) / blocks;
    }
    split = split > chunks ? chunks : split;
    return (int)(split > 65535 ? 65535 : split);
}

}  // namespace sg

using namespace sg;

extern "C" {

size_t sg_meshsdf_distance_workspace_bytes(long S, long T, long Q) {
    if (!sg_msdf_sizes_ok(S, T, Q)) return 0;
    return msdf_recs_bytes(T) + (size_t)(S * Q) * sizeof(unsigned long long);
}

int sg_meshsdf_distance_impl(const float* positions, const int64_t* tri_offsets, long S, long T, const float* points, long Q,
                             float* dist2, int* tri, float* closest, void* workspace, size_t workspace_bytes, int split, int* chosen,
                             hipStream_t stream) {
    if (!sg_msdf_sizes_ok(S, T, Q))
        SG_FAIL(SG_ERR_ARG, "%s: 1 <= S <= 65535, 0 <= T <= 2^24, 1 <= Q <= 2^24, S Q <= 2^28; got S = %ld, T = %ld, Q = %ld", __func__, S, T, Q);
    SG_CHECK_ARG(tri_offsets && points && dist2 && workspace && (T == 0 || positions));
    if (workspace_bytes < sg_meshsdf_distance_workspace_bytes(S, T, Q)) SG_FAIL(SG_ERR_WORKSPACE, "%s: workspace too small", __func__);
    SgMsdfRec* recs = (SgMsdfRec*)workspace;
    unsigned long long* packed = (unsigned long long*)((char*)workspace + msdf_recs_bytes(T));
    const long SQ = S * Q;
    // Q <= 256: one query per lane; <= 512: two; else four (a lane's slots beyond Q would compute for nothing)
    const int qpl = Q <= kMsdfBlock ? 1 : (Q <= 2 * kMsdfBlock ? 2 : 4);
    const int used = msdf_split(S, T, Q, qpl, split);
    if (chosen) *chosen = used;
    if (hipMemsetAsync(packed, 0xFF, (size_t)SQ * sizeof(unsigned long long), stream) != hipSuccess)
        SG_FAIL(SG_ERR_HIP, "%s: hipMemsetAsync failed", __func__);
    if (T > 0) {
        hipLaunchKernelGGL(msdf_records_kernel, dim3(sg_cdiv(T, kMsdfBlock)), dim3(kMsdfBlock), 0, stream, positions, T, recs);
        SG_CHECK_LAUNCH();
        const dim3 grid((unsigned)sg_cdiv(Q, kMsdfBlock * qpl), (unsigned)used, (unsigned)S);
        if (qpl == 1) hipLaunchKernelGGL(msdf_distance_kernel<1>, grid, dim3(kMsdfBlock), 0, stream, recs, tri_offsets, T, points, Q, packed);
        else if (qpl == 2) hipLaunchKernelGGL(msdf_distance_kernel<2>, grid, dim3(kMsdfBlock), 0, stream, recs, tri_offsets, T, points, Q, packed);
        else hipLaunchKernelGGL(msdf_distance_kernel<4>, grid, dim3(kMsdfBlock), 0, stream, recs, tri_offsets, T, points, Q, packed);
        SG_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(msdf_finish_kernel, dim3(sg_cdiv(SQ, kMsdfBlock)), dim3(kMsdfBlock), 0, stream, recs, tri_offsets, T, points, Q, SQ,
                       packed, dist2, tri, closest);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_meshsdf_distance(const float* positions, const int64_t* tri_offsets, long S, long T, const float* points, long Q, float* dist2,
                        int* tri, float* closest, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    return sg_meshsdf_distance_impl(positions, tri_offsets, S, T, points, Q, dist2, tri, closest, workspace, workspace_bytes, 0, nullptr,
                                    stream);
}

int sg_meshsdf_sign(const float* points, long S, long Q, const float* depth, const double* vps, int K, int N, float bias,
                    const float* dist2, float* sdf, unsigned char* outside, hipStream_t stream) {
    if (!sg_msdf_sizes_ok(S, 0, Q)) SG_FAIL(SG_ERR_ARG, "%s: 1 <= S <= 65535, 1 <= Q <= 2^24, S Q <= 2^28; got S = %ld, Q = %ld", __func__, S, Q);
    if (!sg_msdf_scans_ok(vps, K, N, bias))
        SG_FAIL(SG_ERR_ARG, "%s: 1 <= K <= %d orthographic views (row 3 = 0 0 0 1), 1 <= N <= 16384, a finite bias >= 0", __func__,
                SG_MESHSDF_MAX_SCANS);
    SG_CHECK_ARG(points && depth && (sdf != nullptr) == (dist2 != nullptr) && (sdf || outside));
    MsdfViews views;
    memset(&views, 0, sizeof(views));
    for (int k = 0; k < K; ++k)
        for (int i = 0; i < 12; ++i) views.m[k][i] = (float)vps[k * 16 + i];
    hipLaunchKernelGGL(msdf_sign_kernel, dim3(sg_cdiv(S * Q, kMsdfBlock)), dim3(kMsdfBlock), 0, stream, points, S, Q, depth, views, K, N, bias,
                       dist2, sdf, outside);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

}  // extern "C"
