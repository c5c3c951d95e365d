// shapegan_amd/csrc/cloud.hip — signed distances from oriented point clouds (K19): k nearest neighbours, normals, the normal vote.
//
// mesh_to_sdf's sign_method = 'normal' (include/shapegan_hip.h has the contract).  The walk is chamfer_nearest's (csrc/pointcloud.hip)
// with a list in place of one minimum:
//   cloud_walk   one workgroup of 256 queries of ONE shape walks that shape's cloud.  The cloud passes through LDS as three planes
//                in chunks of SG_CLOUD_STAGE points; every lane reads the same address (ds_read_b128: four points per plane, a
//                broadcast without bank conflicts).  Each lane keeps its K best (d2, index) pairs SORTED IN REGISTERS: the form is
//                compiled for 8, 16 and 32 entries, every index into the list is a compile-time constant, so nothing goes to
//                scratch.  The common path of a pair is the six arithmetic steps of d2 and ONE compare against the list's last
//                entry; an insertion puts the pair there and lets it rise through a fully unrolled compare-exchange chain.  The
//                points come in increasing index order and the compares are strict, so equal distances stay in index order: the
//                list is the first K of the order (d2, index) whatever the chunking.  After the first stage a query inserts about
//                K ln(P / K) times in P points; the divergence of that branch is not what the kernel costs.
//                Epilogues: store the first K entries (sg_cloud_knn), or gather the K samples and their normals and vote
//                (sg_cloud_sdf).
//   cloud_normals  one lane per point: csrc/cloud_core.h does all of it.
// Plain vector stores only: no atomics, no scratch buffers, no inline assembly.  Lanes past the end of a query run compute on the
// run's last query and store nothing.
#include <vector>

#include "common.h"
#include "../../include/shapegan_hip.h"

// every value is compared bit for bit with the twin: the only fused steps are the explicit fmaf
#pragma clang fp contract(off)
#include "cloud_core.h"

namespace sg {

constexpr int kClBlock = SG_CLOUD_QUERY_TILE;
constexpr int kClStage = SG_CLOUD_STAGE;
static_assert(kClStage % 4 == 0 && kClBlock == 256, "the staging loop and the launch bounds assume these");

enum { kClLists = 0, kClVote = 1 };

template <int KT, int MODE>
__global__ void __launch_bounds__(kClBlock) cloud_walk_kernel(const float* __restrict__ points, const float* __restrict__ normals,
                                                              const int64_t* __restrict__ cloud_offsets,
                                                              const float* __restrict__ queries,
                                                              const int64_t* __restrict__ query_offsets, int K, int exclude_self,
                                                              int* __restrict__ idx, float* __restrict__ d2, float* __restrict__ sdf,
                                                              int* __restrict__ nearest) {
    __shared__ __attribute__((aligned(16))) float sb[3][kClStage];
    const int tid = threadIdx.x;
    const long s = blockIdx.y;
    const long c0 = cloud_offsets[s], P = cloud_offsets[s + 1] - c0;
    const long q0 = query_offsets[s], Q = query_offsets[s + 1] - q0;
    const long tile0 = (long)blockIdx.x * kClBlock;
    if (tile0 >= Q) return;                              // the whole workgroup: the grid is sized for the longest run
    const long ql = tile0 + tid;
    const bool live = ql < Q;
    const long qc = live ? ql : Q - 1;
    const float* __restrict__ cloud = points + c0 * 3;
    const float qx = queries[(q0 + qc) * 3], qy = queries[(q0 + qc) * 3 + 1], qz = queries[(q0 + qc) * 3 + 2];
    const int self = exclude_self ? (int)qc : -1;

    float ld[KT];
    int li[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) {
        ld[j] = __builtin_inff();
        li[j] = -1;
    }

    for (long p0 = 0; p0 < P; p0 += kClStage) {
        const int n = (int)(P - p0 < kClStage ? P - p0 : kClStage), n4 = (n + 3) & ~3;
        __syncthreads();                                 // the previous stage has been consumed
        for (int t = tid; t < n4; t += kClBlock) {
            const long src = (p0 + (t < n ? t : n - 1)) * 3;
            float x = cloud[src], y = cloud[src + 1], z = cloud[src + 2];
            if (t >= n) x = y = z = __builtin_nanf("");  // the tail: NaN is never smaller than anything
            sb[0][t] = x;
            sb[1][t] = y;
            sb[2][t] = z;
        }
        __syncthreads();
        for (int t = 0; t < n4; t += 4) {
            const f32x4 bx = *(const f32x4*)&sb[0][t], by = *(const f32x4*)&sb[1][t], bz = *(const f32x4*)&sb[2][t];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int pi = (int)p0 + t + u;
                const float d = sg_pc_d2(qx, qy, qz, bx[u], by[u], bz[u]);
                // strict: NaN and +inf never enter, and an equal distance (a higher index) never displaces the last entry
                if (d < ld[KT - 1] && pi != self) {
                    ld[KT - 1] = d;
                    li[KT - 1] = pi;
#pragma unroll
                    for (int j = KT - 1; j > 0; --j) {
                        const bool up = ld[j] < ld[j - 1];      // strict: behind every equal distance, whose index is lower
                        const float dl = ld[j - 1], dh = ld[j];
                        const int il = li[j - 1], ih = li[j];
                        ld[j - 1] = up ? dh : dl;
                        ld[j] = up ? dl : dh;
                        li[j - 1] = up ? ih : il;
                        li[j] = up ? il : ih;
                    }
                }
            }
        }
    }
    if (!live) return;
    const long row = q0 + ql;
    if (MODE == kClLists) {
#pragma unroll
        for (int j = 0; j < KT; ++j)
            if (j < K) {
                idx[row * K + j] = li[j];
                d2[row * K + j] = ld[j];
            }
    } else {
        int valid = 0, negative = 0;
#pragma unroll
        for (int j = 0; j < KT; ++j)
            if (j < K && li[j] >= 0) {
                const long g = (long)li[j] * 3;
                const float t = sg_cloud_vote(qx, qy, qz, cloud[g], cloud[g + 1], cloud[g + 2], normals[c0 * 3 + g],
                                              normals[c0 * 3 + g + 1], normals[c0 * 3 + g + 2]);
                ++valid;
                negative += t < 0.f ? 1 : 0;
            }
        sdf[row] = sg_cloud_signed(ld[0], valid, negative);
        if (nearest) nearest[row] = li[0];
    }
}

__global__ void __launch_bounds__(256) cloud_normals_kernel(const float* __restrict__ points, const int64_t* __restrict__ cloud_offsets,
                                                            long S, long N, const int* __restrict__ idx, int K,
                                                            const float* __restrict__ view, int view_per_point,
                                                            float* __restrict__ normals, float* __restrict__ variation) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    // the shape of point i: the last s with cloud_offsets[s] <= i (empty runs share an offset with their successor)
    long lo = 0, hi = S;
    while (hi - lo > 1) {
        const long mid = (lo + hi) >> 1;
        if (cloud_offsets[mid] <= i) lo = mid; else hi = mid;
    }
    const long c0 = cloud_offsets[lo], size = cloud_offsets[lo + 1] - c0;
    float nrm[3], var;
    sg_cloud_normal(points + c0 * 3, size, i - c0, idx + i * K, K, view ? view + (view_per_point ? i : lo) * 4 : nullptr, nrm, &var);
    normals[i * 3] = nrm[0];
    normals[i * 3 + 1] = nrm[1];
    normals[i * 3 + 2] = nrm[2];
    variation[i] = var;
}

// The runs of an offset table, read back from the device: false when they break the contract.  longest = the longest run.
static bool cloud_runs(const int64_t* offsets, long S, long total, hipStream_t stream, std::vector<int64_t>& host, long* longest) {
    host.resize((size_t)S + 1);
    if (hipMemcpyAsync(host.data(), offsets, ((size_t)S + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, stream) != hipSuccess) return false;
    if (hipStreamSynchronize(stream) != hipSuccess) return false;
    *longest = 0;
    if (host[0] != 0 || host[(size_t)S] != total) return false;
    for (long s = 0; s < S; ++s) {
        const int64_t n = host[(size_t)s + 1] - host[(size_t)s];
        if (n < 0 || n > SG_CLOUD_MAX_POINTS) return false;
        *longest = n > *longest ? (long)n : *longest;
    }
    return true;
}

template <int MODE>
static int cloud_walk(const float* points, const float* normals, const int64_t* cloud_offsets, const float* queries,
                      const int64_t* query_offsets, long S, long N, long M, int K, int exclude_self, int* idx, float* d2, float* sdf,
                      int* nearest, hipStream_t stream, const char* entry) {
    std::vector<int64_t> co, qo;
    long longest_cloud = 0, longest_query = 0;
    if (!cloud_runs(cloud_offsets, S, N, stream, co, &longest_cloud) || !cloud_runs(query_offsets, S, M, stream, qo, &longest_query))
        SG_FAIL(SG_ERR_ARG, "%s: the offsets do not describe S runs of at most 2^26 points that end at N / M", entry);
    if (exclude_self && co != qo) SG_FAIL(SG_ERR_ARG, "%s: exclude_self needs query runs equal to the cloud runs", entry);
    if (longest_query == 0) return SG_OK;
    const dim3 grid((unsigned)((longest_query + kClBlock - 1) / kClBlock), (unsigned)S), block(kClBlock);
    if (K <= 8)
        hipLaunchKernelGGL((cloud_walk_kernel<8, MODE>), grid, block, 0, stream, points, normals, cloud_offsets, queries, query_offsets, K,
                           exclude_self, idx, d2, sdf, nearest);
    else if (K <= 16)
        hipLaunchKernelGGL((cloud_walk_kernel<16, MODE>), grid, block, 0, stream, points, normals, cloud_offsets, queries, query_offsets, K,
                           exclude_self, idx, d2, sdf, nearest);
    else
        hipLaunchKernelGGL((cloud_walk_kernel<32, MODE>), grid, block, 0, stream, points, normals, cloud_offsets, queries, query_offsets, K,
                           exclude_self, idx, d2, sdf, nearest);
    return SG_OK;
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_cloud_knn(const float* points, const int64_t* cloud_offsets, const float* queries, const int64_t* query_offsets, long S, long N,
                 long M, int K, int exclude_self, int* idx, float* d2, hipStream_t stream) {
    SG_CHECK_ARG(S >= 1 && S <= 65535 && N >= 0 && M >= 0 && K >= 1 && K <= SG_CLOUD_MAX_K && cloud_offsets && query_offsets);
    SG_CHECK_ARG((points || N == 0) && (queries || M == 0) && ((idx && d2) || M == 0));
    const int rc = cloud_walk<kClLists>(points, nullptr, cloud_offsets, queries, query_offsets, S, N, M, K, exclude_self, idx, d2, nullptr,
                                        nullptr, stream, __func__);
    if (rc != SG_OK) return rc;
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_cloud_normals(const float* points, const int64_t* cloud_offsets, long S, long N, const int* idx, int K, const float* view,
                     int view_per_point, float* normals, float* variation, hipStream_t stream) {
    SG_CHECK_ARG(S >= 1 && S <= 65535 && N >= 0 && K >= 1 && K <= SG_CLOUD_MAX_K && cloud_offsets);
    SG_CHECK_ARG((points && idx && normals && variation) || N == 0);
    std::vector<int64_t> co;
    long longest = 0;
    if (!cloud_runs(cloud_offsets, S, N, stream, co, &longest))
        SG_FAIL(SG_ERR_ARG, "%s: the offsets do not describe S runs of at most 2^26 points that end at N", __func__);
    if (N == 0) return SG_OK;
    hipLaunchKernelGGL(cloud_normals_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, points, cloud_offsets, S, N, idx, K,
                       view, view_per_point, normals, variation);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_cloud_sdf(const float* points, const float* normals, const int64_t* cloud_offsets, const float* queries,
                 const int64_t* query_offsets, long S, long N, long M, int K, float* sdf, int* nearest, hipStream_t stream) {
    SG_CHECK_ARG(S >= 1 && S <= 65535 && N >= 0 && M >= 0 && K >= 1 && K <= SG_CLOUD_MAX_K && cloud_offsets && query_offsets);
    SG_CHECK_ARG(((points && normals) || N == 0) && ((queries && sdf) || M == 0));
    const int rc = cloud_walk<kClVote>(points, normals, cloud_offsets, queries, query_offsets, S, N, M, K, 0, nullptr, nullptr, sdf, nearest,
                                       stream, __func__);
    if (rc != SG_OK) return rc;
    SG_CHECK_LAUNCH();
    return SG_OK;
}

}  // extern "C"
