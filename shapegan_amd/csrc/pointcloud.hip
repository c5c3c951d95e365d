// shapegan_amd/csrc/pointcloud.hip — point-cloud evaluation (K13): Chamfer matrices, nearest neighbours, occupancy histograms.
//
// The consumer of metrics.py:18-46: the clouds sample_point_clouds / sample_from_voxels produce are scored here instead of in an
// outside tool.  A 1000 x 1000 matrix of 2048-point clouds is 4.2e12 point pairs, all on the f32 vector pipe:
//   chamfer_rows   one workgroup holds 2048 points of ONE cloud A_i in registers (8 per lane, as four float2 so that the six
//                  arithmetic steps of a pair issue as v_pk_*_f32 on two points at once) and walks the clouds B_j of its share of
//                  the row.  B_j sits in LDS as three planes; every lane reads the same address (ds_read_b128: four points per
//                  plane, a broadcast without bank conflicts).  The running minima stay in registers; after a cloud the
//                  workgroup adds them in float64 in the order include/shapegan_hip.h fixes and stores one per-tile sum.
//   chamfer_mean   adds the per-tile sums of an entry in increasing tile order and divides.
// The column minima (ba) come from a SECOND sweep of the same kernel with the roles of A and B exchanged: d2 is bitwise
// symmetric, so the sweep yields the bits a column reduction would, with no cross-lane work and no atomics (DESIGN 3.9 costs
// the alternatives).
//   chamfer_nearest  the same walk for matched batches with (d2, index) pairs, 4 points per lane; the strict `<` in increasing
//                  index order keeps the lowest index of a tie.
//   occupancy_histogram  one lane per point, 64-bit integer atomics.
#include "common.h"
#include "../../include/shapegan_hip.h"

// d2 is compared bit for bit with the twin: the only fused steps are the two explicit fmaf
#pragma clang fp contract(off)
#include "pointcloud_core.h"   // d2 and the occupancy cell, shared with the twin

namespace sg {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kCdBlock = 256;
constexpr int kCdK = 8;                          // points of A per lane (chamfer_rows)
constexpr int kCdTileA = kCdBlock * kCdK;        // 2048: the tile of the summation order in the header
constexpr int kCdTileB = 2048;                   // points of B per LDS stage: 3 planes x 8 KB
constexpr int kNnK = 4;                          // points of A per lane (chamfer_nearest)
constexpr int kNnTileA = kCdBlock * kNnK;
constexpr long kCdGridLimit = 65535;

// Stages `n` points (n <= kCdTileB) of cloud b from point q0 into the three planes, rounded up to a multiple of 4: the tail
// repeats the last point (a duplicate changes no minimum) or, for the index kernel, is NaN (never smaller than anything).
template <bool NanTail>
__device__ __forceinline__ void stage_b(float (*sb)[kCdTileB], const float* __restrict__ b, long q0, int n, int n4) {
    for (int t = threadIdx.x; t < n4; t += kCdBlock) {
        const long src = (q0 + (t < n ? t : n - 1)) * 3;
        float x = b[src], y = b[src + 1], z = b[src + 2];
        if (NanTail && t >= n) x = y = z = __builtin_nanf("");
        sb[0][t] = x;
        sb[1][t] = y;
        sb[2][t] = z;
    }
}

// partial[(i * Sb + j) * tiles + tile] = the header's T[tile] of the minima of A_i's points against B_j
__global__ void __launch_bounds__(kCdBlock) chamfer_rows_kernel(const float* __restrict__ A, const float* __restrict__ B, long P,
                                                                long Q, long Sb, double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float sb[3][kCdTileB];
    __shared__ double red[kCdBlock];
    const int tid = threadIdx.x;
    const long tile = blockIdx.x, tiles = gridDim.x, i = blockIdx.y;
    const long j0 = (long)blockIdx.z * Sb / gridDim.z, j1 = ((long)blockIdx.z + 1) * Sb / gridDim.z;
    const float* __restrict__ a = A + i * P * 3;
    const long p0 = tile * kCdTileA + tid;           // this lane's points: p0 + k * 256

    f32x2 ax[kCdK / 2], ay[kCdK / 2], az[kCdK / 2];
#pragma unroll
    for (int k = 0; k < kCdK; ++k) {
        const long p = p0 + (long)k * kCdBlock;
        const long pc = (p < P ? p : P - 1) * 3;     // lanes beyond the cloud compute on its last point and are left out of the sum
        ax[k >> 1][k & 1] = a[pc];
        ay[k >> 1][k & 1] = a[pc + 1];
        az[k >> 1][k & 1] = a[pc + 2];
    }

    for (long j = j0; j < j1; ++j) {
        const float* __restrict__ b = B + j * Q * 3;
        f32x2 mn[kCdK / 2];
#pragma unroll
        for (int k = 0; k < kCdK / 2; ++k) mn[k] = (f32x2)(__builtin_inff());
        for (long q0 = 0; q0 < Q; q0 += kCdTileB) {
            const int n = (int)(Q - q0 < kCdTileB ? Q - q0 : kCdTileB), n4 = (n + 3) & ~3;
            __syncthreads();                         // the previous stage has been consumed
            stage_b<false>(sb, b, q0, n, n4);
            __syncthreads();
            for (int q = 0; q < n4; q += 4) {
                const f32x4 bx = *(const f32x4*)&sb[0][q], by = *(const f32x4*)&sb[1][q], bz = *(const f32x4*)&sb[2][q];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
#pragma unroll
                    for (int k = 0; k < kCdK / 2; ++k) {
                        // sg_pc_d2 (pointcloud_core.h) on two points at once: the packed form has no scalar statement to share
                        const f32x2 dx = ax[k] - (f32x2)(bx[u]), dy = ay[k] - (f32x2)(by[u]), dz = az[k] - (f32x2)(bz[u]);
                        const f32x2 d = __builtin_elementwise_fma(dz, dz, __builtin_elementwise_fma(dy, dy, dx * dx));
                        mn[k] = __builtin_elementwise_min(mn[k], d);
                    }
                }
            }
        }
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < kCdK; ++k)
            if (p0 + (long)k * kCdBlock < P) s += (double)mn[k >> 1][k & 1];
        red[tid] = s;
        __syncthreads();
#pragma unroll
        for (int off = kCdBlock / 2; off > 0; off >>= 1) {
            if (tid < off) red[tid] += red[tid + off];
            __syncthreads();
        }
        if (tid == 0) partial[(i * Sb + j) * tiles + tile] = red[0];
    }
}

// out[i * si + j * sj] = (partial[(i * Sb + j) * tiles + 0] + ... in increasing tile order) / n
__global__ void __launch_bounds__(256) chamfer_mean_kernel(const double* __restrict__ partial, long Sa, long Sb, long tiles, long n,
                                                           long si, long sj, double* __restrict__ out) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= Sa * Sb) return;
    double s = 0.0;
    for (long t = 0; t < tiles; ++t) s += partial[e * tiles + t];
    out[(e / Sb) * si + (e % Sb) * sj] = s / (double)n;
}

__global__ void __launch_bounds__(kCdBlock) chamfer_nearest_kernel(const float* __restrict__ A, const float* __restrict__ B, long P,
                                                                   long Q, float* __restrict__ dist, int* __restrict__ idx) {
    __shared__ __attribute__((aligned(16))) float sb[3][kCdTileB];
    const int tid = threadIdx.x;
    const long s = blockIdx.y;
    const float* __restrict__ a = A + s * P * 3;
    const float* __restrict__ b = B + s * Q * 3;
    const long p0 = (long)blockIdx.x * kNnTileA + tid;
    float ax[kNnK], ay[kNnK], az[kNnK], best[kNnK];
    int arg[kNnK];
#pragma unroll
    for (int k = 0; k < kNnK; ++k) {
        const long p = p0 + (long)k * kCdBlock;
        const long pc = (p < P ? p : P - 1) * 3;
        ax[k] = a[pc];
        ay[k] = a[pc + 1];
        az[k] = a[pc + 2];
        best[k] = __builtin_inff();
        arg[k] = 0;                                  // stays in range when nothing compares smaller (non-finite input)
    }
    for (long q0 = 0; q0 < Q; q0 += kCdTileB) {
        const int n = (int)(Q - q0 < kCdTileB ? Q - q0 : kCdTileB), n4 = (n + 3) & ~3;
        __syncthreads();
        stage_b<true>(sb, b, q0, n, n4);
        __syncthreads();
        for (int q = 0; q < n4; q += 4) {
            const f32x4 bx = *(const f32x4*)&sb[0][q], by = *(const f32x4*)&sb[1][q], bz = *(const f32x4*)&sb[2][q];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int qi = (int)q0 + q + u;
#pragma unroll
                for (int k = 0; k < kNnK; ++k) {
                    const float d = sg_pc_d2(ax[k], ay[k], az[k], bx[u], by[u], bz[u]);
                    const bool lt = d < best[k];     // increasing index, strict: the lowest index of a tie stays
                    best[k] = lt ? d : best[k];
                    arg[k] = lt ? qi : arg[k];
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kNnK; ++k) {
        const long p = p0 + (long)k * kCdBlock;
        if (p < P) {
            dist[s * P + p] = best[k];
            idx[s * P + p] = arg[k];
        }
    }
}

__global__ void __launch_bounds__(256) occupancy_histogram_kernel(const float* __restrict__ pts, long n, int R,
                                                                  unsigned long long* __restrict__ hist) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float rm1 = (float)(R - 1);
    const int ix = sg_pc_occupancy_axis(pts[i * 3], rm1), iy = sg_pc_occupancy_axis(pts[i * 3 + 1], rm1), iz = sg_pc_occupancy_axis(pts[i * 3 + 2], rm1);
    atomicAdd(&hist[((long)ix * R + iy) * R + iz], 1ull);
}

static inline long cd_tiles(long n) { return (n + kCdTileA - 1) / kCdTileA; }

// one sweep: out[i * si + j * sj] for the clouds A_i (n = P points each) against B_j
static void chamfer_sweep(const float* A, const float* B, long Sa, long Sb, long P, long Q, long si, long sj, double* out,
                          double* partial, hipStream_t stream) {
    const long tiles = cd_tiles(P);
    // enough workgroups to fill the device several times over: rows that are few are split along B
    long split = (4096 + Sa * tiles - 1) / (Sa * tiles);
    split = split < 1 ? 1 : (split > Sb ? Sb : split);
    hipLaunchKernelGGL(chamfer_rows_kernel, dim3((unsigned)tiles, (unsigned)Sa, (unsigned)split), dim3(kCdBlock), 0, stream, A, B, P,
                       Q, Sb, partial);
    hipLaunchKernelGGL(chamfer_mean_kernel, dim3((unsigned)((Sa * Sb + 255) / 256)), dim3(256), 0, stream, (const double*)partial,
                       Sa, Sb, tiles, P, si, sj, out);
}

static bool cd_sizes_ok(long Sa, long Sb, long P, long Q) {
    return Sa >= 1 && Sb >= 1 && P >= 1 && Q >= 1 && Sa <= kCdGridLimit && Sb <= kCdGridLimit && P <= (1L << 26) && Q <= (1L << 26);
}

}  // namespace sg

using namespace sg;

extern "C" {

size_t sg_chamfer_matrix_workspace_bytes(long Sa, long Sb, long P, long Q) {
    if (!cd_sizes_ok(Sa, Sb, P, Q)) return 0;
    const long tiles = cd_tiles(P) > cd_tiles(Q) ? cd_tiles(P) : cd_tiles(Q);
    return (size_t)(Sa * Sb * tiles) * sizeof(double);
}

int sg_chamfer_matrix(const float* A, const float* B, long Sa, long Sb, long P, long Q, double* ab, double* ba, void* workspace,
                      size_t workspace_bytes, hipStream_t stream) {
    SG_CHECK_ARG(cd_sizes_ok(Sa, Sb, P, Q));
    SG_CHECK_ARG(A && B && workspace && (ab || ba));
    if (workspace_bytes < sg_chamfer_matrix_workspace_bytes(Sa, Sb, P, Q))
        SG_FAIL(SG_ERR_WORKSPACE, "sg_chamfer_matrix: workspace too small");
    // the two sweeps share the workspace: they are ordered on the stream
    if (ab) chamfer_sweep(A, B, Sa, Sb, P, Q, Sb, 1, ab, (double*)workspace, stream);
    if (ba) chamfer_sweep(B, A, Sb, Sa, Q, P, 1, Sb, ba, (double*)workspace, stream);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_chamfer_nearest(const float* A, const float* B, long S, long P, long Q, float* dist_a, int* idx_a, float* dist_b, int* idx_b,
                       hipStream_t stream) {
    SG_CHECK_ARG(A && B && S >= 1 && S <= kCdGridLimit && P >= 1 && Q >= 1 && P <= (1L << 26) && Q <= (1L << 26));
    SG_CHECK_ARG((dist_a != nullptr) == (idx_a != nullptr) && (dist_b != nullptr) == (idx_b != nullptr) && (dist_a || dist_b));
    if (dist_a)
        hipLaunchKernelGGL(chamfer_nearest_kernel, dim3((unsigned)((P + kNnTileA - 1) / kNnTileA), (unsigned)S), dim3(kCdBlock), 0,
                           stream, A, B, P, Q, dist_a, idx_a);
    if (dist_b)
        hipLaunchKernelGGL(chamfer_nearest_kernel, dim3((unsigned)((Q + kNnTileA - 1) / kNnTileA), (unsigned)S), dim3(kCdBlock), 0,
                           stream, B, A, Q, P, dist_b, idx_b);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_occupancy_histogram(const float* clouds, long S, long P, int R, int64_t* hist, hipStream_t stream) {
    SG_CHECK_ARG(clouds && hist && S >= 1 && P >= 1 && R >= 2 && R <= 1024 && S * P <= (1L << 38));
    const long n = S * P;
    hipLaunchKernelGGL(occupancy_histogram_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, clouds, n, R,
                       (unsigned long long*)hist);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

}  // extern "C"
