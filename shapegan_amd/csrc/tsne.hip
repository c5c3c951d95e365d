// shapegan_amd/csrc/tsne.hip — exact t-SNE of a latent table (K17; serves shapegan_amd/traversal.py tsne).
//
// reference: demo_latent_space.py:58-60 and create_plot.py:88-96 embed every latent code with scikit-learn's TSNE on the host.  Here
// the exact gradient runs on the GPU: for N codes in 2-D one iteration is one pass over the N x N joint probabilities, a handful of
// flops per pair, nothing stored per pair.
//
// Affinities (once per embedding; every kernel works in place in P):
//   dist        64 x 64 tile of squared distances per workgroup, 4 x 4 per lane, 16 coordinates at a time through LDS
//   search      one workgroup per row: the minimum, then the search for beta (two float64 sums per evaluation, reduced in a fixed order;
//               every lane takes the same decision from the same sums), then the row becomes p_j|i
//   symmetrize  32 x 32 tile pairs (t, u), t <= u, transposed through LDS: one lane owns P[i][j] and P[j][i]
//   plogp       one workgroup per row, then one workgroup over the rows
// Gradient (every iteration), three launches:
//   rows        a workgroup of 256 lanes owns kTsneRows = 4 rows of P and walks their columns together, so a lane's y_j serves four
//               pairs: per 16 B of P it loads 8 B of Y (from L2: Y is 8 N bytes).  With N a multiple of 4 a lane reads float4 of P
//               (a wave 1 KB of a row per instruction), otherwise dwords (rows are then not 16-byte aligned).  The six sums of a row
//               are float over SG_TSNE_FLUSH pairs per lane, flushed into float64 registers (a pass of the workgroup covers
//               256 x SG_TSNE_FLUSH = 4096 columns); at the end 24 float64 go through a wave
//               butterfly and four LDS slots, added in wave order.  Nothing is atomic.  At large N the kernel streams P once
//               (bandwidth-bound: ~16 VALU slots per pair without the KL term); at small N the three launches dominate.
//   total       one workgroup: Z = sum s_i and sum k_i, float64, fixed order; kl
//   finish      one lane per row: the gradient and, for sg_tsne_step, the descent step
// DESIGN 3.14 has the compiler's resource figures.
#include "common.h"
#include "../../include/shapegan_hip.h"

#pragma clang fp contract(off)
#include "tsne_core.h"

namespace sg {

constexpr int kTsneBlock = 256;
constexpr int kTsneTile = 64;      // dist: outputs per workgroup side
constexpr int kTsneKc = 16;        // dist: coordinates per LDS step
constexpr int kTsneSym = 32;       // symmetrize: tile side
constexpr int kTsneRows = 4;       // gradient: rows per workgroup
constexpr int kTsneTotalBlock = 1024;

// the sum over a 256-lane workgroup, the same bits in every lane: butterfly inside a wave, the four waves added in wave order
__device__ __forceinline__ double tsne_block_sum(double v, double* red) {
    v = sg_wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(kTsneBlock) tsne_dist_kernel(const float* __restrict__ X, long N, long D, float* __restrict__ P) {
    __shared__ float xi[kTsneTile][kTsneKc + 1], xj[kTsneTile][kTsneKc + 1];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const long i0 = (long)blockIdx.y * kTsneTile, j0 = (long)blockIdx.x * kTsneTile;
    float acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
    for (long k0 = 0; k0 < D; k0 += kTsneKc) {
        for (int e = tid; e < kTsneTile * kTsneKc; e += kTsneBlock) {
            const int r = e >> 4, k = e & 15;
            const bool kin = k0 + k < D;
            xi[r][k] = (kin && i0 + r < N) ? X[(i0 + r) * D + k0 + k] : 0.f;      // (a coordinate beyond D is 0 on both sides: adds exactly 0)
            xj[r][k] = (kin && j0 + r < N) ? X[(j0 + r) * D + k0 + k] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kTsneKc; ++k) {
            float a4[4], b4[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) a4[a] = xi[ty + 16 * a][k], b4[a] = xj[tx + 16 * a][k];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = sg_tsne_d2_step(acc[a][b], a4[a], b4[b]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const long i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
            if (i < N && j < N) P[i * N + j] = acc[a][b];
        }
}

__global__ void __launch_bounds__(kTsneBlock) tsne_search_kernel(float* __restrict__ P, long N, double log_perp, double tol, int max_steps,
                                                                 float* __restrict__ beta) {
    __shared__ double red[4];
    __shared__ float redm[4];
    const int tid = threadIdx.x;
    const long i = blockIdx.x;
    float* const row = P + i * N;
    float m = INFINITY;
    for (long j = tid; j < N; j += kTsneBlock)
        if (j != i) m = fminf(m, row[j]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fminf(m, __shfl_xor(m, off, 64));
    if ((tid & 63) == 0) redm[tid >> 6] = m;
    __syncthreads();
    m = fminf(fminf(redm[0], redm[1]), fminf(redm[2], redm[3]));
    SgTsneSearch st;
    sg_tsne_search_init(&st);
    double sum_p = 1.0;
    for (int step = 0;; ++step) {
        double sp = 0.0, sdp = 0.0;
        for (long j = tid; j < N; j += kTsneBlock)
            if (j != i) {
                const float d = row[j] - m;
                const float p = sg_tsne_cond(st.beta, d);
                sp += (double)p;
                sdp += (double)d * (double)p;
            }
        sp = tsne_block_sum(sp, red);
        sdp = tsne_block_sum(sdp, red);
        sum_p = sp;
        if (step + 1 >= max_steps) break;
        if (sg_tsne_search_next(&st, sg_tsne_entropy(st.beta, sp, sdp) - log_perp, tol)) break;
    }
    for (long j = tid; j < N; j += kTsneBlock)      // (a lane rewrites only elements it alone reads)
        row[j] = j == i ? 0.f : (float)((double)sg_tsne_cond(st.beta, row[j] - m) / sum_p);
    if (tid == 0) beta[i] = st.beta;
}

__global__ void __launch_bounds__(kTsneBlock) tsne_symmetrize_kernel(float* __restrict__ P, long N) {
    if (blockIdx.x < blockIdx.y) return;      // the pair of tiles (t, u) and (u, t) belongs to the workgroup with t <= u
    __shared__ float A[kTsneSym][kTsneSym + 1], B[kTsneSym][kTsneSym + 1];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long a0 = (long)blockIdx.y * kTsneSym, b0 = (long)blockIdx.x * kTsneSym;
    const bool diagonal = blockIdx.x == blockIdx.y;
    const float two_n = (float)(2 * N);
    for (int r = ty; r < kTsneSym; r += 8) {
        A[r][tx] = (a0 + r < N && b0 + tx < N) ? P[(a0 + r) * N + b0 + tx] : 0.f;
        B[r][tx] = (b0 + r < N && a0 + tx < N) ? P[(b0 + r) * N + a0 + tx] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < kTsneSym; r += 8) {
        if (a0 + r < N && b0 + tx < N) P[(a0 + r) * N + b0 + tx] = sg_tsne_joint(A[r][tx], B[tx][r], two_n);
        if (!diagonal && b0 + r < N && a0 + tx < N) P[(b0 + r) * N + a0 + tx] = sg_tsne_joint(A[tx][r], B[r][tx], two_n);
    }
}

__global__ void __launch_bounds__(kTsneBlock) tsne_plogp_rows_kernel(const float* __restrict__ P, long N, double* __restrict__ rows) {
    __shared__ double red[4];
    const long i = blockIdx.x;
    const float* row = P + i * N;
    double s = 0.0;
    for (long j = threadIdx.x; j < N; j += kTsneBlock) {
        const float p = row[j];
        if (p > 0.f) s += (double)p * log((double)p);
    }
    s = tsne_block_sum(s, red);
    if (threadIdx.x == 0) rows[i] = s;
}

// one workgroup: the float64 sum of v[i * stride], i < n: lane t adds i = t, t + 1024, ... in order, then a tree over the lanes
__device__ __forceinline__ double tsne_total(const double* v, long n, long stride, double* red) {
    double s = 0.0;
    for (long i = threadIdx.x; i < n; i += kTsneTotalBlock) s += v[i * stride];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = kTsneTotalBlock / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(kTsneTotalBlock) tsne_plogp_total_kernel(const double* __restrict__ rows, long N, double* __restrict__ plogp) {
    __shared__ double red[kTsneTotalBlock];
    const double s = tsne_total(rows, N, 1, red);
    if (threadIdx.x == 0) *plogp = s;
}

// stats [N][6] float64: s, a_x, a_y, r_x, r_y, k of every row
template <int V, bool KL>
__global__ void __launch_bounds__(kTsneBlock) tsne_rows_kernel(const float* __restrict__ Y, const float* __restrict__ P, long N,
                                                               double* __restrict__ stats) {
    __shared__ double red[4][kTsneRows * 6];
    const int tid = threadIdx.x;
    const long r0 = (long)blockIdx.x * kTsneRows;
    long ri[kTsneRows];
    float yix[kTsneRows], yiy[kTsneRows];
    const float* prow[kTsneRows];
#pragma unroll
    for (int r = 0; r < kTsneRows; ++r) {
        ri[r] = r0 + r < N ? r0 + r : N - 1;      // (rows beyond N repeat the last one; their sums are dropped)
        yix[r] = Y[2 * ri[r]];
        yiy[r] = Y[2 * ri[r] + 1];
        prow[r] = P + ri[r] * N;
    }
    double acc[kTsneRows][6];
#pragma unroll
    for (int r = 0; r < kTsneRows; ++r)
#pragma unroll
        for (int e = 0; e < 6; ++e) acc[r][e] = 0.0;
    const long units = N / V;      // (V = 4 only when N is a multiple of 4)
    constexpr int kIter = SG_TSNE_FLUSH / V;
    for (long u0 = 0; u0 < units; u0 += (long)kTsneBlock * kIter) {
        SgTsneAcc a[kTsneRows];
#pragma unroll
        for (int r = 0; r < kTsneRows; ++r) sg_tsne_acc_zero(&a[r]);
#pragma unroll 2
        for (int it = 0; it < kIter; ++it) {
            const long unit = u0 + (long)it * kTsneBlock + tid;
            const bool live = unit < units;
            const long c = (live ? unit : units - 1) * V;      // (a lane beyond the row re-reads its last unit and counts nothing)
            float yj[2 * V], p[kTsneRows][V];
            if constexpr (V == 4) {
                const float4 y0 = *reinterpret_cast<const float4*>(Y + 2 * c), y1 = *reinterpret_cast<const float4*>(Y + 2 * c + 4);
                yj[0] = y0.x, yj[1] = y0.y, yj[2] = y0.z, yj[3] = y0.w;
                yj[4] = y1.x, yj[5] = y1.y, yj[6] = y1.z, yj[7] = y1.w;
#pragma unroll
                for (int r = 0; r < kTsneRows; ++r) {
                    const float4 q = *reinterpret_cast<const float4*>(prow[r] + c);
                    p[r][0] = q.x, p[r][1] = q.y, p[r][2] = q.z, p[r][3] = q.w;
                }
            } else {
                yj[0] = Y[2 * c], yj[1] = Y[2 * c + 1];
#pragma unroll
                for (int r = 0; r < kTsneRows; ++r) p[r][0] = prow[r][c];
            }
#pragma unroll
            for (int r = 0; r < kTsneRows; ++r)
#pragma unroll
                for (int v = 0; v < V; ++v)
                    sg_tsne_pair<KL>(&a[r], yix[r], yiy[r], yj[2 * v], yj[2 * v + 1], p[r][v], live && c + v != ri[r]);
        }
#pragma unroll
        for (int r = 0; r < kTsneRows; ++r) {
            acc[r][0] += (double)a[r].s;
            acc[r][1] += (double)a[r].ax;
            acc[r][2] += (double)a[r].ay;
            acc[r][3] += (double)a[r].rx;
            acc[r][4] += (double)a[r].ry;
            if (KL) acc[r][5] += (double)a[r].k;
        }
    }
#pragma unroll
    for (int r = 0; r < kTsneRows; ++r)
#pragma unroll
        for (int e = 0; e < 6; ++e) {
            const double v = sg_wave_sum_d(acc[r][e]);
            if ((tid & 63) == 0) red[tid >> 6][r * 6 + e] = v;
        }
    __syncthreads();
    if (tid < kTsneRows * 6 && r0 + tid / 6 < N)
        stats[(r0 + tid / 6) * 6 + tid % 6] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// scalars[0] = Z; kl = plogp + sum k + log Z
__global__ void __launch_bounds__(kTsneTotalBlock) tsne_total_kernel(const double* __restrict__ stats, long N, const double* __restrict__ plogp,
                                                                     double* __restrict__ scalars, double* __restrict__ kl) {
    __shared__ double red[kTsneTotalBlock];
    const double Z = tsne_total(stats, N, 6, red);
    double K = 0.0;
    if (kl) K = tsne_total(stats + 5, N, 6, red);
    if (threadIdx.x == 0) {
        scalars[0] = Z;
        if (kl) *kl = *plogp + K + log(Z);
    }
}

template <bool UPDATE>
__global__ void __launch_bounds__(kTsneBlock) tsne_finish_kernel(const double* __restrict__ stats, const double* __restrict__ scalars, long N,
                                                                 float exaggeration, float* __restrict__ grad, float* __restrict__ Y,
                                                                 float* __restrict__ velocity, float* __restrict__ gains, float momentum,
                                                                 float lr, float min_gain) {
    const long i = (long)blockIdx.x * kTsneBlock + threadIdx.x;
    if (i >= N) return;
    const double Z = scalars[0];
    const double* s = stats + i * 6;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float g = sg_tsne_grad(s[1 + c], s[3 + c], Z, exaggeration);
        grad[2 * i + c] = g;
        if (UPDATE) sg_tsne_update_one(Y + 2 * i + c, velocity + 2 * i + c, gains + 2 * i + c, g, momentum, lr, min_gain);
    }
}

__global__ void __launch_bounds__(kTsneBlock) tsne_update_kernel(float* __restrict__ Y, float* __restrict__ velocity, float* __restrict__ gains,
                                                                 const float* __restrict__ grad, long n, float momentum, float lr,
                                                                 float min_gain) {
    const long e = (long)blockIdx.x * kTsneBlock + threadIdx.x;
    if (e < n) sg_tsne_update_one(Y + e, velocity + e, gains + e, grad[e], momentum, lr, min_gain);
}

static bool tsne_aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

template <bool UPDATE>
static int tsne_gradient_launch(float* Y, const float* P, long N, float exaggeration, const double* plogp, float* velocity, float* gains,
                                float momentum, float lr, float min_gain, float* grad, double* kl, void* workspace, hipStream_t stream) {
    double* stats = static_cast<double*>(workspace);
    double* scalars = stats + 6 * N;
    const dim3 grid((unsigned)((N + kTsneRows - 1) / kTsneRows)), block(kTsneBlock);
    const bool wide = N % 4 == 0 && (reinterpret_cast<uintptr_t>(P) & 15) == 0 && (reinterpret_cast<uintptr_t>(Y) & 15) == 0;
    if (wide && kl) hipLaunchKernelGGL((tsne_rows_kernel<4, true>), grid, block, 0, stream, Y, P, N, stats);
    else if (wide) hipLaunchKernelGGL((tsne_rows_kernel<4, false>), grid, block, 0, stream, Y, P, N, stats);
    else if (kl) hipLaunchKernelGGL((tsne_rows_kernel<1, true>), grid, block, 0, stream, Y, P, N, stats);
    else hipLaunchKernelGGL((tsne_rows_kernel<1, false>), grid, block, 0, stream, Y, P, N, stats);
    hipLaunchKernelGGL(tsne_total_kernel, dim3(1), dim3(kTsneTotalBlock), 0, stream, stats, N, plogp, scalars, kl);
    hipLaunchKernelGGL((tsne_finish_kernel<UPDATE>), dim3((unsigned)((N + kTsneBlock - 1) / kTsneBlock)), block, 0, stream, stats, scalars, N,
                       exaggeration, grad, Y, velocity, gains, momentum, lr, min_gain);
    return SG_OK;
}

}  // namespace sg

using namespace sg;

extern "C" {

size_t sg_tsne_affinities_workspace_bytes(long N) { return N > 0 ? (size_t)N * sizeof(double) : 0; }
size_t sg_tsne_gradient_workspace_bytes(long N) { return N > 0 ? ((size_t)6 * N + 2) * sizeof(double) : 0; }

int sg_tsne_affinities(const float* X, long N, long D, double perplexity, double tol, int max_steps, float* P, float* beta,
                       double* plogp, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    SG_CHECK_ARG(sg_tsne_sizes_ok(N, D, perplexity));
    SG_CHECK_ARG(X && P && beta && plogp && workspace && tol >= 0.0 && max_steps >= 1);
    SG_CHECK_ARG(tsne_aligned8(workspace) && tsne_aligned8(plogp));
    if (workspace_bytes < sg_tsne_affinities_workspace_bytes(N))
        SG_FAIL(SG_ERR_WORKSPACE, "sg_tsne_affinities: workspace of %zu B, %zu B needed", workspace_bytes, sg_tsne_affinities_workspace_bytes(N));
    double* rows = static_cast<double*>(workspace);
    const unsigned td = (unsigned)((N + kTsneTile - 1) / kTsneTile), ts = (unsigned)((N + kTsneSym - 1) / kTsneSym);
    hipLaunchKernelGGL(tsne_dist_kernel, dim3(td, td), dim3(kTsneBlock), 0, stream, X, N, D, P);
    hipLaunchKernelGGL(tsne_search_kernel, dim3((unsigned)N), dim3(kTsneBlock), 0, stream, P, N, log(perplexity), tol, max_steps, beta);
    hipLaunchKernelGGL(tsne_symmetrize_kernel, dim3(ts, ts), dim3(kTsneBlock), 0, stream, P, N);
    hipLaunchKernelGGL(tsne_plogp_rows_kernel, dim3((unsigned)N), dim3(kTsneBlock), 0, stream, P, N, rows);
    hipLaunchKernelGGL(tsne_plogp_total_kernel, dim3(1), dim3(kTsneTotalBlock), 0, stream, rows, N, plogp);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_tsne_gradient(const float* Y, const float* P, long N, float exaggeration, const double* plogp, float* grad, double* kl,
                     void* workspace, size_t workspace_bytes, hipStream_t stream) {
    SG_CHECK_ARG(N >= 4 && N <= SG_TSNE_MAX_POINTS && Y && P && grad && workspace && tsne_aligned8(workspace));
    SG_CHECK_ARG(!kl || (plogp && tsne_aligned8(kl) && tsne_aligned8(plogp)));
    if (workspace_bytes < sg_tsne_gradient_workspace_bytes(N))
        SG_FAIL(SG_ERR_WORKSPACE, "sg_tsne_gradient: workspace of %zu B, %zu B needed", workspace_bytes, sg_tsne_gradient_workspace_bytes(N));
    tsne_gradient_launch<false>(const_cast<float*>(Y), P, N, exaggeration, plogp, nullptr, nullptr, 0.f, 0.f, 0.f, grad, kl, workspace, stream);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_tsne_update(float* Y, float* velocity, float* gains, const float* grad, long N, float momentum, float lr, float min_gain,
                   hipStream_t stream) {
    SG_CHECK_ARG(N >= 1 && N <= SG_TSNE_MAX_POINTS && Y && velocity && gains && grad);
    hipLaunchKernelGGL(tsne_update_kernel, dim3((unsigned)((2 * N + kTsneBlock - 1) / kTsneBlock)), dim3(kTsneBlock), 0, stream, Y, velocity,
                       gains, grad, 2 * N, momentum, lr, min_gain);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_tsne_step(float* Y, const float* P, long N, float exaggeration, const double* plogp, float* velocity, float* gains,
                 float momentum, float lr, float min_gain, float* grad, double* kl, void* workspace, size_t workspace_bytes,
                 hipStream_t stream) {
    SG_CHECK_ARG(N >= 4 && N <= SG_TSNE_MAX_POINTS && Y && P && velocity && gains && grad && workspace && tsne_aligned8(workspace));
    SG_CHECK_ARG(!kl || (plogp && tsne_aligned8(kl) && tsne_aligned8(plogp)));
    if (workspace_bytes < sg_tsne_gradient_workspace_bytes(N))
        SG_FAIL(SG_ERR_WORKSPACE, "sg_tsne_step: workspace of %zu B, %zu B needed", workspace_bytes, sg_tsne_gradient_workspace_bytes(N));
    tsne_gradient_launch<true>(Y, P, N, exaggeration, plogp, velocity, gains, momentum, lr, min_gain, grad, kl, workspace, stream);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

}  // extern "C"
