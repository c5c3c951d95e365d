// shapegan_amd/csrc/latent_fit.hip — encoding a shape with a frozen SDFNet: forward, loss and the latent-only backward of a tile of
// points in ONE launch (K7c; serves shapegan_amd/reconstruct.py fit_latent_codes and SDFNet.latent_loss_and_grad).
//
// A DeepSDF auto-decoder (model/sdf_net.py, train_sdf_autodecoder.py:80-91) has no encoder: the code of an unseen shape is found by
// minimising  mean_p |SDFNet(x_p, z) - clamp(sdf_p, +-cutoff)| + sigma mean_k z_k^2  over z with the weights frozen.  Composed from the
// training kernels (sg_sdfnet_fwd with `acts`, sg_sdfnet_bwd, sg_sdfnet_bwd_finish) that costs 7 KB of activation images and 7 KB of
// dZ images per point, which only the weight-gradient GEMMs ever read.  With frozen weights the backward chain needs of the forward
// only ReLU' — one bit per element — and the latent gradient needs of the chain only the per-shape row sums of dZ1 and dZ5
// (sg_sdfnet_shape_bias_bwd turns them into d/dz).  So a workgroup here
//   1. runs the eight layers of its tile through sdfnet_fwd_tile (per-shape bias mode, the forward of sg_sdfnet_fwd bit for bit) and
//      KEEPS the seven sign words a lane produces (16 rows x 1 point per word: 7 VGPRs) instead of storing them;
//   2. forms the upstream gradient in the epilogue: out = tanh(v), d = out - clamp(target), dz8 = sign(d) (1 - out^2) / m;
//   3. walks the chain back with the transposed packs of the same weight image, dZ_l = (T_{l+1} dZ_{l+1}) * ReLU'(H_l), reusing the
//      forward's single [256][P] LDS tile as the B operand and the forward's own GEMM loop and fragment mapping — the lane that made
//      a sign word is the lane that needs it (sdfnet_frozen_bwd_tile in sdfnet_frozen.h, shared with K7d, sdfnet_project.hip);
//   4. reduces dZ5 and dZ1 over the tile's points in registers (DPP) and stores [2][256] sums and the tile's sum of |d|.
// Nothing else goes to memory: 16 B in per point, 2 KB out per TILE.  latent_reduce_kernel adds a shape's tiles in tile order.
//
// Tiles never straddle shapes and a lane beyond a shape's used points contributes exact zeros (its dz8 is 0), so a shape's result does
// not depend on what else is in the call.  The points of a shape that a call uses are a window that wraps around its cloud: used
// point i < m is seg_off[s] + (win_start + i) mod n — a fit loop walks mini-batches through the cloud without an index tensor.
//
// This file holds what is the latent fit's own: the loss epilogue (LatentFitIo::store), the window, the row sums and the reduction.
// The sign keeping, the table row, the forward's arguments and the chain back are in sdfnet_frozen.h.
#include "common.h"
#include "sdfnet_frozen.h"
#include "../../include/shapegan_hip.h"

namespace sg {

// 32-point tiles: NT = 1 accumulator tile per wave.  The 64-point forward sits just under the 128 VGPRs of two workgroups per CU
// (sdfnet.hip); fourteen more live words across it would spill or halve the occupancy, and sign words in LDS (14 KB on top of 77 KB)
// would leave one workgroup per CU.  At 32 points the words are 7 VGPRs, the kernel stays far below 128 and its 42 KB of LDS put
// three workgroups on a CU (DESIGN 3.13 has the compiler's figures for both).
constexpr int kFitTile = SG_SDFNET_LATENT_TILE;
constexpr int kFitRow = SG_SDFNET_LATENT_PARTIAL_ROW;
static_assert(kFitRow >= 2 * kH + 1, "partial row");

struct LatentFitArgs {
    const float* points;      // [*,3]
    const float* target;      // [*]
    const int64_t* seg_off;   // [S+1]
    long S;
    const float* zb1;         // [S][256]
    const float* zb5;
    const float* packed;
    SdfPackLayout lay;
    float cutoff;
    long win_start, win_count;
    const int* tiles;         // [T][2]: shape, first used point i0 of the tile
    float* part;              // [T][kFitRow]
};

struct LatentFitIo : SdfSignKeeper {
    const LatentFitArgs* f;
    long beg, n, first;       // the shape's run and (win_start + i0) mod n
    int cnt;                  // used points of this tile
    float inv_den;            // divisor m as a float
    float* dz8s;              // LDS [P]
    float* absd;              // LDS [P]
    __device__ __forceinline__ long index(long gp) const {
        const long i = first + gp;      // (gp < cnt <= n and first < n: one wrap at most)
        return beg + (i >= n ? i - n : i);
    }
    __device__ __forceinline__ float coord(const SdfFwdArgs&, long gp, int c) const { return f->points[index(gp) * 3 + c]; }
    __device__ __forceinline__ void store(const SdfFwdArgs&, long gp, float v) const {
        float dz = 0.f, ad = 0.f;
        if (gp < cnt) {
            const float o = tanhf(v);
            const float c = f->cutoff;
            const float t = fminf(fmaxf(f->target[index(gp)], -c), c);
            const float d = o - t;
            ad = fabsf(d);
            const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            dz = sg * ((1.f - o * o) / inv_den);
        }
        dz8s[gp] = dz;
        absd[gp] = ad;
    }
};

template <int P>
__global__ void __launch_bounds__(512, 4) latent_fit_kernel(LatentFitArgs f) {
    __shared__ float s_dz8[P], s_abs[P];
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kh = lane >> 5, r = lane & 31;
    const long tile = blockIdx.x;
    const SdfTileRow row = sdf_tile_row(f.tiles, f.seg_off, f.S, tile);
    const long n = row.n;
    float* const prow = f.part + tile * kFitRow;
    const long m = n <= 0 ? 0 : (f.win_count <= 0 || f.win_count > n ? n : f.win_count);
    long cnt = row.i0 < 0 ? 0 : m - row.i0;
    if (cnt > P) cnt = P;
    if (cnt <= 0) {       // (a table row that names nothing: the whole workgroup leaves, its partial row is zero)
        for (int e = tid; e < 2 * kH + 1; e += 512) prow[e] = 0.f;
        return;
    }
    unsigned signs[7];
#pragma unroll
    for (int e = 0; e < 7; ++e) signs[e] = 0u;
    LatentFitIo io;
    io.signs = signs;
    io.f = &f;
    io.beg = row.beg;
    io.n = n;
    io.first = (f.win_start + row.i0) % n;
    io.cnt = (int)cnt;
    io.inv_den = (float)m;
    io.dz8s = s_dz8;
    io.absd = s_abs;

    const SdfFwdArgs a = sdf_frozen_tile_args(f.points, f.packed, f.lay, f.zb1 + (long)row.s * kH, f.zb5 + (long)row.s * kH, cnt);
    sdfnet_fwd_tile<P, true, false, false, LatentFitIo, true>(a, 0, io);
    __syncthreads();      // dz8 / |d| of every point are in LDS, every read of H7 is done

    // the tile's sum of |d| in point order (points beyond cnt hold 0)
    if (tid == 0) {
        float l = 0.f;
#pragma unroll 8
        for (int p = 0; p < P; ++p) l += s_abs[p];
        prow[2 * kH] = l;
    }

    // dZ5 and dZ1 are the rows behind the latent gradient: their sums over the tile's points (lane 31 / 63 of a half-wave holds one)
    sdfnet_frozen_bwd_tile<P>(f.packed, f.lay, smem, signs[0], signs[1], signs[2], signs[3], signs[4], signs[5], signs[6], s_dz8,
                              [&](int i, int q, float g) __attribute__((always_inline)) {
                                  if (i == 4 || i == 0) {
                                      const float rsum = half_wave_sum(g);
                                      if (r == 31) prow[(i == 0 ? 0 : kH) + wave * 32 + 4 * kh + frag_rowoff(q)] = rsum;
                                  }
                              });
}

// per shape: t1 / t5 [256][S] = the sums of its tiles' dZ1 / dZ5 rows and loss = sum |d| / m, tiles added in tile order (double)
__global__ void __launch_bounds__(512) latent_reduce_kernel(const float* __restrict__ part, const int64_t* __restrict__ tile_off,
                                                            const int64_t* __restrict__ seg_off, long S, long win_count,
                                                            float* __restrict__ t1, float* __restrict__ t5, float* __restrict__ loss) {
    __shared__ double red[64];
    const long s = blockIdx.x;
    const int tid = threadIdx.x;
    const long ta = tile_off[s], tb = tile_off[s + 1];
    const float* src = part + tid;
    double acc = 0;
    long t = ta;
    for (; t + 8 <= tb; t += 8) {      // eight loads in flight, added in tile order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(t + u) * kFitRow];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; t < tb; ++t) acc += src[t * kFitRow];
    (tid < kH ? t1 : t5)[(long)(tid & (kH - 1)) * S + s] = (float)acc;
    if (tid < 64) {
        double l = 0;
        for (long u = ta + tid; u < tb; u += 64) l += part[u * kFitRow + 2 * kH];
        red[tid] = l;
    }
    __syncthreads();
    if (tid == 0) {
        double l = 0;
        for (int u = 0; u < 64; ++u) l += red[u];
        const long n = seg_off[s + 1] - seg_off[s];
        const long m = win_count <= 0 || win_count > n ? n : win_count;
        loss[s] = (float)(l / (double)(m > 0 ? m : 1));
    }
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_sdfnet_latent_grad(const float* points, const float* target, const int64_t* seg_off, long nshapes, const float* zb1,
                          const float* zb5, const float* packed, float cutoff, long win_start, long win_count, const int* tiles,
                          long ntiles, float* partials, hipStream_t stream) {
    SG_CHECK_ARG(points && target && seg_off && zb1 && zb5 && packed && tiles && partials);
    SG_CHECK_ARG(nshapes >= 1 && win_start >= 0 && ntiles >= 1 && ntiles < (1L << 31) && cutoff >= 0.f);
    LatentFitArgs f;
    f.points = points;
    f.target = target;
    f.seg_off = seg_off;
    f.S = nshapes;
    f.zb1 = zb1;
    f.zb5 = zb5;
    f.packed = packed;
    f.lay = make_layout(3);
    f.cutoff = cutoff;
    f.win_start = win_start;
    f.win_count = win_count;
    f.tiles = tiles;
    f.part = partials;
    const size_t lds = sdf_fwd_lds_bytes(kFitTile, f.lay.KUp);
    static SgPerDeviceOnce once;
    if (const int rc = sg_reserve_lds(once, latent_fit_kernel<kFitTile>, lds, "sg_sdfnet_latent_grad")) return rc;
    hipLaunchKernelGGL((latent_fit_kernel<kFitTile>), dim3((unsigned)ntiles), dim3(512), lds, stream, f);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_sdfnet_latent_reduce(const float* partials, const int64_t* tile_off, const int64_t* seg_off, long nshapes, long win_count,
                            float* t1, float* t5, float* loss, hipStream_t stream) {
    SG_CHECK_ARG(partials && tile_off && seg_off && t1 && t5 && loss && nshapes >= 1 && nshapes < (1L << 31));
    hipLaunchKernelGGL(latent_reduce_kernel, dim3((unsigned)nshapes), dim3(512), 0, stream, partials, tile_off, seg_off, nshapes,
                       win_count, t1, t5, loss);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

}  // extern "C"
