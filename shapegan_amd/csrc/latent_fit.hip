// shapegan_amd/csrc/latent_fit.hip — encoding a shape with a frozen SDFNet: forward, loss and the latent-only backward of a tile of
// points in ONE launch (K7c; serves shapegan_amd/reconstruct.py fit_latent_codes and SDFNet.latent_loss_and_grad), and the same with
// the gradient with respect to an affine map of the observed points (K7e; fit_codes_and_poses and SDFNet.latent_pose_loss_and_grad).
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
// The pose (the POSE instance of both kernels).  A scan does not arrive in the network's canonical frame: a partial cloud's bounding
// sphere is not the object's and a sensor's cloud is not upright.  An auto-decoder has no other model of where the shape should be
// than the network itself, so the pose is optimised through it: observed q, canonical x = A q + t, target' = clamp(ts target, +-cutoff)
// (a similarity scales distances by ts = s), and  loss = mean_p |SDFNet(A q_p + t, z) - target'_p|.  d loss / dz is the above at the
// posed points.  d loss / d(A|t) is K7d's point gradient  g[p] = W5[:, 256:259]^T dZ5[:, p] + W1[:, 0:3]^T dZ1[:, p]  (SdfPointGrad
// in sdfnet_frozen.h) of this loss, contracted with the observed coordinates: dA = sum_p g[p] (x) q[p], dt = sum_p g[p]; and
// d loss / d ts = sum_p e[p], e = -sign(d) target / m inside the clamp.  With a pose a workgroup therefore also
//   - stages its tile's q in LDS (0 beyond the tile's count), forms x there (the order of the header: three nested fmas per
//     coordinate) and hands the forward its coordinates from there, as K7d's Io does;
//   - leaves e per point in the epilogue;
//   - multiplies dZ5 / dZ1 by the point columns in the chain's functor;
//   - reduces g (x) q, g and e over the tile's points in point order: 13 more floats per tile, g itself never goes to memory.
// Every sum has a fixed order.  The instances are one body, and with the identity pose and ts = 1, x == q and target' ==
// clamp(target) bit for bit: floats [0, 513) of a partial row, the loss and the latent gradient are then the same without and with a pose.
//
// This file holds what is the latent fit's own: the loss epilogue (LatentFitIo::store), the row sums, the pose sums and the
// reduction.  The sign keeping, the table row and its window, the forward's arguments, the chain back and the point gradient are in
// sdfnet_frozen.h.
#include "common.h"
#include "sdfnet_frozen.h"
#include "../../include/shapegan_hip.h"

namespace sg {

// 32-point tiles: NT = 1 accumulator tile per wave.  The 64-point forward sits just under the 128 VGPRs of two workgroups per CU
// (sdfnet.hip); fourteen more live words across it would spill or halve the occupancy, and sign words in LDS (14 KB on top of 77 KB)
// would leave one workgroup per CU.  At 32 points the words are 7 VGPRs, the kernel stays far below 128 and its 42 KB of LDS put
// three workgroups on a CU (DESIGN 3.13 has the compiler's figures for both).
constexpr int kFitTile = SG_SDFNET_LATENT_TILE;
constexpr int kPoseSums = 13;      // 9 of g (x) q, 3 of g, 1 of e
// floats of a partial row: [0, 513) the row sums of dZ1 / dZ5 and the sum of |d|; with a pose the pose sums and two zeros behind them
template <bool POSE>
constexpr int kFitRow = POSE ? SG_SDFNET_POSE_PARTIAL_ROW : SG_SDFNET_LATENT_PARTIAL_ROW;
static_assert(kFitRow<false> >= 2 * kH + 1 && kFitRow<true> >= 2 * kH + 1 + kPoseSums && kFitRow<true> == kFitRow<false> + 15, "partial row");

struct LatentFitArgs {
    const float* points;      // [*,3] (with a pose: observed)
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
    const float* pose;        // [S][16], NULL without a pose
    float* part;              // [T][kFitRow<POSE>]
};

template <bool POSE>
struct LatentFitIo : SdfSignKeeper {
    const LatentFitArgs* f;
    SdfTileWindow win;
    float inv_den;            // divisor m as a float
    float* dz8s;              // LDS [P]
    float* absd;              // LDS [P]
    // with a pose only:
    float ts;
    const lds_float* xyz;     // LDS [P][3]: the posed points
    float* es;                // LDS [P]
    __device__ __forceinline__ float coord(const SdfFwdArgs&, long gp, int c) const {
        if constexpr (POSE)
            return xyz[gp * 3 + c];
        else
            return f->points[win.index(gp) * 3 + c];
    }
    __device__ __forceinline__ void store(const SdfFwdArgs&, long gp, float v) const {
        float dz = 0.f, ad = 0.f, e = 0.f;
        if (gp < win.cnt) {
            const float o = tanhf(v);
            const float c = f->cutoff;
            const float raw = f->target[win.index(gp)];
            float st = raw;
            if constexpr (POSE) st = ts * raw;
            const float t = fminf(fmaxf(st, -c), c);
            const float d = o - t;
            ad = fabsf(d);
            const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            dz = sg * ((1.f - o * o) / inv_den);
            if constexpr (POSE)
                if (st > -c && st < c) e = (-sg * raw) / inv_den;
        }
        dz8s[gp] = dz;
        absd[gp] = ad;
        if constexpr (POSE) es[gp] = e;
    }
};

template <int P, bool POSE>
__global__ void __launch_bounds__(512, 4) latent_fit_kernel(LatentFitArgs f) {
    __shared__ float s_dz8[P], s_abs[P];
    // (referenced with a pose only; arrays of their own: members of one struct lose the 16-byte alignment of the point-order sums' reads)
    __shared__ float s_q[P * 3], s_xyz[P * 3], s_e[P], s_gp[8 * 3 * P], s_g[3 * P];
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int kRow = kFitRow<POSE>;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kh = lane >> 5, r = lane & 31;
    const long tile = blockIdx.x;
    const SdfTileRow row = sdf_tile_row(f.tiles, f.seg_off, f.S, tile);
    const SdfTileWindow win = sdf_tile_window(row, f.win_start, f.win_count, P);
    const long cnt = win.cnt;
    float* const prow = f.part + tile * kRow;
    if (cnt <= 0) {       // (a table row that names nothing: the whole workgroup leaves, its partial row is zero)
        for (int e = tid; e < kRow; e += 512) prow[e] = 0.f;
        return;
    }
    unsigned signs[7];
#pragma unroll
    for (int e = 0; e < 7; ++e) signs[e] = 0u;
    LatentFitIo<POSE> io;
    io.signs = signs;
    io.f = &f;
    io.win = win;
    io.inv_den = (float)win.m;
    io.dz8s = s_dz8;
    io.absd = s_abs;

    if constexpr (POSE) {
        const float* const ps = f.pose + (long)row.s * 16;
        io.ts = ps[12];
        io.xyz = (const lds_float*)s_xyz;
        io.es = s_e;
        // the tile's observed points (0 beyond cnt), then x_c = fma(A_c0, qx, fma(A_c1, qy, fma(A_c2, qz, t_c)))
        for (int e = tid; e < 3 * P; e += 512) {
            const int p = e / 3, c = e - 3 * p;
            s_q[e] = p < cnt ? f.points[win.index(p) * 3 + c] : 0.f;
        }
        __syncthreads();
        if (tid < 3 * P) {
            const int p = tid / 3, c = tid - 3 * p;
            const float* a = ps + 4 * c;
            s_xyz[tid] = __builtin_fmaf(a[0], s_q[p * 3], __builtin_fmaf(a[1], s_q[p * 3 + 1], __builtin_fmaf(a[2], s_q[p * 3 + 2], a[3])));
        }
        __syncthreads();
    }

    const SdfFwdArgs a = sdf_frozen_tile_args(f.points, f.packed, f.lay, f.zb1 + (long)row.s * kH, f.zb5 + (long)row.s * kH, cnt);
    sdfnet_fwd_tile<P, true, false, false, LatentFitIo<POSE>, true>(a, 0, io);
    [[maybe_unused]] SdfPointGrad<P> pg(smem, f.lay);
    if constexpr (POSE) pg.stage(f.packed, f.lay);
    __syncthreads();      // dz8 / |d| (/ e) of every point (and Wx) are in LDS, every read of H7 is done

    // the tile's sums of |d| and of e in point order (points beyond cnt hold 0)
    if (tid == 0) {
        float l = 0.f;
#pragma unroll 8
        for (int p = 0; p < P; ++p) l += s_abs[p];
        prow[2 * kH] = l;
    }
    if constexpr (POSE) {
        if (tid == 64) {
            float l = 0.f;
#pragma unroll 8
            for (int p = 0; p < P; ++p) l += s_e[p];
            prow[2 * kH + 1 + 12] = l;
            prow[2 * kH + 1 + 13] = 0.f;
            prow[2 * kH + 1 + 14] = 0.f;
        }
    }

    // dZ5 and dZ1 are the rows behind the latent gradient: their sums over the tile's points (lane 31 / 63 of a half-wave holds one);
    // with a pose also their products with the point columns
    sdfnet_frozen_bwd_tile<P>(f.packed, f.lay, smem, signs[0], signs[1], signs[2], signs[3], signs[4], signs[5], signs[6], s_dz8,
                              [&](int i, int q, float g) __attribute__((always_inline)) {
                                  if (i == 4 || i == 0) {
                                      const float rsum = half_wave_sum(g);
                                      if (r == 31) prow[(i == 0 ? 0 : kH) + wave * 32 + 4 * kh + frag_rowoff(q)] = rsum;
                                      if constexpr (POSE) pg.add(i, q, g);
                                  }
                              });
    if constexpr (POSE) {
        pg.partials(s_gp);
        __syncthreads();
        if (tid < 3 * P) {      // g_c of point p = tid % P, c = tid / P: the eight waves in wave order
            float v = s_gp[tid];
#pragma unroll
            for (int w = 1; w < 8; ++w) v += s_gp[w * 3 * P + tid];
            s_g[tid] = v;
        }
        __syncthreads();
        // sum_p g_c q_j (row-major c, j), then sum_p g_c: one thread each, in point order
        if (tid < 12) {
            const int c = tid < 9 ? tid / 3 : tid - 9, j = tid < 9 ? tid - 3 * c : -1;
            float l = 0.f;
#pragma unroll 8
            for (int p = 0; p < P; ++p) l = j < 0 ? l + s_g[c * P + p] : __builtin_fmaf(s_g[c * P + p], s_q[p * 3 + j], l);
            prow[2 * kH + 1 + tid] = l;
        }
    }
}

// per shape: t1 / t5 [256][S] = the sums of its tiles' dZ1 / dZ5 rows and loss = sum |d| / m, tiles added in tile order (double).
// With a pose (576 threads) also gpose [S][16] = the sums of its tiles' pose sums: threads [512, 525) own its thirteen live floats.
template <bool POSE>
__global__ void __launch_bounds__(POSE ? 576 : 512)
    latent_reduce_kernel(const float* __restrict__ part, const int64_t* __restrict__ tile_off, const int64_t* __restrict__ seg_off, long S,
                         long win_count, float* __restrict__ t1, float* __restrict__ t5, float* __restrict__ loss,
                         float* __restrict__ gpose) {
    __shared__ double red[64];
    constexpr int kRow = kFitRow<POSE>;
    const long s = blockIdx.x;
    const int tid = threadIdx.x;
    const long ta = tile_off[s], tb = tile_off[s + 1];
    int col = tid;
    [[maybe_unused]] bool live = true;
    if constexpr (POSE) {
        // float k of gpose is in pose's layout, rows of A_c0 A_c1 A_c2 t_c: from sum g_c q_j (513 + 3 c + j), sum g_c (522 + c), sum e (525)
        const int k = tid - 2 * kH;
        live = tid < 2 * kH + kPoseSums;
        if (tid >= 2 * kH) col = !live ? 0 : k == 12 ? 2 * kH + 13 : (k & 3) == 3 ? 2 * kH + 10 + (k >> 2) : 2 * kH + 1 + 3 * (k >> 2) + (k & 3);
    }
    const float* src = part + col;
    double acc = 0;
    long t = ta;
    for (; t + 8 <= tb; t += 8) {      // eight loads in flight, added in tile order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(t + u) * kRow];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; t < tb; ++t) acc += src[t * kRow];
    if (!POSE || tid < 2 * kH)
        (tid < kH ? t1 : t5)[(long)(tid & (kH - 1)) * S + s] = (float)acc;
    else if (tid < 2 * kH + 16)
        gpose[s * 16 + (tid - 2 * kH)] = live ? (float)acc : 0.f;
    if (tid < 64) {
        double l = 0;
        for (long u = ta + tid; u < tb; u += 64) l += part[u * kRow + 2 * kH];
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

// the launches behind the four entry points, which check their arguments before and the launch after (both name the entry point);
// `pose` / `gpose` are NULL without a pose
template <bool POSE>
static int latent_grad_launch(const char* name, const float* points, const float* target, const int64_t* seg_off, long nshapes,
                              const float* zb1, const float* zb5, const float* packed, const float* pose, float cutoff, long win_start,
                              long win_count, const int* tiles, long ntiles, float* partials, hipStream_t stream) {
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
    f.pose = pose;
    f.part = partials;
    const size_t lds = sdf_fwd_lds_bytes(kFitTile, f.lay.KUp);
    static SgPerDeviceOnce once;      // (one per instance)
    if (const int rc = sg_reserve_lds(once, latent_fit_kernel<kFitTile, POSE>, lds, name)) return rc;
    hipLaunchKernelGGL((latent_fit_kernel<kFitTile, POSE>), dim3((unsigned)ntiles), dim3(512), lds, stream, f);
    return SG_OK;
}

template <bool POSE>
static void latent_reduce_launch(const float* partials, const int64_t* tile_off, const int64_t* seg_off, long nshapes, long win_count,
                                 float* t1, float* t5, float* loss, float* gpose, hipStream_t stream) {
    hipLaunchKernelGGL(latent_reduce_kernel<POSE>, dim3((unsigned)nshapes), dim3(POSE ? 576 : 512), 0, stream, partials, tile_off,
                       seg_off, nshapes, win_count, t1, t5, loss, gpose);
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_sdfnet_latent_grad(const float* points, const float* target, const int64_t* seg_off, long nshapes, const float* zb1,
                          const float* zb5, const float* packed, float cutoff, long win_start, long win_count, const int* tiles,
                          long ntiles, float* partials, hipStream_t stream) {
    SG_CHECK_ARG(points && target && seg_off && zb1 && zb5 && packed && tiles && partials);
    SG_CHECK_ARG(nshapes >= 1 && win_start >= 0 && ntiles >= 1 && ntiles < (1L << 31) && cutoff >= 0.f);
    if (const int rc = latent_grad_launch<false>(__func__, points, target, seg_off, nshapes, zb1, zb5, packed, nullptr, cutoff, win_start,
                                                 win_count, tiles, ntiles, partials, stream))
        return rc;
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_sdfnet_latent_reduce(const float* partials, const int64_t* tile_off, const int64_t* seg_off, long nshapes, long win_count,
                            float* t1, float* t5, float* loss, hipStream_t stream) {
    SG_CHECK_ARG(partials && tile_off && seg_off && t1 && t5 && loss && nshapes >= 1 && nshapes < (1L << 31));
    latent_reduce_launch<false>(partials, tile_off, seg_off, nshapes, win_count, t1, t5, loss, nullptr, stream);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_sdfnet_latent_pose_grad(const float* points, const float* target, const int64_t* seg_off, long nshapes, const float* zb1,
                               const float* zb5, const float* packed, const float* pose, float cutoff, long win_start,
                               long win_count, const int* tiles, long ntiles, float* partials, hipStream_t stream) {
    SG_CHECK_ARG(points && target && seg_off && zb1 && zb5 && packed && pose && tiles && partials);
    SG_CHECK_ARG(nshapes >= 1 && win_start >= 0 && ntiles >= 1 && ntiles < (1L << 31) && cutoff >= 0.f);
    if (const int rc = latent_grad_launch<true>(__func__, points, target, seg_off, nshapes, zb1, zb5, packed, pose, cutoff, win_start,
                                                win_count, tiles, ntiles, partials, stream))
        return rc;
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_sdfnet_latent_pose_reduce(const float* partials, const int64_t* tile_off, const int64_t* seg_off, long nshapes,
                                 long win_count, float* t1, float* t5, float* loss, float* gpose, hipStream_t stream) {
    SG_CHECK_ARG(partials && tile_off && seg_off && t1 && t5 && loss && gpose && nshapes >= 1 && nshapes < (1L << 31));
    latent_reduce_launch<true>(partials, tile_off, seg_off, nshapes, win_count, t1, t5, loss, gpose, stream);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

}  // extern "C"
