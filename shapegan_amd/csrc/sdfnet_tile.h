// shapegan_amd/csrc/sdfnet_tile.h — the forward tile of the fused SDFNet MLP (sdfnet.hip) and what it runs on: the packed
// weight layout, the MFMA GEMM loops and sdfnet_fwd_tile.  A header so that a kernel in another file can run the same eight
// layers on its own points; sdfnet.hip holds the kernels and entry points of the MLP itself.  Users: sdfnet.hip (sg_sdfnet_fwd /
// sg_sdfgen_fwd and, for the fragment helpers, the training backward), raymarch.hip (the sphere tracer) and, through
// sdfnet_frozen.h, latent_fit.hip (K7c) and sdfnet_project.hip (K7d), which also run the chain back on the tile.
#pragma once
#include "common.h"

// cache policy of the activation / dZ image stores (aux of the raw buffer store: 0 default, 2 = nt: streaming, evict-first in L2 —
// the images are written once and read by a later kernel, the weight packs every wave streams should keep the L2)
#ifndef SG_IMG_AUX
#define SG_IMG_AUX 2
#endif   // (the tile layout of the partial sums is part of the ABI: include/shapegan_hip.h)

namespace sg {

constexpr int kH = 256;  // SDF_NET_BREADTH, model/sdf_net.py:21

struct SdfPackLayout {
    int KU, KUp, KUr;
    long F1, F2, F3, F4, F5x, F5i, F6, F7;  // forward packs: A(i=out, k=in)
    long T1, T2, T3, T4, T5x, T5i, T6, T7;  // transposed packs: A(i=in, k=out)
    long W8, B;                              // w8[256], b[8][256]
    long G, Be;                              // LayerNorm weight / bias [7][256] each (the SDFGenerator form)
    long total;
};
static SdfPackLayout make_layout(int KU) {
    SdfPackLayout L;
    L.KU = KU;
    L.KUp = (KU + 7) / 8 * 8;
    L.KUr = (KU + 31) / 32 * 32;
    long o = 0;
    auto take = [&](long n) {
        long r = o;
        o += n;
        return r;
    };
    L.F1 = take((long)kH * L.KUp);
    L.F2 = take(kH * kH);
    L.F3 = take(kH * kH);
    L.F4 = take(kH * kH);
    L.F5x = take(kH * kH);
    L.F5i = take((long)kH * L.KUp);
    L.F6 = take(kH * kH);
    L.F7 = take(kH * kH);
    L.T1 = take((long)L.KUr * kH);
    L.T2 = take(kH * kH);
    L.T3 = take(kH * kH);
    L.T4 = take(kH * kH);
    L.T5x = take(kH * kH);
    L.T5i = take((long)L.KUr * kH);
    L.T6 = take(kH * kH);
    L.T7 = take(kH * kH);
    L.W8 = take(kH);
    L.B = take(8 * kH);
    L.G = take(7 * kH);
    L.Be = take(7 * kH);
    L.total = o;
    return L;
}

// acc[t] += A_tile(32 x K) * B(K x [t*32, t*32+32)) ; wp = this wave's packed A rows (wave-uniform), Bs = LDS [K][ld].
// Software-pipelined like the conv halo kernels: A fragments come through a 4-deep ring of buffer loads (scalar base,
// fixed lane offset, k-group in the scalar offset), the B fragments of k-group sq+1 are read from LDS (immediate offsets
// from one running address) while the 4*NT MFMAs of group sq run; sched_barriers keep the loads where they are issued.
// One VALU instruction (the LDS address step) per 4*NT MFMAs.
template <int NT, int RING = 4, int TS = 32>   // TS: floats between the column tiles of a row (32: one [K][ld] tile; else one tile per chain)
__device__ __forceinline__ void mlp_gemm(f32x16 (&acc)[NT], const float4* __restrict__ wp, int nsq,
                                         const float* __restrict__ Bs, int ld, int lane) {
    const int r = lane & 31, kh = lane >> 5;
    // the packed rows are per wave: make the base a scalar so that the loads need no vector address arithmetic
    const unsigned long long wq = (unsigned long long)wp;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)wq), hi = __builtin_amdgcn_readfirstlane((unsigned)(wq >> 32));
    const __amdgpu_buffer_rsrc_t wres = make_rsrc((const void*)(((unsigned long long)hi << 32) | lo));
    const unsigned wvoff = lane * 16;
    const lds_float* bp = (const lds_float*)Bs + kh * ld + r;
    const int last = nsq - 1;
    float4 ar[RING];
#pragma unroll
    for (int u = 0; u < RING; ++u) ar[u] = buf_load4(wres, wvoff, (unsigned)(u < last ? u : last) * 1024u);
    float b[4][NT], bn[4][NT];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < NT; ++t) b[j][t] = bp[j * 2 * ld + t * TS];
    auto group = [&](float4 a, int sq) __attribute__((always_inline)) {
        // B of the next group (the last group re-reads its own: no branch)
        const lds_float* nb = bp + (sq < last ? 8 * ld : 0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < NT; ++t) bn[j][t] = nb[j * 2 * ld + t * TS];
        bp = nb;
        __builtin_amdgcn_sched_barrier(0);
        const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], b[j][t], acc[t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < NT; ++t) b[j][t] = bn[j][t];
    };
    int sq = 0;
    for (; sq + RING <= nsq; sq += RING) {
#pragma unroll
        for (int u = 0; u < RING; ++u) {
            const float4 a = ar[u];
            const int nx = sq + u + RING;
            ar[u] = buf_load4(wres, wvoff, (unsigned)(nx < last ? nx : last) * 1024u);
            group(a, sq + u);
        }
    }
    // remainder (group count not a multiple of the ring): the ring already holds these groups
#pragma unroll
    for (int u = 0; u < RING - 1; ++u)
        if (sq + u < nsq) group(ar[u], sq + u);
}

// The same GEMM with the weight ring as caller-visible state, for the 256-wide layers that follow one another:
//   * wring_start() issues the first RING weight loads of a layer.  The caller does that BEFORE the stores of the previous
//     layer's epilogue: vmcnt retires in order, so a ring started after the 32 - 64 activation stores of an epilogue makes the
//     first MFMA of the next layer wait for every one of those stores to be acknowledged by memory;
//   * hook() runs once, right after the LAST weight load of the layer has been issued (RING groups before the end): loads the
//     caller wants to have arrived by the end of the GEMM (the backward's ReLU-mask operand) go there — issued earlier they
//     would sit in front of the remaining weight loads in the in-order return queue and stall the MFMAs for a full memory
//     latency, issued later their latency is exposed in the epilogue.
template <int RING>
struct WRing {
    __amdgpu_buffer_rsrc_t res;
    float4 ar[RING];
};
template <int RING>
__device__ __forceinline__ void wring_start(WRing<RING>& w, const float4* __restrict__ wp, int lane) {
    const unsigned long long wq = (unsigned long long)wp;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)wq), hi = __builtin_amdgcn_readfirstlane((unsigned)(wq >> 32));
    w.res = make_rsrc((const void*)(((unsigned long long)hi << 32) | lo));
#pragma unroll
    for (int u = 0; u < RING; ++u) w.ar[u] = buf_load4(w.res, lane * 16u, (unsigned)u * 1024u);
}
template <int NT, int RING, int NSQ, class Hook>
__device__ __forceinline__ void mlp_gemm_ring(f32x16 (&acc)[NT], WRing<RING>& w, const float* __restrict__ Bs, int ld, int lane,
                                              Hook hook) {
    static_assert(NSQ >= 2 * RING, "ring deeper than the GEMM");
    const int r = lane & 31, kh = lane >> 5;
    const unsigned wvoff = lane * 16;
    const lds_float* bp = (const lds_float*)Bs + kh * ld + r;
    float b[4][NT], bn[4][NT];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < NT; ++t) b[j][t] = bp[j * 2 * ld + t * 32];
#pragma unroll
    for (int sq = 0; sq < NSQ; ++sq) {
        const float4 a = w.ar[sq % RING];
        if (sq + RING < NSQ) w.ar[sq % RING] = buf_load4(w.res, wvoff, (unsigned)(sq + RING) * 1024u);
        if (sq + RING == NSQ) hook();
        const lds_float* nb = bp + (sq + 1 < NSQ ? 8 * ld : 0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < NT; ++t) bn[j][t] = nb[j * 2 * ld + t * 32];
        bp = nb;
        __builtin_amdgcn_sched_barrier(0);
        const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], b[j][t], acc[t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int t = 0; t < NT; ++t) b[j][t] = bn[j][t];
    }
}

// row of accumulator element q of a 32x32 MFMA tile for the half-wave kh; frag_rowoff: the part a lane that has 4 kh in its base adds
__device__ __forceinline__ int frag_rowoff(int q) { return (q & 3) + 8 * (q >> 2); }
__device__ __forceinline__ int frag_row(int q, int kh) { return frag_rowoff(q) + 4 * kh; }

// v + (v of another lane), the lane picked by a DPP control; half_wave_sum: lane 31 / 63 ends up with the sum over its half-wave
// (the 32 points of a column tile)
template <int CTRL, int ROWMASK>
__device__ __forceinline__ float dpp_add(float v) {
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROWMASK, 0xf, false));
}
__device__ __forceinline__ float half_wave_sum(float v) {
    v = dpp_add<0xB1, 0xf>(v);
    v = dpp_add<0x4E, 0xf>(v);
    v = dpp_add<0x141, 0xf>(v);
    v = dpp_add<0x140, 0xf>(v);
    return dpp_add<0x142, 0xa>(v);
}

// The activation buffer of a training call: [7][256][ldn] fp32 images H1..H7 followed by the sign masks, unsigned short
// [7][16][ldn]: bit q of masks[l][2 w + kh][p] = (H_{l+1}[32 w + frag_row(q, kh)][p] > 0)  (sg_sdfnet_acts_floats in the header).
__host__ __device__ __forceinline__ const unsigned short* sdf_mask_base(const float* acts, long ldn) {
    return reinterpret_cast<const unsigned short*>(acts + 7L * kH * ldn);
}

struct SdfFwdArgs {
    const float* points;    // [*,3]
    long points_period;     // >0: point index = p % period (shared voxel grid); 0: p
    const float* latent;    // per-point mode: [N,L] rows, or table rows if latent_idx
    const int64_t* latent_idx;  // optional [N] row index into latent
    int L;
    const float* packed;
    SdfPackLayout lay;
    const float* zb1;  // per-shape mode: [S][256] (bias of layer 1 incl. latent part)
    const float* zb5;
    long pps;          // points per shape (per-shape mode, uniform segments)
    const int* sid;    // per-shape mode with ragged segments: shape index of every point (NULL: p / pps)
    float* out;        // [N]
    float* acts;       // optional [7][256][ldn]
    long ldn;
    long N;
    long nbig;         // workgroups [0, nbig): full tiles; the rest: kSmallTile points each
    float eps;         // NORM: LayerNorm epsilon
};

// The LayerNorm form (NORM; SDFGenerator, model/point_sdf_net.py:49-119 with hidden_channels 256, num_layers 8): the same eight
// layers with x = relu(LayerNorm(lin(x) [+ z_lin(z)])) (:104-116) instead of relu(lin(x)), no tanh at the end, and
// cat([x, pos]) (:100) where SDFNet has cat(x, input).  A point's 256 features are spread over the eight waves (32 rows each), so
// a layer's statistics are combined through LDS: every wave reduces its 32 rows of a point to (mean, sum of squared deviations)
// in registers (16 in-lane terms + one cross-half exchange), parks the pair in `red` in front of the barrier the write-back
// has anyway, and combines the eight pairs behind it (Chan's formula for equal counts) — no extra barrier, no E[x^2] - E[x]^2
// cancellation.  In training the images hold xhat = (x - mean) * rstd (the LayerNorm backward needs it where the ReLU is off
// too; the weight-gradient GEMM applies relu(gamma xhat + beta) when it loads them), the sign masks are those of the ReLU
// input, and rstd [7][ldn] follows the masks.
__host__ __device__ __forceinline__ const float* sdf_rstd_base(const float* acts, long ldn) { return acts + 7L * kH * ldn + 56L * ldn; }

// What a tile reads and writes, point by point (gp: the point's index in the launch, gp < a.N for the points that exist):
//   coord(a, gp, c)  coordinate c of the point                         (here: points[gp % period])
//   ragged(a)        per-point shape index (else shape = p0 / pps)       (here: sid given)
//   shape(a, gp)     the shape index of a point, ragged mode             (here: sid[gp])
//   store(a, gp, v)  the epilogue, called by the threads tid < P with the last layer's pre-activation v of point p0 + tid, for
//                    every tid (also gp >= a.N: wave 0 runs it whole, so a store may use wave-wide operations)
// SdfPointIo is the MLP's own (sg_sdfnet_fwd / sg_sdfgen_fwd); the sphere tracer (raymarch.hip) supplies another.
template <bool NORM>
struct SdfPointIo {
    __device__ __forceinline__ float coord(const SdfFwdArgs& a, long gp, int c) const {
        const long pi = a.points_period > 0 ? gp % a.points_period : gp;
        return a.points[pi * 3 + c];
    }
    __device__ __forceinline__ bool ragged(const SdfFwdArgs& a) const { return a.sid != nullptr; }
    __device__ __forceinline__ int shape(const SdfFwdArgs& a, long gp) const { return a.sid[gp < a.N ? gp : a.N - 1]; }
    __device__ __forceinline__ void store(const SdfFwdArgs& a, long gp, float v) const {
        if (gp < a.N) a.out[gp] = NORM ? v : tanhf(v);   // (SDFGenerator ends in a plain Linear, point_sdf_net.py:106-111)
    }
};

// KEEP: the sign word of every hidden layer (the one TRAIN stores to `acts`, same bit order) is handed to io.keep(layer, words) instead
// of memory — for a kernel that runs the backward chain of the tile itself (sdfnet_frozen.h).  Off in every other instantiation.
// The tile's dynamic LDS, the size every kernel that calls sdfnet_fwd_tile launches with: H [256][P], X [KUp][P + 1], the layer-8
// partials [16][P], the biases [7][256] and, NORM, gamma / beta of the layer in flight [8][64].
static size_t sdf_fwd_lds_bytes(int P, int KUp, bool norm = false) {
    return ((size_t)kH * P + (size_t)KUp * (P + 1) + 16 * P + 7 * kH + (norm ? 8 * 64 : 0)) * sizeof(float);
}

template <int P, bool SHAPE_BIAS, bool TRAIN, bool NORM = false, class Io = SdfPointIo<NORM>, bool KEEP = false>   // TRAIN: `acts` is given (H images + sign masks are written)
__device__ __forceinline__ void sdfnet_fwd_tile(const SdfFwdArgs& a, const long p0, const Io& io = Io()) {
    constexpr int NT = P / 32;
    constexpr int LDX = P + 1;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Hs = smem;                // [256][P]
    float* Xs = Hs + kH * P;         // [KUp][LDX]
    float* red = Xs + a.lay.KUp * LDX;  // [16][P]
    float* Bl = red + 16 * P;           // [7][256]: the bias vectors (see init_acc_lds)
    float* GBs = Bl + 7 * kH;           // NORM: [8 waves][gamma 32 | beta 32] of the layer in flight

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kh = lane >> 5, r = lane & 31;
    const int KU = a.lay.KU, KUp = a.lay.KUp;
    // The seven bias vectors go to LDS once per tile.  A layer used to start with four 16-byte global loads of its bias into the
    // accumulators and an s_waitcnt for them in front of its first MFMA — and vmcnt counts in issue order, so that wait also drained
    // everything older: the weight ring of the layer (started early on purpose) and, in training, the 32 activation-image stores
    // of the previous write-back (ISA listing, round 4).  From LDS the accumulators are initialised under lgkmcnt only.
    for (int e = tid; e < 7 * kH; e += 512) Bl[e] = (a.packed + a.lay.B)[e];

    // ---- stage X = [xyz | latent] feature-major ----
    for (int e = tid; e < 3 * P; e += 512) {
        const int p = e / 3, c = e - p * 3;
        const long gp = p0 + p;
        float v = 0.f;
        if (gp < a.N) v = io.coord(a, gp, c);
        Xs[c * LDX + p] = v;
    }
    if constexpr (!SHAPE_BIAS) {
        const int L = a.L;
        for (int e = tid; e < P * L; e += 512) {
            const int p = e / L, k = e - p * L;
            const long gp = p0 + p;
            float v = 0.f;
            if (gp < a.N) {
                const long row = a.latent_idx ? (long)a.latent_idx[gp] : gp;
                v = a.latent[row * L + k];
            }
            Xs[(3 + k) * LDX + p] = v;
        }
    }
    for (int e = tid; e < (KUp - KU) * P; e += 512) {
        const int k = KU + e / P, p = e % P;
        Xs[k * LDX + p] = 0.f;
    }
    __syncthreads();

    const float* bias = a.packed + a.lay.B;
    const long shape = (SHAPE_BIAS && !io.ragged(a)) ? (p0 / a.pps) : 0;
    const float4* pk = reinterpret_cast<const float4*>(a.packed);

    f32x16 acc[NT];
    auto init_acc = [&](const float* b) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float bv = b[wave * 32 + frag_row(q, kh)];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t][q] = bv;
        }
    };
    auto init_acc_lds = [&](int layer) {      // the same from the LDS copy of bias vector `layer`
        const lds_float* b = (const lds_float*)Bl + layer * kH + wave * 32;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float bv = b[frag_row(q, kh)];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t][q] = bv;
        }
    };
    // ragged per-shape mode: every point (= fragment column) looks its folded bias row up by its own shape index
    int psid[NT];
    if (SHAPE_BIAS && io.ragged(a)) {
#pragma unroll
        for (int t = 0; t < NT; ++t) psid[t] = io.shape(a, p0 + t * 32 + r);
    }
    auto init_acc_sid = [&](const float* zb) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float* b = zb + (long)psid[t] * kH + wave * 32;
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[t][q] = b[frag_row(q, kh)];
        }
    };
    // training: H_l also goes to `acts` — buffer stores from a scalar base (this wave's row block at the tile's first point),
    // lane offset = (4 kh) rows + point, fragment row in the scalar offset; lanes beyond N carry an out-of-range offset (dropped
    // by the hardware), so the epilogue has neither 64-bit address arithmetic nor exec-mask branches
    const int wrow = __builtin_amdgcn_readfirstlane(wave) * 32;
    unsigned astore[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
        astore[t] = p0 + t * 32 + r < a.N ? (unsigned)((4L * kh * a.ldn + t * 32 + r) * 4) : kBufOutside;
    // ... and the SIGN MASK of H_l, 1 bit per element: a lane holds 16 rows (q) of one point per column tile, so it packs them
    // into one 16-bit word at masks[layer][16-row group = 2 wave + kh][point] (sg_sdfnet_mask_* in the header): 1/32 of the H
    // traffic.  The backward reads ReLU'(.) from these words instead of re-reading the fp32 images.
    unsigned mstore[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
        mstore[t] = p0 + t * 32 + r < a.N ? (unsigned)(((long)kh * a.ldn + t * 32 + r) * 2) : kBufOutside;
    // (`save` stays a run-time condition even in the TRAIN instantiation: as a compile-time constant the stores lose their place
    // in the schedule, the write-back's live ranges grow and the kernel no longer fits the 128 VGPRs of two workgroups per CU)
    // NORM: this lane's LayerNorm weight (lanes 0..31) / bias (32..63) element of a layer, row wrow + r: requested in front of the
    // layer's GEMM, parked in LDS behind it (in front of the next weight ring: its wait covers only loads that were consumed)
    float gbv = 0.f;
    auto gb_load = [&](int layer) __attribute__((always_inline)) {
        if constexpr (NORM) gbv = (a.packed + (kh ? a.lay.Be : a.lay.G))[layer * kH + wave * 32 + r];
    };
    auto gb_commit = [&]() __attribute__((always_inline)) {
        if constexpr (NORM) GBs[wave * 64 + lane] = gbv;
    };
    auto writeback = [&](int layer) {  // H <- relu(acc) (NORM: relu(LayerNorm(acc))); optionally save
        float mean[NT], rstd[NT];
        if constexpr (NORM) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float s = 0.f;
#pragma unroll
                for (int q = 0; q < 16; ++q) s += acc[t][q];
                s += __shfl_xor(s, 32, 64);
                const float mw = s * (1.f / 32.f);
                float d = 0.f;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const float e = acc[t][q] - mw;
                    d = fmaf(e, e, d);
                }
                d += __shfl_xor(d, 32, 64);
                if (kh == 0) {
                    red[(2 * wave) * P + t * 32 + r] = mw;
                    red[(2 * wave + 1) * P + t * 32 + r] = d;
                }
            }
        }
        __syncthreads();
        const bool save = (NORM ? TRAIN : true) && a.acts != nullptr;
        if constexpr (NORM) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const lds_float* rp = (const lds_float*)red + t * 32 + r;
                float sum = 0.f;
#pragma unroll
                for (int w = 0; w < 8; ++w) sum += rp[(2 * w) * P];
                const float m = sum * 0.125f;
                float M2 = 0.f;
#pragma unroll
                for (int w = 0; w < 8; ++w) {
                    const float e = rp[(2 * w) * P] - m;
                    M2 += rp[(2 * w + 1) * P];
                    M2 = fmaf(32.f * e, e, M2);
                }
                mean[t] = m;
                rstd[t] = 1.f / sqrtf(M2 * (1.f / 256.f) + a.eps);
                if (TRAIN && save && wave == 0 && kh == 0 && p0 + t * 32 + r < a.N)
                    const_cast<float*>(sdf_rstd_base(a.acts, a.ldn))[(long)layer * a.ldn + p0 + t * 32 + r] = rstd[t];
            }
        }
        const __amdgpu_buffer_rsrc_t ares = make_rsrc(a.acts + ((long)layer * kH + wrow) * a.ldn + p0);
        unsigned mk[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) mk[t] = 0u;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int row = wave * 32 + frag_row(q, kh);
            float gq = 1.f, bq = 0.f;
            if constexpr (NORM) {
                gq = GBs[wave * 64 + frag_row(q, kh)];
                bq = GBs[wave * 64 + 32 + frag_row(q, kh)];
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float v, img;
                if constexpr (NORM) {
                    img = (acc[t][q] - mean[t]) * rstd[t];
                    acc[t][q] = fmaf(gq, img, bq);      // (the sign mask below is that of the ReLU input)
                    v = fmaxf(acc[t][q], 0.f);
                } else {
                    v = img = fmaxf(acc[t][q], 0.f);
                }
                Hs[row * P + t * 32 + r] = v;
                if (save)
                    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, img), ares, (int)astore[t],
                                                          (int)(frag_rowoff(q) * a.ldn * 4), SG_IMG_AUX);
            }
        }
        if constexpr (TRAIN) {
            if (save) {
                // sign word: mk = 2 mk + (acc > 0), rows 15 .. 0, so that bit q ends up belonging to row q — compare into vcc and
                // add-with-carry, two VALU instructions per element (the C form `mk |= v > 0 ? 1 << q : 0` took three and kept
                // 16 more values live).  The accumulators were all read by the loop above: no MFMA result hazard is left.
#pragma unroll
                for (int q = 15; q >= 0; --q)
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        asm volatile("v_cmp_lt_f32 vcc, 0, %1\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(mk[t]) : "v"(acc[t][q]) : "vcc");
                const __amdgpu_buffer_rsrc_t mres =
                    make_rsrc(sdf_mask_base(a.acts, a.ldn) + ((long)layer * 16 + (wrow >> 4)) * a.ldn + p0);
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    __builtin_amdgcn_raw_buffer_store_b16((unsigned short)mk[t], mres, (int)mstore[t], 0, 0);
            }
        }
        if constexpr (KEEP) {
            static_assert(!NORM && !TRAIN, "the kept sign words are those of the plain ReLU form");
#pragma unroll
            for (int q = 15; q >= 0; --q)
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    asm volatile("v_cmp_lt_f32 vcc, 0, %1\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(mk[t]) : "v"(acc[t][q]) : "vcc");
            io.keep(layer, mk);
        }
        __syncthreads();
    };
    auto wtile = [&](long off, int nsq) { return pk + (off >> 2) + (long)wave * nsq * 64; };

    // layer 1: K over X
    if (SHAPE_BIAS && io.ragged(a))
        init_acc_sid(a.zb1);
    else
        SHAPE_BIAS ? init_acc(a.zb1 + shape * kH) : init_acc_lds(0);
    gb_load(0);
    mlp_gemm<NT>(acc, wtile(a.lay.F1, KUp / 8), KUp / 8, Xs, LDX, lane);
    gb_commit();
    // the weight ring of the next 256-wide layer is started before each write-back (its stores would otherwise sit in front of
    // the first weight loads in the in-order return queue, see WRing)
    WRing<4> wr;
    auto noop = []() {};
    auto next_ring = [&](long off) __attribute__((always_inline)) {
        wring_start(wr, wtile(off, kH / 8), lane);
        __builtin_amdgcn_sched_barrier(0);
    };
    next_ring(a.lay.F2);
    writeback(0);
    // layers 2..4
    const long Fnext[3] = {a.lay.F3, a.lay.F4, a.lay.F5x};
#pragma unroll 1
    for (int l = 0; l < 3; ++l) {
        init_acc_lds(l + 1);
        gb_load(l + 1);
        mlp_gemm_ring<NT, 4, kH / 8>(acc, wr, Hs, P, lane, noop);
        gb_commit();
        next_ring(Fnext[l]);
        writeback(l + 1);
    }
    // layer 5: K over H (256) then X (skip connection, model/sdf_net.py:59)
    if (SHAPE_BIAS && io.ragged(a))
        init_acc_sid(a.zb5);
    else
        SHAPE_BIAS ? init_acc(a.zb5 + shape * kH) : init_acc_lds(4);
    gb_load(4);
    mlp_gemm_ring<NT, 4, kH / 8>(acc, wr, Hs, P, lane, noop);
    mlp_gemm<NT>(acc, wtile(a.lay.F5i, KUp / 8), KUp / 8, Xs, LDX, lane);
    gb_commit();
    next_ring(a.lay.F6);
    writeback(4);
    // layers 6, 7
    init_acc_lds(5);
    gb_load(5);
    mlp_gemm_ring<NT, 4, kH / 8>(acc, wr, Hs, P, lane, noop);
    gb_commit();
    next_ring(a.lay.F7);
    writeback(5);
    init_acc_lds(6);
    gb_load(6);
    mlp_gemm_ring<NT, 4, kH / 8>(acc, wr, Hs, P, lane, noop);
    gb_commit();
    writeback(6);
    // layer 8: 256 -> 1, tanh.  The dot product is cut into sixteen 16-row groups summed in a fixed order, whatever the tile
    // size (a thread takes P / 32 groups of its point), so that a point's output does not depend on the tile it falls into.
    {
        constexpr int PARTS = 512 / P;     // threads per point
        constexpr int SUB = 16 / PARTS;    // row groups per thread
        const int p = tid % P, part = tid / P;
        const float* w8 = a.packed + a.lay.W8;
#pragma unroll
        for (int u = 0; u < SUB; ++u) {
            const int g = part * SUB + u;
            float s = 0.f;
#pragma unroll
            for (int k = 16 * g; k < 16 * g + 16; ++k) s = fmaf(w8[k], Hs[k * P + p], s);
            red[g * P + p] = s;
        }
        __syncthreads();
        if (tid < P) {
            float v = bias[7 * kH];
#pragma unroll
            for (int q = 0; q < 16; ++q) v += red[q * P + tid];
            io.store(a, p0 + tid, v);
        }
    }
}

}  // namespace sg
