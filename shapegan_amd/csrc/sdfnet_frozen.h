// shapegan_amd/csrc/sdfnet_frozen.h — SDFNet with FROZEN weights on a 32-point tile of one shape, per-shape bias mode: what the latent
// fit without and with a pose (latent_fit.hip, K7c and K7e) and the level-set projection (sdfnet_project.hip, K7d) share.  All run
// sdfnet_fwd_tile with KEEP, hold the seven sign words a lane produces in registers instead of storing them, and walk the chain back
// through the transposed packs of the same weight image, dZ_l = (T_{l+1} dZ_{l+1}) * ReLU'(H_l), in the forward's own [256][P] LDS tile.
// They differ in the epilogue of the forward (Io::store: what dz8 is) and in what they do with dZ5 and dZ1 (the functor of
// sdfnet_frozen_bwd_tile): row sums over the tile's points (the fit), the point gradient (SdfPointGrad: K7d and K7e), or both.
#pragma once
#include "sdfnet_tile.h"

namespace sg {

// The part of a tile's Io that keeps the sign words: `signs` points at the kernel's seven registers.
struct SdfSignKeeper {
    unsigned* signs;      // registers [7]
    __device__ __forceinline__ bool ragged(const SdfFwdArgs&) const { return false; }
    __device__ __forceinline__ int shape(const SdfFwdArgs&, long) const { return 0; }
    __device__ __forceinline__ void keep(int layer, const unsigned (&mk)[1]) const {
        // (select chain with constant indices: `layer` is a loop variable in the forward, a dynamic index would put the words in scratch)
#pragma unroll
        for (int l = 0; l < 7; ++l) signs[l] = layer == l ? mk[0] : signs[l];
    }
};

// A table row (shape, first point of the tile within the shape's used points) and the shape's run; a row that names no shape has n = 0.
struct SdfTileRow {
    int s, i0;
    long beg, n;
};
__device__ __forceinline__ SdfTileRow sdf_tile_row(const int* tiles, const int64_t* seg_off, long S, long tile) {
    SdfTileRow t{tiles[2 * tile], tiles[2 * tile + 1], 0, 0};
    if (t.s >= 0 && t.s < S) {
        t.beg = seg_off[t.s];
        t.n = seg_off[t.s + 1] - t.beg;
    }
    return t;
}

// The points of a row's tile that a call uses.  Shape s uses m = n or min(win_count, n) of its points, the i-th being
// beg + (win_start + i) mod n (a window that wraps around the cloud); the tile holds cnt <= P of them from i0 on, cnt <= 0 for a row that
// names nothing.  m is the divisor of the shape's mean.
struct SdfTileWindow {
    long beg, n, m, cnt, first;      // first = (win_start + i0) mod n
    __device__ __forceinline__ long index(long gp) const {
        const long i = first + gp;      // (gp < cnt <= n and first < n: one wrap at most)
        return beg + (i >= n ? i - n : i);
    }
};
__device__ __forceinline__ SdfTileWindow sdf_tile_window(const SdfTileRow& row, long win_start, long win_count, int P) {
    SdfTileWindow w{row.beg, row.n, 0, 0, 0};
    w.m = row.n <= 0 ? 0 : (win_count <= 0 || win_count > row.n ? row.n : win_count);
    w.cnt = row.i0 < 0 ? 0 : w.m - row.i0;
    if (w.cnt > P) w.cnt = P;
    if (w.cnt > 0) w.first = (win_start + row.i0) % row.n;
    return w;
}

// The forward's arguments for one tile of `cnt` points that takes its bias rows from zb1 / zb5 directly (shape = p0 / pps = 0), stores
// nothing and leaves the points to its Io.
__device__ __forceinline__ SdfFwdArgs sdf_frozen_tile_args(const float* points, const float* packed, const SdfPackLayout& lay,
                                                           const float* zb1_row, const float* zb5_row, long cnt) {
    SdfFwdArgs a;
    a.points = points;
    a.points_period = 0;
    a.latent = nullptr;
    a.latent_idx = nullptr;
    a.L = 0;
    a.packed = packed;
    a.lay = lay;
    a.zb1 = zb1_row;
    a.zb5 = zb5_row;
    a.pps = 1L << 40;
    a.sid = nullptr;
    a.out = nullptr;
    a.acts = nullptr;
    a.ldn = 0;
    a.N = cnt;
    a.nbig = 0;
    a.eps = 0.f;
    return a;
}

// The chain back from dz8 [P] (LDS; 0 for the points beyond the tile's count) to dZ1, run by the whole workgroup behind a barrier that
// follows the forward's epilogue.  s0 .. s6 are the lane's kept words of layers 1 .. 7.  fn(i, q, g) is called for each of the lane's
// 16 elements of image i = 5 .. 0 (dZ_{i+1}): g is element q, row wave * 32 + frag_row(q, kh) of point lane & 31, ReLU' applied and
// (i > 0) written back to the tile.  Nothing reads the tile after image 0, which is handed to fn only.
// (The words come by value and are picked by a select chain on constants: through a pointer or an array reference they end up in
// scratch and are loaded with a dynamic offset — DESIGN 3.13 has the compiler's figures.)
template <int P, class Fn>
__device__ __forceinline__ void sdfnet_frozen_bwd_tile(const float* packed, const SdfPackLayout& lay, float* Hs, const unsigned s0,
                                                       const unsigned s1, const unsigned s2, const unsigned s3, const unsigned s4,
                                                       const unsigned s5, const unsigned s6, const float* dz8s, Fn fn) {
    static_assert(P == 32, "one accumulator tile per wave");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kh = lane >> 5, r = lane & 31;
    const float4* pk = reinterpret_cast<const float4*>(packed);
    auto wtile = [&](long off) { return pk + (off >> 2) + (long)wave * (kH / 8) * 64; };
    // this lane's element q of the tile: row wave * 32 + frag_row(q, kh), point r
    lds_float* const hw = (lds_float*)Hs + (wave * 32 + 4 * kh) * P + r;
    auto noop = []() {};
    WRing<4> wr;
    wring_start(wr, wtile(lay.T7), lane);
    __builtin_amdgcn_sched_barrier(0);
    // dZ7 = (w8 (x) dz8) * ReLU'(H7)
    {
        const float* w8 = packed + lay.W8;
        const float d8 = dz8s[r];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float wv = w8[wave * 32 + frag_row(q, kh)];
            hw[frag_rowoff(q) * P] = ((s6 >> q) & 1u) ? wv * d8 : 0.f;
        }
    }
    __syncthreads();
    // images 5 .. 0 (dZ6 .. dZ1): GEMM with the transposed pack of the layer above, ReLU' from the kept word, back into the tile
    f32x16 acc[1];
#pragma unroll 1
    for (int i = 5; i >= 0; --i) {
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[0][q] = 0.f;
        mlp_gemm_ring<1, 4, kH / 8>(acc, wr, Hs, P, lane, noop);
        if (i > 0) {
            const long nxt = i == 5 ? lay.T6 : i == 4 ? lay.T5x : i == 3 ? lay.T4 : i == 2 ? lay.T3 : lay.T2;
            wring_start(wr, wtile(nxt), lane);
            __builtin_amdgcn_sched_barrier(0);
        }
        unsigned mk = s0;
        mk = i == 1 ? s1 : mk;
        mk = i == 2 ? s2 : mk;
        mk = i == 3 ? s3 : mk;
        mk = i == 4 ? s4 : mk;
        mk = i == 5 ? s5 : mk;
        __syncthreads();      // every wave has read the tile
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const float g = ((mk >> q) & 1u) ? acc[0][q] : 0.f;
            if (i > 0) hw[frag_rowoff(q) * P] = g;
            fn(i, q, g);
        }
        if (i > 0) __syncthreads();
    }
}

// The point gradient of a tile, g[p] = W5[:, 256:259]^T dZ5[:, p] + W1[:, 0:3]^T dZ1[:, p]: every lane multiplies the 16 rows of dZ5
// (later dZ1) it holds for its point by the matching rows of the point columns — K split over the eight waves, VALU, while the tile
// still holds the image.  The forward's bias vectors (7 KB behind H, X and the layer-8 partials) are dead once its last GEMM has
// started and are staged again by every forward: the chain back keeps the point columns there, Wx[2][256][3].
static_assert(2 * kH * 3 <= 7 * kH, "the point columns fit where the forward keeps its biases");
template <int P>
struct SdfPointGrad {
    float* Wx;
    const lds_float* wxw;               // the rows of this lane's elements of the tile: wave * 32 + frag_row(q, kh)
    float gx = 0.f, gy = 0.f, gz = 0.f;      // this lane's 16 rows of W5x^T dZ5 + W1x^T dZ1 for point lane & 31
    __device__ __forceinline__ SdfPointGrad(float* smem, const SdfPackLayout& lay)
        : Wx(smem + kH * P + lay.KUp * (P + 1) + 16 * P),
          wxw((const lds_float*)Wx + ((threadIdx.x >> 6) * 32 + 4 * ((threadIdx.x & 63) >> 5)) * 3) {}
    // by the whole workgroup between the forward and the barrier in front of sdfnet_frozen_bwd_tile
    __device__ __forceinline__ void stage(const float* packed, const SdfPackLayout& lay) const {
        // element M(c, k) of a transposed 32-row pack (pack_mfma_a_kernel): ((k >> 3) * 64 + c + 32 (k & 1)) * 4 + ((k >> 1) & 3)
        for (int e = threadIdx.x; e < 2 * kH * 3; e += 512) {
            const int l = e / (kH * 3), k = (e - l * kH * 3) / 3, c = e % 3;
            Wx[e] = packed[(l ? lay.T5i : lay.T1) + ((k >> 3) * 64 + c + 32 * (k & 1)) * 4 + ((k >> 1) & 3)];
        }
    }
    // from the chain's functor, for the elements of images i == 4 (dZ5) and i == 0 (dZ1)
    __device__ __forceinline__ void add(int i, int q, float g) {
        const lds_float* w = wxw + (i == 0 ? 0 : kH * 3) + frag_rowoff(q) * 3;
        gx = __builtin_fmaf(w[0], g, gx);
        gy = __builtin_fmaf(w[1], g, gy);
        gz = __builtin_fmaf(w[2], g, gz);
    }
    // The two half-waves hold rows 4 kh + {0..3, 8..11, ...} of the same point; their sum goes to gp [8][3][P] (LDS), which the
    // caller adds in wave order behind a barrier.
    __device__ __forceinline__ void partials(float* gp) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31;
        gx += __shfl_xor(gx, 32, 64);
        gy += __shfl_xor(gy, 32, 64);
        gz += __shfl_xor(gz, 32, 64);
        if (lane < 32) {
            gp[(wave * 3 + 0) * P + r] = gx;
            gp[(wave * 3 + 1) * P + r] = gy;
            gp[(wave * 3 + 2) * P + r] = gz;
        }
    }
};

}  // namespace sg
