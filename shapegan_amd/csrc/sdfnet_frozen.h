// shapegan_amd/csrc/sdfnet_frozen.h — SDFNet with FROZEN weights on a 32-point tile of one shape, per-shape bias mode: what the latent
// fit (latent_fit.hip, K7c) and the level-set projection (sdfnet_project.hip, K7d) share.  Both run sdfnet_fwd_tile with KEEP, hold the
// seven sign words a lane produces in registers instead of storing them, and walk the chain back through the transposed packs of the
// same weight image, dZ_l = (T_{l+1} dZ_{l+1}) * ReLU'(H_l), in the forward's own [256][P] LDS tile.  They differ in the epilogue of
// the forward (Io::store: what dz8 is) and in what they do with dZ5 and dZ1 (the functor of sdfnet_frozen_bwd_tile).
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

}  // namespace sg
