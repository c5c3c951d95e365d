// shapegan_amd/csrc/sdfnet_project.hip — value, point gradient and Newton steps onto a level set of a frozen SDFNet for a tile of
// points in ONE launch (K7d; serves SDFNet.sdf_and_gradient / project_to_level_set and shapegan_amd/surface.py).
//
// The reference takes its normals and its surface points from autograd with respect to the points (model/sdf_net.py:118-156): one
// forward that keeps every activation, one backward, and a single first-order step that takes |grad f| = 1 for granted.  Composed from
// the training kernels that is 14.8 KB of activation and dZ images per point which only the weight-gradient GEMMs ever read.  With
// frozen weights the chain needs of the forward only ReLU' (latent_fit.hip, K7c), and where K7c sums dZ1 / dZ5 over the points of a
// tile to get d/dz, the point gradient multiplies them by the three point columns of W1 / W5:
//     g[p] = W5[:, 256:259]^T dZ5[:, p] + W1[:, 0:3]^T dZ1[:, p].
// So a workgroup here keeps x, f(x) and grad f(x) of its 32 points on the chip and runs `iterations + 1` rounds of
//   1. the eight layers through sdfnet_fwd_tile (per-shape bias mode, the forward of sg_sdfnet_fwd bit for bit), coordinates read from
//      an LDS xyz[32][3] the tile owns, the seven sign words kept in registers;
//   2. out = tanh(v), dz8 = 1 - out^2, and the chain back through the transposed packs exactly as in latent_fit_kernel;
//   3. the two products above: every lane multiplies the 16 rows of dZ5 (later dZ1) it holds for its point by the matching rows of
//      the point columns — K split over the eight waves, VALU, while the tile still holds the image —, the two half-waves are added
//      and the eight waves' [3][32] partials meet in LDS, summed in wave order;
//   4. on all rounds but the last, the step of project_core.h on xyz.
// Memory traffic: 12 B in and 28 B out per point, whatever the number of rounds.  There is no reduction across points: the k order of a
// point's sums is fixed (q within the lane, half-wave, wave), so its outputs do not depend on the rest of the call or on its place.
#include "common.h"
#include "sdfnet_tile.h"
#include "../../include/shapegan_hip.h"
#pragma clang fp contract(off)
#include "project_core.h"      // shared with the twin

namespace sg {

// 32-point tiles for the reasons of latent_fit.hip: the sign words are 7 VGPRs and the LDS leaves room for three workgroups per CU
constexpr int kProjTile = SG_SDFNET_PROJECT_TILE;

struct ProjectArgs {
    const float* points;      // [*,3]
    const int64_t* seg_off;   // [S+1]
    long S;
    const float* zb1;         // [S][256]
    const float* zb5;
    const float* packed;
    SdfPackLayout lay;
    float level;
    int iterations, rule;
    float max_step;
    const int* tiles;         // [T][2]: shape, first point of the tile within the shape
    float* out_points;        // [*,3] or NULL (iterations == 0)
    float* value;             // [*]
    float* grad;              // [*,3]
};

template <int NT>
struct ProjectIo {
    const lds_float* xyz;     // LDS [P][3]
    lds_float* outs;          // LDS [P]: tanh(v)
    lds_float* dz8s;          // LDS [P]: 1 - out^2 (0 beyond cnt)
    int cnt;
    unsigned* signs;          // registers [7][NT]
    __device__ __forceinline__ float coord(const SdfFwdArgs&, long gp, int c) const { return xyz[gp * 3 + c]; }
    __device__ __forceinline__ bool ragged(const SdfFwdArgs&) const { return false; }
    __device__ __forceinline__ int shape(const SdfFwdArgs&, long) const { return 0; }
    __device__ __forceinline__ void keep(int layer, const unsigned (&mk)[NT]) const {
        // (select chain with constant indices, as in latent_fit.hip: a dynamic index would put the words in scratch)
#pragma unroll
        for (int l = 0; l < 7; ++l)
#pragma unroll
            for (int t = 0; t < NT; ++t) signs[l * NT + t] = layer == l ? mk[t] : signs[l * NT + t];
    }
    __device__ __forceinline__ void store(const SdfFwdArgs&, long gp, float v) const {
        const float o = tanhf(v);
        outs[gp] = o;
        dz8s[gp] = gp < cnt ? 1.f - o * o : 0.f;
    }
};

template <int P>
__global__ void __launch_bounds__(512, 4) sdfnet_project_kernel(ProjectArgs f) {
    constexpr int NT = P / 32;
    static_assert(NT == 1, "one accumulator tile per wave");
    __shared__ float s_xyz[P * 3], s_out[P], s_dz8[P], s_gp[8 * 3 * P];
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kh = lane >> 5, r = lane & 31;
    const long tile = blockIdx.x;
    const int s = f.tiles[2 * tile], i0 = f.tiles[2 * tile + 1];
    long beg = 0, n = 0;
    if (s >= 0 && s < f.S) {
        beg = f.seg_off[s];
        n = f.seg_off[s + 1] - beg;
    }
    long cnt = i0 < 0 ? 0 : n - i0;
    if (cnt > P) cnt = P;
    if (cnt <= 0) return;      // (a table row that names nothing: the whole workgroup leaves and writes nothing)
    const long first = beg + i0;
    // the tile reads all its points before it writes any: out_points may alias points
    for (int e = tid; e < 3 * P; e += 512) s_xyz[e] = e < 3 * cnt ? f.points[first * 3 + e] : 0.f;
    __syncthreads();

    unsigned signs[7 * NT];
    ProjectIo<NT> io;
    io.xyz = (const lds_float*)s_xyz;
    io.outs = (lds_float*)s_out;
    io.dz8s = (lds_float*)s_dz8;
    io.cnt = (int)cnt;
    io.signs = signs;

    SdfFwdArgs a;
    a.points = f.points;
    a.points_period = 0;
    a.latent = nullptr;
    a.latent_idx = nullptr;
    a.L = 0;
    a.lay = f.lay;
    a.pps = 1L << 40;
    a.sid = nullptr;
    a.out = nullptr;
    a.acts = nullptr;
    a.ldn = 0;
    a.N = cnt;
    a.nbig = 0;
    a.eps = 0.f;

    float* const Hs = smem;      // [256][P], as in the forward
    // the forward's bias vectors (7 KB behind H, X and the layer-8 partials) are dead once its last GEMM has started and are staged
    // again by every forward: the backward keeps the point columns of W1 / W5 there, Wx[2][256][3]
    float* const Wx = smem + kH * P + f.lay.KUp * (P + 1) + 16 * P;
    auto rowoff = [](int q) { return (q & 3) + 8 * (q >> 2); };
    // this lane's element (q, t) of the tile: row wave * 32 + frag_row(q, kh), point t * 32 + r
    lds_float* const hw = (lds_float*)Hs + (wave * 32 + 4 * kh) * P + r;
    const lds_float* const wxw = (const lds_float*)Wx + (wave * 32 + 4 * kh) * 3;
    auto noop = []() {};

#pragma unroll 1
    for (int round = 0;; ++round) {
        // (the rounds load the same weights and biases: pointers the compiler cannot see through keep it from hoisting those loads out
        // of the loop, where they would hold some fifty VGPRs across both GEMM chains)
        const float *packed = f.packed, *zb1 = f.zb1 + (long)s * kH, *zb5 = f.zb5 + (long)s * kH;
        asm volatile("" : "+s"(packed), "+s"(zb1), "+s"(zb5));
        a.packed = packed;
        a.zb1 = zb1;      // (shape = p0 / pps = 0: the tile's own bias rows)
        a.zb5 = zb5;
        const float4* pk = reinterpret_cast<const float4*>(packed);
        auto wtile = [&](long off) { return pk + (off >> 2) + (long)wave * (kH / 8) * 64; };
#pragma unroll
        for (int e = 0; e < 7 * NT; ++e) signs[e] = 0u;
        sdfnet_fwd_tile<P, true, false, false, ProjectIo<NT>, true>(a, 0, io);
        // element M(c, k) of a transposed 32-row pack (pack_mfma_a_kernel): ((k >> 3) * 64 + c + 32 (k & 1)) * 4 + ((k >> 1) & 3)
        for (int e = tid; e < 2 * kH * 3; e += 512) {
            const int l = e / (kH * 3), k = (e - l * kH * 3) / 3, c = e % 3;
            Wx[e] = packed[(l ? f.lay.T5i : f.lay.T1) + ((k >> 3) * 64 + c + 32 * (k & 1)) * 4 + ((k >> 1) & 3)];
        }
        __syncthreads();      // out / dz8 of every point and Wx are in LDS, every read of H7 is done

        WRing<4> wr;
        wring_start(wr, wtile(f.lay.T7), lane);
        __builtin_amdgcn_sched_barrier(0);
        // dZ7 = (w8 (x) dz8) * ReLU'(H7)
        {
            const float* w8 = packed + f.lay.W8;
            const float d8 = s_dz8[r];
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float wv = w8[wave * 32 + frag_row(q, kh)];
                hw[rowoff(q) * P] = ((signs[6] >> q) & 1u) ? wv * d8 : 0.f;
            }
        }
        __syncthreads();
        // images 5 .. 0 (dZ6 .. dZ1): GEMM with the transposed pack of the layer above, ReLU' from the kept word, back into the tile
        float gx = 0.f, gy = 0.f, gz = 0.f;      // this lane's 16 rows of W5x^T dZ5 + W1x^T dZ1 for point r
        f32x16 acc[NT];
#pragma unroll 1
        for (int i = 5; i >= 0; --i) {
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[0][q] = 0.f;
            mlp_gemm_ring<NT, 4, kH / 8>(acc, wr, Hs, P, lane, noop);
            if (i > 0) {
                const long nxt = i == 5 ? f.lay.T6 : i == 4 ? f.lay.T5x : i == 3 ? f.lay.T4 : i == 2 ? f.lay.T3 : f.lay.T2;
                wring_start(wr, wtile(nxt), lane);
                __builtin_amdgcn_sched_barrier(0);
            }
            unsigned mk = signs[0];
#pragma unroll
            for (int l = 1; l < 6; ++l) mk = i == l ? signs[l] : mk;
            __syncthreads();      // every wave has read the tile
            const bool cols = i == 4 || i == 0;      // dZ5 and dZ1: the images behind the point gradient
            const lds_float* const wx = wxw + (i == 0 ? 0 : kH * 3);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const float g = ((mk >> q) & 1u) ? acc[0][q] : 0.f;
                if (i > 0) hw[rowoff(q) * P] = g;      // (dZ1 only feeds the point gradient: nothing reads the tile after it)
                if (cols) {
                    const lds_float* w = wx + rowoff(q) * 3;
                    gx = __builtin_fmaf(w[0], g, gx);
                    gy = __builtin_fmaf(w[1], g, gy);
                    gz = __builtin_fmaf(w[2], g, gz);
                }
            }
            if (i > 0) __syncthreads();
        }
        // the two half-waves hold rows 4 kh + {0..3, 8..11, ...} of the same point; then the eight waves in wave order
        gx += __shfl_xor(gx, 32, 64);
        gy += __shfl_xor(gy, 32, 64);
        gz += __shfl_xor(gz, 32, 64);
        if (kh == 0) {
            s_gp[(wave * 3 + 0) * P + r] = gx;
            s_gp[(wave * 3 + 1) * P + r] = gy;
            s_gp[(wave * 3 + 2) * P + r] = gz;
        }
        __syncthreads();
        const bool last = round == f.iterations;
        if (tid < P) {
            float g[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v = s_gp[c * P + tid];
#pragma unroll
                for (int w = 1; w < 8; ++w) v += s_gp[(w * 3 + c) * P + tid];
                g[c] = v;
            }
            if (!last) {
                float x[3] = {s_xyz[tid * 3], s_xyz[tid * 3 + 1], s_xyz[tid * 3 + 2]};
                sg_project_step(x, s_out[tid], g, f.level, f.rule, f.max_step);
                s_xyz[tid * 3] = x[0];
                s_xyz[tid * 3 + 1] = x[1];
                s_xyz[tid * 3 + 2] = x[2];
            } else if (tid < cnt) {
                const long gp = first + tid;
                if (f.out_points) {
                    f.out_points[gp * 3] = s_xyz[tid * 3];
                    f.out_points[gp * 3 + 1] = s_xyz[tid * 3 + 1];
                    f.out_points[gp * 3 + 2] = s_xyz[tid * 3 + 2];
                }
                f.value[gp] = s_out[tid];
                f.grad[gp * 3] = g[0];
                f.grad[gp * 3 + 1] = g[1];
                f.grad[gp * 3 + 2] = g[2];
            }
        }
        if (last) break;
        __syncthreads();      // the next forward stages the moved points
    }
}

// the forward's dynamic LDS (sdfnet.hip fwd_lds_bytes): H [256][P], X [KUp][P + 1], the layer-8 partials [16][P], the biases [7][256]
static size_t project_lds_bytes(int P, int KUp) { return ((size_t)kH * P + (size_t)KUp * (P + 1) + 16 * P + 7 * kH) * sizeof(float); }
static_assert(2 * kH * 3 <= 7 * kH, "the point columns fit where the forward keeps its biases");

}  // namespace sg

using namespace sg;

extern "C" {

int sg_sdfnet_project(const float* points, const int64_t* seg_off, long nshapes, const float* zb1, const float* zb5,
                      const float* packed, float level, int iterations, int rule, float max_step, const int* tiles, long ntiles,
                      float* out_points, float* value, float* grad, hipStream_t stream) {
    SG_CHECK_ARG(points && seg_off && zb1 && zb5 && packed && tiles && value && grad);
    SG_CHECK_ARG(nshapes >= 1 && ntiles >= 1 && ntiles < (1L << 31));
    SG_CHECK_ARG(iterations >= 0 && iterations <= 64 && (rule == SG_PROJECT_RULE_NEWTON || rule == SG_PROJECT_RULE_UNIT));
    SG_CHECK_ARG(max_step >= 0.f && (out_points || iterations == 0));
    ProjectArgs f;
    f.points = points;
    f.seg_off = seg_off;
    f.S = nshapes;
    f.zb1 = zb1;
    f.zb5 = zb5;
    f.packed = packed;
    f.lay = make_layout(3);
    f.level = level;
    f.iterations = iterations;
    f.rule = rule;
    f.max_step = max_step;
    f.tiles = tiles;
    f.out_points = out_points;
    f.value = value;
    f.grad = grad;
    const size_t lds = project_lds_bytes(kProjTile, f.lay.KUp);
    static SgPerDeviceOnce once;
    if (once.begin()) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sdfnet_project_kernel<kProjTile>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        once.end();
        if (e != hipSuccess) SG_FAIL(SG_ERR_HIP, "sg_sdfnet_project: cannot reserve %zu B LDS", lds);
    }
    hipLaunchKernelGGL((sdfnet_project_kernel<kProjTile>), dim3((unsigned)ntiles), dim3(512), lds, stream, f);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

}  // extern "C"
