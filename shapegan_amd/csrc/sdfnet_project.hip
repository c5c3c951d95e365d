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
//   2. out = tanh(v), dz8 = 1 - out^2, and the chain back through the transposed packs: sdfnet_frozen_bwd_tile (sdfnet_frozen.h), the
//      one K7c runs — that header also has the sign keeping, the table row and the forward's arguments;
//   3. the two products above (SdfPointGrad in the same header, shared with the pose fit of latent_fit.hip): every lane multiplies the
//      16 rows of dZ5 (later dZ1) it holds for its point by the matching rows of the point columns, the two half-waves are added and
//      the eight waves' [3][32] partials meet in LDS, summed in wave order;
//   4. on all rounds but the last, the step of project_core.h on xyz.
// Memory traffic: 12 B in and 28 B out per point, whatever the number of rounds.  There is no reduction across points: the k order of a
// point's sums is fixed (q within the lane, half-wave, wave), so its outputs do not depend on the rest of the call or on its place.
#include "common.h"
#include "sdfnet_frozen.h"
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

struct ProjectIo : SdfSignKeeper {
    const lds_float* xyz;     // LDS [P][3]
    lds_float* outs;          // LDS [P]: tanh(v)
    lds_float* dz8s;          // LDS [P]: 1 - out^2 (0 beyond cnt)
    int cnt;
    __device__ __forceinline__ float coord(const SdfFwdArgs&, long gp, int c) const { return xyz[gp * 3 + c]; }
    __device__ __forceinline__ void store(const SdfFwdArgs&, long gp, float v) const {
        const float o = tanhf(v);
        outs[gp] = o;
        dz8s[gp] = gp < cnt ? 1.f - o * o : 0.f;
    }
};

template <int P>
__global__ void __launch_bounds__(512, 4) sdfnet_project_kernel(ProjectArgs f) {
    __shared__ float s_xyz[P * 3], s_out[P], s_dz8[P], s_gp[8 * 3 * P];
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x;
    const SdfTileRow row = sdf_tile_row(f.tiles, f.seg_off, f.S, blockIdx.x);
    const int s = row.s;
    long cnt = row.i0 < 0 ? 0 : row.n - row.i0;
    if (cnt > P) cnt = P;
    if (cnt <= 0) return;      // (a table row that names nothing: the whole workgroup leaves and writes nothing)
    const long first = row.beg + row.i0;
    // the tile reads all its points before it writes any: out_points may alias points
    for (int e = tid; e < 3 * P; e += 512) s_xyz[e] = e < 3 * cnt ? f.points[first * 3 + e] : 0.f;
    __syncthreads();

    unsigned signs[7];
    ProjectIo io;
    io.signs = signs;
    io.xyz = (const lds_float*)s_xyz;
    io.outs = (lds_float*)s_out;
    io.dz8s = (lds_float*)s_dz8;
    io.cnt = (int)cnt;

    // (packed / zb1 / zb5 are set by every round, below)
    SdfFwdArgs a = sdf_frozen_tile_args(f.points, nullptr, f.lay, nullptr, nullptr, cnt);

#pragma unroll 1
    for (int round = 0;; ++round) {
        // (the rounds load the same weights and biases: pointers the compiler cannot see through keep it from hoisting those loads out
        // of the loop, where they would hold some fifty VGPRs across both GEMM chains)
        const float *packed = f.packed, *zb1 = f.zb1 + (long)s * kH, *zb5 = f.zb5 + (long)s * kH;
        asm volatile("" : "+s"(packed), "+s"(zb1), "+s"(zb5));
        a.packed = packed;
        a.zb1 = zb1;      // (shape = p0 / pps = 0: the tile's own bias rows)
        a.zb5 = zb5;
#pragma unroll
        for (int e = 0; e < 7; ++e) signs[e] = 0u;
        sdfnet_fwd_tile<P, true, false, false, ProjectIo, true>(a, 0, io);
        SdfPointGrad<P> pg(smem, f.lay);
        pg.stage(packed, f.lay);      // (through this round's opaque pointer)
        __syncthreads();      // out / dz8 of every point and Wx are in LDS, every read of H7 is done

        // the chain back and the point gradient (sdfnet_frozen.h); dZ5 and dZ1 are the images behind it
        sdfnet_frozen_bwd_tile<P>(packed, f.lay, smem, signs[0], signs[1], signs[2], signs[3], signs[4], signs[5], signs[6], s_dz8,
                                  [&](int i, int q, float g) __attribute__((always_inline)) {
                                      if (i == 4 || i == 0) pg.add(i, q, g);
                                  });
        pg.partials(s_gp);      // the two half-waves; then the eight waves in wave order
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
    const size_t lds = sdf_fwd_lds_bytes(kProjTile, f.lay.KUp);
    static SgPerDeviceOnce once;
    if (const int rc = sg_reserve_lds(once, sdfnet_project_kernel<kProjTile>, lds, "sg_sdfnet_project")) return rc;
    hipLaunchKernelGGL((sdfnet_project_kernel<kProjTile>), dim3((unsigned)ntiles), dim3(512), lds, stream, f);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

}  // extern "C"
