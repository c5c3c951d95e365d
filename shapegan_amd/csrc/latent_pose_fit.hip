// shapegan_amd/csrc/latent_pose_fit.hip — fitting the pose of a cloud together with its latent code: forward, loss, the latent-only
// backward AND the gradient with respect to an affine map of the observed points, for a tile of points in ONE launch (K7e; serves
// shapegan_amd/reconstruct.py fit_codes_and_poses and SDFNet.latent_pose_loss_and_grad).
//
// A scan does not arrive in the network's canonical frame: a partial cloud's bounding sphere is not the object's and a sensor's cloud
// is not upright.  An auto-decoder has no other model of where the shape should be than the network itself, so the pose is optimised
// through it: observed q, canonical x = A q + t, target' = clamp(ts target, +-cutoff) (a similarity scales distances by ts = s), and
//     loss = mean_p |SDFNet(A q_p + t, z) - target'_p|.
// d loss / dz is K7c's (latent_fit.hip) at the posed points.  d loss / d(A|t) is K7d's point gradient (sdfnet_project.hip)
//     g[p] = W5[:, 256:259]^T dZ5[:, p] + W1[:, 0:3]^T dZ1[:, p]
// of K7c's loss, contracted with the observed coordinates: dA = sum_p g[p] (x) q[p], dt = sum_p g[p]; and d loss / d ts = sum_p e[p],
// e = -sign(d) target / m inside the clamp.  So a workgroup here
//   1. stages its tile's q in LDS and forms x there (the order of the header: three nested fmas per coordinate);
//   2. runs K7c's forward and epilogue at x (the coordinates read from LDS as K7d's Io does), which also leaves e per point;
//   3. walks the chain back (sdfnet_frozen_bwd_tile) with a functor that does K7c's half-wave row sums of dZ1 / dZ5 and K7d's three fmas
//      against the point columns, then K7d's cross-half exchange and [8][3][32] partials through LDS;
//   4. reduces g (x) q, g and e over the tile's points in point order.  g itself never goes to memory.
// 16 B in per point, 2.1 KB out per TILE.  Tiles never straddle shapes, a lane beyond the tile's count contributes exact zeros (its
// dz8, hence its g, and its e are 0; its q is staged as 0), and every sum has a fixed order: a shape's rows do not depend on what
// else is in the call.  With the identity pose and ts = 1, x == q and target' == clamp(target) bit for bit, so floats [0, 513) of a
// row are K7c's.
#include "common.h"
#include "sdfnet_frozen.h"
#include "../../include/shapegan_hip.h"

namespace sg {

// 32-point tiles for the reasons of latent_fit.hip
constexpr int kPoseTile = SG_SDFNET_LATENT_TILE;
constexpr int kPoseRow = SG_SDFNET_POSE_PARTIAL_ROW;
constexpr int kPoseSums = 13;      // 9 of g (x) q, 3 of g, 1 of e
static_assert(kPoseRow >= 2 * kH + 1 + kPoseSums && kPoseRow == SG_SDFNET_LATENT_PARTIAL_ROW + 15, "partial row");

struct LatentPoseArgs {
    const float* points;      // [*,3] observed
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
    const float* pose;        // [S][16]
    float* part;              // [T][kPoseRow]
};

struct LatentPoseIo : SdfSignKeeper {
    const float* target;
    long beg, n, first;       // the shape's run and (win_start + i0) mod n
    int cnt;                  // used points of this tile
    float inv_den;            // divisor m as a float
    float cutoff, ts;
    const lds_float* xyz;     // LDS [P][3]: the posed points
    float* dz8s;              // LDS [P]
    float* absd;              // LDS [P]
    float* es;                // LDS [P]
    __device__ __forceinline__ long index(long gp) const {
        const long i = first + gp;      // (gp < cnt <= n and first < n: one wrap at most)
        return beg + (i >= n ? i - n : i);
    }
    __device__ __forceinline__ float coord(const SdfFwdArgs&, long gp, int c) const { return xyz[gp * 3 + c]; }
    __device__ __forceinline__ void store(const SdfFwdArgs&, long gp, float v) const {
        float dz = 0.f, ad = 0.f, e = 0.f;
        if (gp < cnt) {
            const float o = tanhf(v);
            const float c = cutoff;
            const float raw = target[index(gp)];
            const float st = ts * raw;
            const float t = fminf(fmaxf(st, -c), c);
            const float d = o - t;
            ad = fabsf(d);
            const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
            dz = sg * ((1.f - o * o) / inv_den);
            if (st > -c && st < c) e = (-sg * raw) / inv_den;
        }
        dz8s[gp] = dz;
        absd[gp] = ad;
        es[gp] = e;
    }
};

template <int P>
__global__ void __launch_bounds__(512, 4) latent_pose_fit_kernel(LatentPoseArgs f) {
    __shared__ float s_q[P * 3], s_xyz[P * 3], s_dz8[P], s_abs[P], s_e[P], s_gp[8 * 3 * P], s_g[3 * P];
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kh = lane >> 5, r = lane & 31;
    const long tile = blockIdx.x;
    const SdfTileRow row = sdf_tile_row(f.tiles, f.seg_off, f.S, tile);
    const long n = row.n;
    float* const prow = f.part + tile * kPoseRow;
    const long m = n <= 0 ? 0 : (f.win_count <= 0 || f.win_count > n ? n : f.win_count);
    long cnt = row.i0 < 0 ? 0 : m - row.i0;
    if (cnt > P) cnt = P;
    if (cnt <= 0) {       // (a table row that names nothing: the whole workgroup leaves, its partial row is zero)
        for (int e = tid; e < kPoseRow; e += 512) prow[e] = 0.f;
        return;
    }
    unsigned signs[7];
#pragma unroll
    for (int e = 0; e < 7; ++e) signs[e] = 0u;
    const float* const ps = f.pose + (long)row.s * 16;
    LatentPoseIo io;
    io.signs = signs;
    io.target = f.target;
    io.beg = row.beg;
    io.n = n;
    io.first = (f.win_start + row.i0) % n;
    io.cnt = (int)cnt;
    io.inv_den = (float)m;
    io.cutoff = f.cutoff;
    io.ts = ps[12];
    io.xyz = (const lds_float*)s_xyz;
    io.dz8s = s_dz8;
    io.absd = s_abs;
    io.es = s_e;

    // the tile's observed points (0 beyond cnt), then x_c = fma(A_c0, qx, fma(A_c1, qy, fma(A_c2, qz, t_c)))
    for (int e = tid; e < 3 * P; e += 512) {
        const int p = e / 3, c = e - 3 * p;
        s_q[e] = p < cnt ? f.points[io.index(p) * 3 + c] : 0.f;
    }
    __syncthreads();
    if (tid < 3 * P) {
        const int p = tid / 3, c = tid - 3 * p;
        const float* a = ps + 4 * c;
        s_xyz[tid] = __builtin_fmaf(a[0], s_q[p * 3], __builtin_fmaf(a[1], s_q[p * 3 + 1], __builtin_fmaf(a[2], s_q[p * 3 + 2], a[3])));
    }
    __syncthreads();

    const SdfFwdArgs a = sdf_frozen_tile_args(f.points, f.packed, f.lay, f.zb1 + (long)row.s * kH, f.zb5 + (long)row.s * kH, cnt);
    sdfnet_fwd_tile<P, true, false, false, LatentPoseIo, true>(a, 0, io);
    // the forward's bias vectors (7 KB behind H, X and the layer-8 partials) are dead once its last GEMM has started: the backward keeps
    // the point columns of W1 / W5 there, Wx[2][256][3], as K7d does
    float* const Wx = smem + kH * P + f.lay.KUp * (P + 1) + 16 * P;
    const lds_float* const wxw = (const lds_float*)Wx + (wave * 32 + 4 * kh) * 3;
    // element M(c, k) of a transposed 32-row pack (pack_mfma_a_kernel): ((k >> 3) * 64 + c + 32 (k & 1)) * 4 + ((k >> 1) & 3)
    for (int e = tid; e < 2 * kH * 3; e += 512) {
        const int l = e / (kH * 3), k = (e - l * kH * 3) / 3, c = e % 3;
        Wx[e] = f.packed[(l ? f.lay.T5i : f.lay.T1) + ((k >> 3) * 64 + c + 32 * (k & 1)) * 4 + ((k >> 1) & 3)];
    }
    __syncthreads();      // dz8 / |d| / e of every point and Wx are in LDS, every read of H7 is done

    // the tile's sums of |d| and of e in point order (points beyond cnt hold 0)
    if (tid == 0) {
        float l = 0.f;
#pragma unroll 8
        for (int p = 0; p < P; ++p) l += s_abs[p];
        prow[2 * kH] = l;
    } else if (tid == 64) {
        float l = 0.f;
#pragma unroll 8
        for (int p = 0; p < P; ++p) l += s_e[p];
        prow[2 * kH + 1 + 12] = l;
        prow[2 * kH + 1 + 13] = 0.f;
        prow[2 * kH + 1 + 14] = 0.f;
    }

    // dZ5 and dZ1: their row sums over the tile's points (K7c) and their products with the point columns (K7d)
    float gx = 0.f, gy = 0.f, gz = 0.f;      // this lane's 16 rows of W5x^T dZ5 + W1x^T dZ1 for point r
    sdfnet_frozen_bwd_tile<P>(f.packed, f.lay, smem, signs[0], signs[1], signs[2], signs[3], signs[4], signs[5], signs[6], s_dz8,
                              [&](int i, int q, float g) __attribute__((always_inline)) {
                                  if (i == 4 || i == 0) {
                                      const float rsum = half_wave_sum(g);
                                      if (r == 31) prow[(i == 0 ? 0 : kH) + wave * 32 + 4 * kh + frag_rowoff(q)] = rsum;
                                      const lds_float* w = wxw + (i == 0 ? 0 : kH * 3) + frag_rowoff(q) * 3;
                                      gx = __builtin_fmaf(w[0], g, gx);
                                      gy = __builtin_fmaf(w[1], g, gy);
                                      gz = __builtin_fmaf(w[2], g, gz);
                                  }
                              });
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
    if (tid < 3 * P) {      // g_c of point p = tid % P, c = tid / P
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

// per shape: t1 / t5 and loss as latent_reduce_kernel (latent_fit.hip) from the longer rows, and gpose [S][16] = the sums of its tiles'
// pose sums, tiles added in tile order (double).  Threads [512, 525) own the thirteen live floats of gpose.
__global__ void __launch_bounds__(576) latent_pose_reduce_kernel(const float* __restrict__ part, const int64_t* __restrict__ tile_off,
                                                                 const int64_t* __restrict__ seg_off, long S, long win_count,
                                                                 float* __restrict__ t1, float* __restrict__ t5,
                                                                 float* __restrict__ loss, float* __restrict__ gpose) {
    __shared__ double red[64];
    const long s = blockIdx.x;
    const int tid = threadIdx.x;
    const long ta = tile_off[s], tb = tile_off[s + 1];
    const bool live = tid < 2 * kH + kPoseSums;
    // float k of gpose is in pose's layout, rows of A_c0 A_c1 A_c2 t_c: from sum g_c q_j (513 + 3 c + j), sum g_c (522 + c), sum e (525)
    const int k = tid - 2 * kH;
    const int col = tid < 2 * kH ? tid : !live ? 0 : k == 12 ? 2 * kH + 13 : (k & 3) == 3 ? 2 * kH + 10 + (k >> 2) : 2 * kH + 1 + 3 * (k >> 2) + (k & 3);
    const float* src = part + col;
    double acc = 0;
    long t = ta;
    for (; t + 8 <= tb; t += 8) {      // eight loads in flight, added in tile order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[(t + u) * kPoseRow];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; t < tb; ++t) acc += src[t * kPoseRow];
    if (tid < 2 * kH)
        (tid < kH ? t1 : t5)[(long)(tid & (kH - 1)) * S + s] = (float)acc;
    else if (tid < 2 * kH + 16)
        gpose[s * 16 + (tid - 2 * kH)] = live ? (float)acc : 0.f;
    if (tid < 64) {
        double l = 0;
        for (long u = ta + tid; u < tb; u += 64) l += part[u * kPoseRow + 2 * kH];
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

static_assert(2 * kH * 3 <= 7 * kH, "the point columns fit where the forward keeps its biases");

}  // namespace sg

using namespace sg;

extern "C" {

int sg_sdfnet_latent_pose_grad(const float* points, const float* target, const int64_t* seg_off, long nshapes, const float* zb1,
                               const float* zb5, const float* packed, const float* pose, float cutoff, long win_start,
                               long win_count, const int* tiles, long ntiles, float* partials, hipStream_t stream) {
    SG_CHECK_ARG(points && target && seg_off && zb1 && zb5 && packed && pose && tiles && partials);
    SG_CHECK_ARG(nshapes >= 1 && win_start >= 0 && ntiles >= 1 && ntiles < (1L << 31) && cutoff >= 0.f);
    LatentPoseArgs f;
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
    const size_t lds = sdf_fwd_lds_bytes(kPoseTile, f.lay.KUp);
    static SgPerDeviceOnce once;
    if (const int rc = sg_reserve_lds(once, latent_pose_fit_kernel<kPoseTile>, lds, "sg_sdfnet_latent_pose_grad")) return rc;
    hipLaunchKernelGGL((latent_pose_fit_kernel<kPoseTile>), dim3((unsigned)ntiles), dim3(512), lds, stream, f);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_sdfnet_latent_pose_reduce(const float* partials, const int64_t* tile_off, const int64_t* seg_off, long nshapes,
                                 long win_count, float* t1, float* t5, float* loss, float* gpose, hipStream_t stream) {
    SG_CHECK_ARG(partials && tile_off && seg_off && t1 && t5 && loss && gpose && nshapes >= 1 && nshapes < (1L << 31));
    hipLaunchKernelGGL(latent_pose_reduce_kernel, dim3((unsigned)nshapes), dim3(576), 0, stream, partials, tile_off, seg_off, nshapes,
                       win_count, t1, t5, loss, gpose);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

}  // extern "C"
