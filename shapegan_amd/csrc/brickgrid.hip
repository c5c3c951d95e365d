// shapegan_amd/csrc/brickgrid.hip — narrow-band voxel grids: the SDFNet evaluated only in bricks near the surface (K18).
//
// Serves SDFNet.voxel_grids (model/sdf_net.py:77-112: get_voxels / get_mesh evaluate the network at every lattice point).  The
// network itself is sg_sdfnet_fwd; these kernels are the bookkeeping around it, all bandwidth- or latency-bound:
//   points    a brick list (or every brick's 8 corners) -> the point table and per-point shape index of one sg_sdfnet_fwd launch;
//   seed      corner values -> per-brick fill and seed flag, one lane per brick; then the whole grid set to the fills (1 where the
//             mask leaves a point out), one lane per point, lanes along z;
//   compact   flags -> the ascending list of newly active bricks and its count: per-workgroup totals, one workgroup scans them, the
//             flagged bricks take their places.  Positions follow from prefix sums, never from atomics: the list is the same on
//             every run and equals the twin's, which walks the bricks in order;
//   scatter   values of a brick list -> the grid, lanes along z;
//   grow      one workgroup per newly active brick: its points' sides reduce to two 27-bit region masks (which neighbours have an
//             inside / an outside point of this brick within Chebyshev distance 2), then lane d flags neighbour d.  Workgroups only
//             ever store the value 1 into `flag`, so concurrent flagging of one neighbour is the same store twice.
// A round of the continuation is compact, points, sg_sdfnet_fwd, scatter, grow: seven launches and one host read of the count.
#include "common.h"
#include "../../include/shapegan_hip.h"

#include "brickgrid_core.h"      // shared with the twin

namespace sg {

constexpr int kBrickBlock = 256;

struct BrickTables {
    const float *ax, *ay, *az;
};

// i = (position in the list) * ppb + (local point); corners: ppb = 8, local point = corner n
__global__ void __launch_bounds__(kBrickBlock) brick_points_kernel(SgBrickGeom g, const int* __restrict__ bricks, long M, int corners,
                                                                   BrickTables t, float* __restrict__ points,
                                                                   int* __restrict__ shape_index) {
    const long ppb = corners ? 8 : (long)g.B * g.B * g.B;
    const long i = (long)blockIdx.x * kBrickBlock + threadIdx.x;
    if (i >= M * ppb) return;
    const long j = i / ppb;
    const int l = (int)(i - j * ppb);
    long brick = bricks ? (long)bricks[j] : j;
    if (brick < 0 || brick >= g.S * g.nb) brick = 0;      // (a list entry out of range never leaves the tables)
    long s;
    int bx, by, bz, lx, ly, lz;
    sg_brick_decode(g, brick, s, bx, by, bz);
    if (corners) {
        sg_brick_corner_local(g, l, lx, ly, lz);
    } else {
        lx = l >> (2 * g.shift);
        ly = (l >> g.shift) & (g.B - 1);
        lz = l & (g.B - 1);
    }
    points[i * 3] = t.ax[bx * g.B + lx];
    points[i * 3 + 1] = t.ay[by * g.B + ly];
    points[i * 3 + 2] = t.az[bz * g.B + lz];
    shape_index[i] = (int)s;
}

__global__ void __launch_bounds__(kBrickBlock) brick_seed_kernel(SgBrickGeom g, const float* __restrict__ corner_values,
                                                                 const unsigned char* __restrict__ mask, float level, float band, int pad,
                                                                 int* __restrict__ state, float* __restrict__ fill, int* __restrict__ flag) {
    const long brick = (long)blockIdx.x * kBrickBlock + threadIdx.x;
    if (brick >= g.S * g.nb) return;
    long s;
    int bx, by, bz;
    sg_brick_decode(g, brick, s, bx, by, bz);
    float f;
    const bool hit = sg_brick_seed_test(g, corner_values, mask, s, bx, by, bz, level, band, pad, &f);
    fill[brick] = f;
    state[brick] = 0;
    flag[brick] = hit ? 1 : 0;
}

// one lane per lattice point of one shape (blockIdx.y), lanes along z
__global__ void __launch_bounds__(kBrickBlock) brick_fill_kernel(SgBrickGeom g, const unsigned char* __restrict__ mask,
                                                                 const float* __restrict__ fill, float* __restrict__ grid) {
    const long cells = (long)g.R * g.R * g.R;
    const long p = (long)blockIdx.x * kBrickBlock + threadIdx.x;
    if (p >= cells) return;
    const long s = blockIdx.y;
    const int z = (int)(p % g.R), y = (int)((p / g.R) % g.R), x = (int)(p / ((long)g.R * g.R));
    const long brick = s * g.nb + ((long)((x >> g.shift) * g.nbx + (y >> g.shift)) * g.nbx + (z >> g.shift));
    grid[s * cells + p] = (mask && !mask[p]) ? 1.f : fill[brick];
}

__global__ void __launch_bounds__(kBrickBlock) brick_count_kernel(const int* __restrict__ flag, long n, int* __restrict__ block_tot) {
    __shared__ int lds[kBrickBlock / 64];
    const long i = (long)blockIdx.x * kBrickBlock + threadIdx.x;
    int total;
    sg_block_exclusive_256(i < n && flag[i] ? 1 : 0, lds, total);
    if (threadIdx.x == 0) block_tot[blockIdx.x] = total;
}

// one workgroup of 1024: thread i scans a contiguous range of the workgroup totals
__global__ void __launch_bounds__(1024) brick_scan_kernel(const int* __restrict__ block_tot, int* __restrict__ block_off, long n,
                                                          int* __restrict__ count) {
    __shared__ int part[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long per = (n + 1023) / 1024;
    const long i0 = threadIdx.x * per < n ? threadIdx.x * per : n, i1 = i0 + per < n ? i0 + per : n;
    int sum = 0;
    for (long i = i0; i < i1; ++i) sum += block_tot[i];
    int incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(incl, off, 64);
        if (lane >= off) incl += y;
    }
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        before += w < wave ? part[w] : 0;
        all += part[w];
    }
    int run = before + incl - sum;
    for (long i = i0; i < i1; ++i) {
        block_off[i] = run;
        run += block_tot[i];
    }
    if (threadIdx.x == 0) *count = all;
}

// the flagged bricks take their places; states move on (newly active -> active, flagged -> newly active) and the flags are cleared
__global__ void __launch_bounds__(kBrickBlock) brick_emit_kernel(int* __restrict__ state, int* __restrict__ flag, long n,
                                                                 const int* __restrict__ block_off, int* __restrict__ list) {
    __shared__ int lds[kBrickBlock / 64];
    const long i = (long)blockIdx.x * kBrickBlock + threadIdx.x;
    const int f = i < n && flag[i] ? 1 : 0;
    int total;
    const int excl = sg_block_exclusive_256(f, lds, total);
    if (i >= n) return;
    if (f) {
        list[block_off[blockIdx.x] + excl] = (int)i;
        state[i] = 2;
        flag[i] = 0;
    } else if (state[i] == 2) {
        state[i] = 1;
    }
}

__global__ void __launch_bounds__(kBrickBlock) brick_scatter_kernel(SgBrickGeom g, const float* __restrict__ values,
                                                                    const int* __restrict__ bricks, long M,
                                                                    const unsigned char* __restrict__ mask, float* __restrict__ grid) {
    const int ppb = g.B * g.B * g.B;
    const long i = (long)blockIdx.x * kBrickBlock + threadIdx.x;
    if (i >= M * ppb) return;
    const long j = i >> (3 * g.shift);
    const int l = (int)(i & (ppb - 1));
    const long brick = bricks[j];
    if (brick < 0 || brick >= g.S * g.nb) return;
    long s;
    int bx, by, bz;
    sg_brick_decode(g, brick, s, bx, by, bz);
    const long p = sg_brick_lattice(g, bx, by, bz, l >> (2 * g.shift), (l >> g.shift) & (g.B - 1), l & (g.B - 1));
    grid[s * (long)g.R * g.R * g.R + p] = (mask && !mask[p]) ? 1.f : values[i];
}

// one workgroup per newly active brick (64 lanes for B = 4, 256 otherwise)
__global__ void __launch_bounds__(kBrickBlock) brick_grow_kernel(SgBrickGeom g, const int* __restrict__ bricks, const float* __restrict__ grid,
                                                                 const int* __restrict__ state, const float* __restrict__ fill, float level,
                                                                 int* __restrict__ flag) {
    __shared__ unsigned lds[2][kBrickBlock / 64];
    const long brick = bricks[blockIdx.x];
    if (brick < 0 || brick >= g.S * g.nb) return;      // (uniform over the workgroup)
    long s;
    int bx, by, bz;
    sg_brick_decode(g, brick, s, bx, by, bz);
    const float* gs = grid + s * (long)g.R * g.R * g.R;
    const int ppb = g.B * g.B * g.B;
    unsigned in_mask = 0, out_mask = 0;
    for (int l = threadIdx.x; l < ppb; l += blockDim.x) {
        const int lx = l >> (2 * g.shift), ly = (l >> g.shift) & (g.B - 1), lz = l & (g.B - 1);
        const unsigned m = sg_brick_region_mask(g.B, lx, ly, lz);
        if (sg_brick_inside(gs[sg_brick_lattice(g, bx, by, bz, lx, ly, lz)], level))
            in_mask |= m;
        else
            out_mask |= m;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        in_mask |= (unsigned)__shfl_xor((int)in_mask, off, 64);
        out_mask |= (unsigned)__shfl_xor((int)out_mask, off, 64);
    }
    const int waves = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        lds[0][threadIdx.x >> 6] = in_mask;
        lds[1][threadIdx.x >> 6] = out_mask;
    }
    __syncthreads();
    if (threadIdx.x < 27) {
        unsigned im = 0, om = 0;
        for (int w = 0; w < waves; ++w) {
            im |= lds[0][w];
            om |= lds[1][w];
        }
        sg_brick_grow_apply(g, state, fill, flag, brick, threadIdx.x, im, om, level);
    }
}

static unsigned brick_blocks(long n) { return (unsigned)((n + kBrickBlock - 1) / kBrickBlock); }

}  // namespace sg

using namespace sg;

extern "C" {

size_t sg_brick_compact_workspace_bytes(long S, int R, int B) {
    SgBrickGeom g;
    if (!sg_brick_geom(g, S, R, B)) return 0;
    return (size_t)brick_blocks(g.S * g.nb) * 2 * sizeof(int);
}

int sg_brick_points(const int* bricks, long M, int corners, long S, int R, int B, const float* axis_x, const float* axis_y,
                    const float* axis_z, float* points, int* shape_index, hipStream_t stream) {
    SgBrickGeom g;
    SG_CHECK_ARG(sg_brick_geom(g, S, R, B));
    SG_CHECK_ARG(axis_x && axis_y && axis_z && points && shape_index && M > 0 && M <= g.S * g.nb && (corners == 0 || corners == 1));
    SG_CHECK_ARG(bricks || M == g.S * g.nb);
    const long n = M * (corners ? 8 : (long)B * B * B);
    SG_CHECK_ARG(n <= 2147483647L * (long)kBrickBlock);
    const BrickTables t = {axis_x, axis_y, axis_z};
    hipLaunchKernelGGL(brick_points_kernel, dim3(brick_blocks(n)), dim3(kBrickBlock), 0, stream, g, bricks, M, corners, t, points,
                       shape_index);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_brick_seed(const float* corner_values, const unsigned char* mask, long S, int R, int B, float level, float band, int pad,
                  int* state, float* fill, int* flag, float* grid, hipStream_t stream) {
    SgBrickGeom g;
    SG_CHECK_ARG(sg_brick_geom(g, S, R, B));
    SG_CHECK_ARG(corner_values && state && fill && flag && grid && band >= 0.f && (pad == 0 || pad == 1) && S <= 65535);
    hipLaunchKernelGGL(brick_seed_kernel, dim3(brick_blocks(g.S * g.nb)), dim3(kBrickBlock), 0, stream, g, corner_values, mask, level,
                       band, pad, state, fill, flag);
    hipLaunchKernelGGL(brick_fill_kernel, dim3(brick_blocks((long)R * R * R), (unsigned)S), dim3(kBrickBlock), 0, stream, g, mask,
                       (const float*)fill, grid);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_brick_compact(int* state, int* flag, long S, int R, int B, int* list, int* count, void* workspace, size_t workspace_bytes,
                     hipStream_t stream) {
    SgBrickGeom g;
    SG_CHECK_ARG(sg_brick_geom(g, S, R, B));
    SG_CHECK_ARG(state && flag && list && count && workspace);
    if (workspace_bytes < sg_brick_compact_workspace_bytes(S, R, B)) SG_FAIL(SG_ERR_WORKSPACE, "sg_brick_compact: workspace too small");
    const long n = g.S * g.nb;
    const unsigned blocks = brick_blocks(n);
    int* block_tot = (int*)workspace;
    int* block_off = block_tot + blocks;
    hipLaunchKernelGGL(brick_count_kernel, dim3(blocks), dim3(kBrickBlock), 0, stream, (const int*)flag, n, block_tot);
    hipLaunchKernelGGL(brick_scan_kernel, dim3(1), dim3(1024), 0, stream, (const int*)block_tot, block_off, (long)blocks, count);
    hipLaunchKernelGGL(brick_emit_kernel, dim3(blocks), dim3(kBrickBlock), 0, stream, state, flag, n, (const int*)block_off, list);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_brick_scatter(const float* values, const int* bricks, long M, const unsigned char* mask, long S, int R, int B, float* grid,
                     hipStream_t stream) {
    SgBrickGeom g;
    SG_CHECK_ARG(sg_brick_geom(g, S, R, B));
    SG_CHECK_ARG(values && bricks && grid && M > 0 && M <= g.S * g.nb);
    const long n = M * (long)B * B * B;
    hipLaunchKernelGGL(brick_scatter_kernel, dim3(brick_blocks(n)), dim3(kBrickBlock), 0, stream, g, values, bricks, M, mask, grid);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_brick_grow(const int* bricks, long M, const float* grid, const int* state, const float* fill, long S, int R, int B, float level,
                  int* flag, hipStream_t stream) {
    SgBrickGeom g;
    SG_CHECK_ARG(sg_brick_geom(g, S, R, B));
    SG_CHECK_ARG(bricks && grid && state && fill && flag && M > 0 && M <= g.S * g.nb);
    hipLaunchKernelGGL(brick_grow_kernel, dim3((unsigned)M), dim3(B == 4 ? 64 : kBrickBlock), 0, stream, g, bricks, grid, state, fill, level,
                       flag);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

}  // extern "C"
