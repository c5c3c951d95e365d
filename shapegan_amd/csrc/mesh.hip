// shapegan_amd/csrc/mesh.hip — batched marching cubes and area-weighted surface sampling (K12).
//
// Replaces the CPU meshing of model/sdf_net.py:97-116 (skimage.measure.marching_cubes_lewiner + trimesh.Trimesh(...).sample) and
// of metrics.py:31-46, one shape at a time in the reference, with four launches for a whole batch of grids:
//   count     one lane per cell (lanes along the fastest axis, so the corner loads coalesce): the vertices the cell owns (the
//             crossing edges at its minimum corner, axes 0, 1, 2) and the triangles of its case; per-workgroup totals;
//   scan      one workgroup: exclusive offsets of the workgroup totals, per-shape vertex / triangle offsets [S+1];
//   vertices  the classification again, in-workgroup exclusive scan + the workgroup offset: every owned crossing edge's vertex and
//             normal, and the cell's entry of the vertex-offset image (first vertex * 8 | mask of its crossing edges);
//   triangles the case again: each triangle edge names the cell that owns it, whose image entry gives the vertex index.
// Every output position follows from counts and prefix sums, never from atomics, so the result is the same bit for bit on every
// run and equals the order the CPU twin (csrc_cpu/shapegan_cpu.cpp) produces by walking the cells in row-major order.
//
// The "cells" walked are the corners of the (virtually padded) grid, P0 x P1 x P2: corner (a, b, c) owns the edges toward +1 along
// each axis that exist and, when a + 1 < P0, b + 1 < P1 and c + 1 < P2, the cube with that minimum corner.  With padding the last
// corner layer owns nothing (its edges run between two pad values), so the order is the row-major order of the padded cells.
#include "common.h"
#include "mc_tables.h"
#include "../../include/shapegan_hip.h"

// positions and normals are compared with the twin: no contraction of a * b + c into one rounding
#pragma clang fp contract(off)

namespace sg {

constexpr int kMcBlock = 256;
constexpr long kMcIndexLimit = 2147483647L;   // int32 indices: S * cells * kMcSlots must stay below
constexpr int kMcSlots = 24;                  // image entries are vertex * 8 | mask with up to 3 vertices per cell

struct McArgs {
    const float* grids;
    long S;
    int R0, R1, R2;
    int P0, P1, P2;   // corner counts of the padded grid
    int pad;
    float pad_value, level;
    long cells;       // P0 * P1 * P2 per shape
    int blocks;       // workgroups per shape
};

__device__ __forceinline__ float mc_value(const McArgs& m, const float* g, int a, int b, int c) {
    if (m.pad) {
        a -= 1;
        b -= 1;
        c -= 1;
        if ((unsigned)a >= (unsigned)m.R0 || (unsigned)b >= (unsigned)m.R1 || (unsigned)c >= (unsigned)m.R2) return m.pad_value;
    }
    return g[((long)a * m.R1 + b) * m.R2 + c];
}

// corner n of the cell at (a, b, c): offset ((n >> 2) & 1, (n >> 1) & 1, n & 1); corners outside the grid read as pad_value
// (they belong only to edges and cubes that do not exist, whose results are discarded)
__device__ __forceinline__ void mc_corners(const McArgs& m, const float* g, int a, int b, int c, float v[8]) {
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        const int x = a + ((n >> 2) & 1), y = b + ((n >> 1) & 1), z = c + (n & 1);
        v[n] = (x < m.P0 && y < m.P1 && z < m.P2) ? mc_value(m, g, x, y, z) : m.pad_value;
    }
}

struct McCell {
    int mask;   // bit k: the edge along axis k owned by this cell crosses the level
    int nv, nt;
    int cube;   // case index, -1 when the cell has no cube
};

__device__ __forceinline__ McCell mc_classify(const McArgs& m, const float v[8], int a, int b, int c) {
    McCell r;
    int cs = 0;
#pragma unroll
    for (int n = 0; n < 8; ++n) cs |= (v[n] < m.level ? 1 : 0) << n;
    const int in0 = cs & 1;
    r.mask = 0;
    if (a + 1 < m.P0 && in0 != ((cs >> 4) & 1)) r.mask |= 1;
    if (b + 1 < m.P1 && in0 != ((cs >> 2) & 1)) r.mask |= 2;
    if (c + 1 < m.P2 && in0 != ((cs >> 1) & 1)) r.mask |= 4;
    r.nv = __builtin_popcount(r.mask);
    const bool has_cube = a + 1 < m.P0 && b + 1 < m.P1 && c + 1 < m.P2;
    r.cube = has_cube ? cs : -1;
    r.nt = has_cube ? (int)sg_mc_tri_count[cs] : 0;
    return r;
}

__device__ __forceinline__ void mc_decode(const McArgs& m, long cell, int& a, int& b, int& c) {
    const long plane = (long)m.P1 * m.P2;
    a = (int)(cell / plane);
    const long r = cell - (long)a * plane;
    b = (int)(r / m.P2);
    c = (int)(r - (long)b * m.P2);
}

// exclusive scan of one int per thread over the 256-thread workgroup (wave64 shuffles, then the 4 wave totals through LDS)
__device__ __forceinline__ int mc_block_exclusive(int x, int* lds_waves, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = x;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_up(incl, off, 64);
        if (lane >= off) incl += y;
    }
    if (lane == 63) lds_waves[wave] = incl;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kMcBlock / 64; ++w) {
        const int t = lds_waves[w];
        before += w < wave ? t : 0;
        total += t;
    }
    __syncthreads();
    return before + incl - x;
}

__global__ void __launch_bounds__(kMcBlock) mc_count_kernel(McArgs m, int* __restrict__ block_tot) {
    __shared__ int lds[2][kMcBlock / 64];
    const long s = blockIdx.y;
    const long cell = (long)blockIdx.x * kMcBlock + threadIdx.x;
    const float* g = m.grids + s * (long)m.R0 * m.R1 * m.R2;
    int nv = 0, nt = 0;
    if (cell < m.cells) {
        int a, b, c;
        mc_decode(m, cell, a, b, c);
        float v[8];
        mc_corners(m, g, a, b, c, v);
        const McCell r = mc_classify(m, v, a, b, c);
        nv = r.nv;
        nt = r.nt;
    }
    int tv, tt;
    mc_block_exclusive(nv, lds[0], tv);
    mc_block_exclusive(nt, lds[1], tt);
    if (threadIdx.x == 0) {
        block_tot[2 * (s * m.blocks + blockIdx.x)] = tv;
        block_tot[2 * (s * m.blocks + blockIdx.x) + 1] = tt;
    }
}

// one workgroup of 1024: thread i scans a contiguous range of the S * blocks (vertex, triangle) totals
__global__ void __launch_bounds__(1024) mc_scan_kernel(const int* __restrict__ block_tot, int* __restrict__ block_off, long n,
                                                       int blocks, long S, int64_t* __restrict__ vert_offsets,
                                                       int64_t* __restrict__ tri_offsets) {
    __shared__ int part[2][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long per = (n + 1023) / 1024;
    const long i0 = threadIdx.x * per, i1 = i0 + per < n ? i0 + per : n;
    int sv = 0, st = 0;
    for (long i = i0; i < i1; ++i) {
        sv += block_tot[2 * i];
        st += block_tot[2 * i + 1];
    }
    int iv = sv, it = st;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int yv = __shfl_up(iv, off, 64), yt = __shfl_up(it, off, 64);
        if (lane >= off) {
            iv += yv;
            it += yt;
        }
    }
    if (lane == 63) {
        part[0][wave] = iv;
        part[1][wave] = it;
    }
    __syncthreads();
    int bv = 0, bt = 0, allv = 0, allt = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        bv += w < wave ? part[0][w] : 0;
        bt += w < wave ? part[1][w] : 0;
        allv += part[0][w];
        allt += part[1][w];
    }
    int rv = bv + iv - sv, rt = bt + it - st;
    for (long i = i0; i < i1; ++i) {
        block_off[2 * i] = rv;
        block_off[2 * i + 1] = rt;
        if (i % blocks == 0) {
            vert_offsets[i / blocks] = rv;
            tri_offsets[i / blocks] = rt;
        }
        rv += block_tot[2 * i];
        rt += block_tot[2 * i + 1];
    }
    if (threadIdx.x == 0) {
        vert_offsets[S] = allv;
        tri_offsets[S] = allt;
    }
}

// gradient of the padded grid at corner (a, b, c) along `axis`: central difference inside, one-sided at the outermost layer
__device__ __forceinline__ float mc_grad(const McArgs& m, const float* g, int a, int b, int c, int axis, float spacing) {
    int p = axis == 0 ? a : axis == 1 ? b : c;
    const int P = axis == 0 ? m.P0 : axis == 1 ? m.P1 : m.P2;
    const int lo = p > 0 ? p - 1 : p, hi = p < P - 1 ? p + 1 : p;
    if (hi == lo) return 0.f;
    float vl, vh;
    if (axis == 0) {
        vl = mc_value(m, g, lo, b, c);
        vh = mc_value(m, g, hi, b, c);
    } else if (axis == 1) {
        vl = mc_value(m, g, a, lo, c);
        vh = mc_value(m, g, a, hi, c);
    } else {
        vl = mc_value(m, g, a, b, lo);
        vh = mc_value(m, g, a, b, hi);
    }
    return (vh - vl) / ((float)(hi - lo) * spacing);
}

struct McGeom {
    float sp[3], org[3];
};

__global__ void __launch_bounds__(kMcBlock) mc_vertices_kernel(McArgs m, McGeom geo, const int* __restrict__ block_off,
                                                               int* __restrict__ image, float* __restrict__ vertices,
                                                               float* __restrict__ normals, long max_verts) {
    __shared__ int lds[kMcBlock / 64];
    const long s = blockIdx.y;
    const long cell = (long)blockIdx.x * kMcBlock + threadIdx.x;
    const float* g = m.grids + s * (long)m.R0 * m.R1 * m.R2;
    int a = 0, b = 0, c = 0;
    float v[8];
    McCell r;
    r.nv = 0;
    r.mask = 0;
    if (cell < m.cells) {
        mc_decode(m, cell, a, b, c);
        mc_corners(m, g, a, b, c, v);
        r = mc_classify(m, v, a, b, c);
    }
    int total;
    const int excl = mc_block_exclusive(r.nv, lds, total);
    if (cell >= m.cells) return;
    const long base = (long)block_off[2 * (s * m.blocks + blockIdx.x)] + excl;
    image[s * m.cells + cell] = (int)(base * 8 + r.mask);
    if (!r.mask) return;
    const int idx[3] = {a, b, c};
    float g0[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) g0[k] = mc_grad(m, g, a, b, c, k, geo.sp[k]);
    long out = base;
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
        if (!((r.mask >> axis) & 1)) continue;
        const float va = v[0], vb = v[axis == 0 ? 4 : axis == 1 ? 2 : 1];
        const float t = (m.level - va) / (vb - va);
        const int a1 = a + (axis == 0), b1 = b + (axis == 1), c1 = c + (axis == 2);
        float n[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float g1 = mc_grad(m, g, a1, b1, c1, k, geo.sp[k]);
            n[k] = g0[k] + t * (g1 - g0[k]);
        }
        const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        if (out < max_verts) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float pos = ((float)idx[k] + (k == axis ? t : 0.f)) * geo.sp[k] + geo.org[k];
                vertices[out * 3 + k] = pos;
                normals[out * 3 + k] = len > 0.f ? n[k] / len : 0.f;
            }
        }
        ++out;
    }
}

__global__ void __launch_bounds__(kMcBlock) mc_triangles_kernel(McArgs m, const int* __restrict__ block_off,
                                                                const int* __restrict__ image,
                                                                const int64_t* __restrict__ vert_offsets,
                                                                int64_t* __restrict__ faces, long max_tris) {
    __shared__ int lds[kMcBlock / 64];
    const long s = blockIdx.y;
    const long cell = (long)blockIdx.x * kMcBlock + threadIdx.x;
    const float* g = m.grids + s * (long)m.R0 * m.R1 * m.R2;
    int a = 0, b = 0, c = 0;
    McCell r;
    r.nt = 0;
    r.cube = -1;
    if (cell < m.cells) {
        mc_decode(m, cell, a, b, c);
        float v[8];
        mc_corners(m, g, a, b, c, v);
        r = mc_classify(m, v, a, b, c);
    }
    int total;
    const int excl = mc_block_exclusive(r.nt, lds, total);
    if (cell >= m.cells || r.nt == 0) return;
    const long tbase = (long)block_off[2 * (s * m.blocks + blockIdx.x) + 1] + excl;
    const long vshape = vert_offsets[s];
    const int* img = image + s * m.cells;
    const long plane = (long)m.P1 * m.P2;
    for (int j = 0; j < r.nt; ++j) {
        if (tbase + j >= max_tris) break;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int e = sg_mc_tri_edges[r.cube][3 * j + k];
            const int axis = e >> 2, u = (e >> 1) & 1, w = e & 1;
            // owner = the edge's minimum corner: the two other axes (increasing order) take offsets u, w
            const int oa = axis == 0 ? 0 : u, ob = axis == 1 ? 0 : (axis == 0 ? u : w), oc = axis == 2 ? 0 : w;
            const int ent = img[(long)(a + oa) * plane + (long)(b + ob) * m.P2 + (c + oc)];
            const int rank = __builtin_popcount((ent & 7) & ((1 << axis) - 1));
            faces[(tbase + j) * 3 + k] = (long)(ent >> 3) + rank - vshape;
        }
    }
}

// ---- surface sampling -----------------------------------------------------------------------------------------------------------
// cdf[f] (double) = sum of the doubled areas of triangles [tri_offsets[s], f] of shape s: one workgroup per shape, 256 triangles at a
// time, a fixed tree of additions (deterministic; the twin adds sequentially, which differs in the last bits of a double only)
__device__ __forceinline__ double mc_tri_area2(const float* __restrict__ verts, const int64_t* __restrict__ faces, long vbase, long f) {
    const long i0 = vbase + faces[f * 3], i1 = vbase + faces[f * 3 + 1], i2 = vbase + faces[f * 3 + 2];
    const double ax = (double)verts[i1 * 3] - (double)verts[i0 * 3], ay = (double)verts[i1 * 3 + 1] - (double)verts[i0 * 3 + 1],
                 az = (double)verts[i1 * 3 + 2] - (double)verts[i0 * 3 + 2];
    const double bx = (double)verts[i2 * 3] - (double)verts[i0 * 3], by = (double)verts[i2 * 3 + 1] - (double)verts[i0 * 3 + 1],
                 bz = (double)verts[i2 * 3 + 2] - (double)verts[i0 * 3 + 2];
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    return sqrt(cx * cx + cy * cy + cz * cz);
}

__global__ void __launch_bounds__(256) mesh_cdf_kernel(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                       const int64_t* __restrict__ vert_offsets,
                                                       const int64_t* __restrict__ tri_offsets, double* __restrict__ cdf) {
    __shared__ double lds[4];
    const long s = blockIdx.x;
    const long f0 = tri_offsets[s], f1 = tri_offsets[s + 1], vbase = vert_offsets[s];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double carry = 0.0;
    for (long f = f0; f < f1; f += 256) {
        const long my = f + threadIdx.x;
        double x = my < f1 ? mc_tri_area2(verts, faces, vbase, my) : 0.0;
        double incl = x;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double y = __shfl_up(incl, off, 64);
            if (lane >= off) incl += y;
        }
        if (lane == 63) lds[wave] = incl;
        __syncthreads();
        double before = 0.0, all = 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const double t = lds[w];
            before += w < wave ? t : 0.0;
            all += t;
        }
        __syncthreads();
        if (my < f1) cdf[my] = carry + (before + incl);
        carry += all;
    }
}

__global__ void __launch_bounds__(256) mesh_sample_kernel(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                          const int64_t* __restrict__ vert_offsets,
                                                          const int64_t* __restrict__ tri_offsets, const double* __restrict__ cdf,
                                                          const float* __restrict__ uniforms, long S, long P, float* __restrict__ out,
                                                          int* __restrict__ empty) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= S * P) return;
    const long s = i / P;
    const long f0 = tri_offsets[s], f1 = tri_offsets[s + 1];
    if (i % P == 0) empty[s] = f1 > f0 ? 0 : 1;
    if (f1 <= f0) {
        out[i * 3] = 0.f;
        out[i * 3 + 1] = 0.f;
        out[i * 3 + 2] = 0.f;
        return;
    }
    const float u0 = uniforms[i * 3], u1 = uniforms[i * 3 + 1], u2 = uniforms[i * 3 + 2];
    const double x = (double)u0 * cdf[f1 - 1];
    // first triangle whose cumulative area reaches x (numpy.searchsorted, side 'left'), clamped to the last one
    long lo = f0, hi = f1 - 1;
    while (lo < hi) {
        const long mid = lo + (hi - lo) / 2;
        if (cdf[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    const long vb = vert_offsets[s];
    const long i0 = vb + faces[lo * 3], i1 = vb + faces[lo * 3 + 1], i2 = vb + faces[lo * 3 + 2];
    float p = u1, q = u2;
    if (p + q > 1.f) {
        p = 1.f - p;
        q = 1.f - q;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float o = verts[i0 * 3 + k];
        out[i * 3 + k] = o + (p * (verts[i1 * 3 + k] - o) + q * (verts[i2 * 3 + k] - o));
    }
}

static bool mc_setup(McArgs& m, const float* grids, long S, int R0, int R1, int R2, float level, int pad, float pad_value) {
    if (!grids || S <= 0 || R0 <= 0 || R1 <= 0 || R2 <= 0 || (pad != 0 && pad != 1)) return false;
    m.grids = grids;
    m.S = S;
    m.R0 = R0;
    m.R1 = R1;
    m.R2 = R2;
    m.P0 = R0 + 2 * pad;
    m.P1 = R1 + 2 * pad;
    m.P2 = R2 + 2 * pad;
    m.pad = pad;
    m.pad_value = pad_value;
    m.level = level;
    m.cells = (long)m.P0 * m.P1 * m.P2;
    m.blocks = (int)((m.cells + kMcBlock - 1) / kMcBlock);
    // every int32 index (image entries vertex * 8 | mask, vertex / triangle counts and offsets) stays below 2^31
    return m.cells <= kMcIndexLimit / kMcSlots && S <= kMcIndexLimit / kMcSlots / m.cells;
}

}  // namespace sg

using namespace sg;

extern "C" {

size_t sg_mc_workspace_bytes(long S, int R0, int R1, int R2, int pad) {
    McArgs m;
    float dummy = 0.f;
    if (!mc_setup(m, &dummy, S, R0, R1, R2, 0.f, pad, 0.f)) return 0;
    return (size_t)(S * m.cells) * sizeof(int) + (size_t)(S * m.blocks) * 4 * sizeof(int);
}

int sg_mc_count(const float* grids, long S, int R0, int R1, int R2, float level, int pad, float pad_value, int64_t* vert_offsets,
                int64_t* tri_offsets, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    McArgs m;
    SG_CHECK_ARG(mc_setup(m, grids, S, R0, R1, R2, level, pad, pad_value));
    SG_CHECK_ARG(vert_offsets && tri_offsets && workspace);
    if (workspace_bytes < sg_mc_workspace_bytes(S, R0, R1, R2, pad)) SG_FAIL(SG_ERR_WORKSPACE, "sg_mc_count: workspace too small");
    int* image = (int*)workspace;
    int* block_tot = image + S * m.cells;
    int* block_off = block_tot + 2 * S * m.blocks;
    hipLaunchKernelGGL(mc_count_kernel, dim3((unsigned)m.blocks, (unsigned)S), dim3(kMcBlock), 0, stream, m, block_tot);
    hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(1024), 0, stream, block_tot, block_off, S * m.blocks, m.blocks, S,
                       vert_offsets, tri_offsets);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_mc_emit(const float* grids, long S, int R0, int R1, int R2, float level, int pad, float pad_value, float sx, float sy,
               float sz, float ox, float oy, float oz, const int64_t* vert_offsets, const int64_t* tri_offsets, float* vertices,
               float* normals, int64_t* faces, long max_verts, long max_tris, void* workspace, size_t workspace_bytes,
               hipStream_t stream) {
    McArgs m;
    SG_CHECK_ARG(mc_setup(m, grids, S, R0, R1, R2, level, pad, pad_value));
    SG_CHECK_ARG(vert_offsets && tri_offsets && workspace && max_verts >= 0 && max_tris >= 0);
    SG_CHECK_ARG((max_verts == 0 || (vertices && normals)) && (max_tris == 0 || faces));
    if (workspace_bytes < sg_mc_workspace_bytes(S, R0, R1, R2, pad)) SG_FAIL(SG_ERR_WORKSPACE, "sg_mc_emit: workspace too small");
    int* image = (int*)workspace;
    const int* block_off = image + S * m.cells + 2 * S * m.blocks;
    McGeom geo = {{sx, sy, sz}, {ox, oy, oz}};
    hipLaunchKernelGGL(mc_vertices_kernel, dim3((unsigned)m.blocks, (unsigned)S), dim3(kMcBlock), 0, stream, m, geo, block_off,
                       image, vertices, normals, max_verts);
    hipLaunchKernelGGL(mc_triangles_kernel, dim3((unsigned)m.blocks, (unsigned)S), dim3(kMcBlock), 0, stream, m, block_off,
                       (const int*)image, vert_offsets, faces, max_tris);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

size_t sg_mesh_sample_workspace_bytes(long S, long F) {
    if (S <= 0 || F < 0) return 0;
    return (size_t)(F > 0 ? F : 1) * sizeof(double);
}

int sg_mesh_sample(const float* vertices, const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S,
                   long F, const float* uniforms, long P, float* out, int* empty, void* workspace, size_t workspace_bytes,
                   hipStream_t stream) {
    SG_CHECK_ARG(vert_offsets && tri_offsets && uniforms && out && empty && workspace && S > 0 && P > 0 && F >= 0);
    SG_CHECK_ARG(F == 0 || (vertices && faces));
    SG_CHECK_ARG(S <= 2147483647L && P <= 2147483647L / 3 && S * P <= (1L << 40));
    if (workspace_bytes < sg_mesh_sample_workspace_bytes(S, F)) SG_FAIL(SG_ERR_WORKSPACE, "sg_mesh_sample: workspace too small");
    double* cdf = (double*)workspace;
    hipLaunchKernelGGL(mesh_cdf_kernel, dim3((unsigned)S), dim3(256), 0, stream, vertices, faces, vert_offsets, tri_offsets, cdf);
    const long n = S * P;
    hipLaunchKernelGGL(mesh_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, vertices, faces, vert_offsets,
                       tri_offsets, (const double*)cdf, uniforms, S, P, out, empty);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

}  // extern "C"
