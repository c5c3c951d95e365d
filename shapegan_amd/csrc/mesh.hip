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
#include "../../include/shapegan_hip.h"

// positions and normals are compared with the twin: no contraction of a * b + c into one rounding
#pragma clang fp contract(off)
#include "mesh_core.h"      // the per-cell arithmetic, shared with the twin

namespace sg {

constexpr int kMcBlock = 256;
static_assert(kMcBlock == 256, "sg_block_exclusive_256 scans four waves");

struct McArgs {
    const float* grids;
    long S;
    SgMcGrid grid;
    long cells;       // P0 * P1 * P2 per shape
    int blocks;       // workgroups per shape
};

__device__ __forceinline__ const float* mc_shape(const McArgs& m, long s) { return m.grids + s * (long)m.grid.R0 * m.grid.R1 * m.grid.R2; }

__device__ __forceinline__ void mc_decode(const McArgs& m, long cell, int& a, int& b, int& c) {
    const long plane = (long)m.grid.P1 * m.grid.P2;
    a = (int)(cell / plane);
    const long r = cell - (long)a * plane;
    b = (int)(r / m.grid.P2);
    c = (int)(r - (long)b * m.grid.P2);
}

__global__ void __launch_bounds__(kMcBlock) mc_count_kernel(McArgs m, int* __restrict__ block_tot) {
    __shared__ int lds[2][kMcBlock / 64];
    const long s = blockIdx.y;
    const long cell = (long)blockIdx.x * kMcBlock + threadIdx.x;
    const float* g = mc_shape(m, s);
    int nv = 0, nt = 0;
    if (cell < m.cells) {
        int a, b, c;
        mc_decode(m, cell, a, b, c);
        float v[8];
        sg_mc_corners(m.grid, g, a, b, c, v);
        const SgMcCell r = sg_mc_classify(m.grid, v, a, b, c);
        nv = r.nv;
        nt = r.nt;
    }
    int tv, tt;
    sg_block_exclusive_256(nv, lds[0], tv);
    sg_block_exclusive_256(nt, lds[1], tt);
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

struct McGeom {
    float sp[3], org[3];
};

__global__ void __launch_bounds__(kMcBlock) mc_vertices_kernel(McArgs m, McGeom geo, const int* __restrict__ block_off,
                                                               int* __restrict__ image, float* __restrict__ vertices,
                                                               float* __restrict__ normals, long max_verts) {
    __shared__ int lds[kMcBlock / 64];
    const long s = blockIdx.y;
    const long cell = (long)blockIdx.x * kMcBlock + threadIdx.x;
    const float* g = mc_shape(m, s);
    int a = 0, b = 0, c = 0;
    float v[8];
    SgMcCell r;
    r.nv = 0;
    r.mask = 0;
    if (cell < m.cells) {
        mc_decode(m, cell, a, b, c);
        sg_mc_corners(m.grid, g, a, b, c, v);
        r = sg_mc_classify(m.grid, v, a, b, c);
    }
    int total;
    const int excl = sg_block_exclusive_256(r.nv, lds, total);
    if (cell >= m.cells) return;
    const long base = (long)block_off[2 * (s * m.blocks + blockIdx.x)] + excl;
    image[s * m.cells + cell] = (int)(base * 8 + r.mask);
    if (!r.mask) return;
    float g0[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) g0[k] = sg_mc_grad(m.grid, g, a, b, c, k, geo.sp[k]);
    long out = base;
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
        if (!((r.mask >> axis) & 1)) continue;
        float pos[3], nrm[3];
        sg_mc_vertex(m.grid, g, geo.sp, geo.org, a, b, c, v, g0, axis, pos, nrm);
        if (out < max_verts) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                vertices[out * 3 + k] = pos[k];
                normals[out * 3 + k] = nrm[k];
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
    const float* g = mc_shape(m, s);
    int a = 0, b = 0, c = 0;
    SgMcCell r;
    r.nt = 0;
    r.cube = -1;
    if (cell < m.cells) {
        mc_decode(m, cell, a, b, c);
        float v[8];
        sg_mc_corners(m.grid, g, a, b, c, v);
        r = sg_mc_classify(m.grid, v, a, b, c);
    }
    int total;
    const int excl = sg_block_exclusive_256(r.nt, lds, total);
    if (cell >= m.cells || r.nt == 0) return;
    const long tbase = (long)block_off[2 * (s * m.blocks + blockIdx.x) + 1] + excl;
    const long vshape = vert_offsets[s];
    const int* img = image + s * m.cells;
    const long plane = (long)m.grid.P1 * m.grid.P2;
    for (int j = 0; j < r.nt; ++j) {
        if (tbase + j >= max_tris) break;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int oa, ob, oc;
            const int axis = sg_mc_edge_owner(sg_mc_tri_edges[r.cube][3 * j + k], oa, ob, oc);
            const int ent = img[(long)(a + oa) * plane + (long)(b + ob) * m.grid.P2 + (c + oc)];
            faces[(tbase + j) * 3 + k] = (long)(ent >> 3) + sg_mc_rank(ent, axis) - vshape;
        }
    }
}

// ---- surface sampling -----------------------------------------------------------------------------------------------------------
// cdf[f] (double) = sum of the doubled areas of triangles [tri_offsets[s], f] of shape s: one workgroup per shape, 256 triangles at a
// time, a fixed tree of additions (deterministic; the twin adds sequentially, which differs in the last bits of a double only)
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
        double x = 0.0;
        if (my < f1) x = sg_mesh_area2(verts + (vbase + faces[my * 3]) * 3, verts + (vbase + faces[my * 3 + 1]) * 3, verts + (vbase + faces[my * 3 + 2]) * 3);
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
    sg_mesh_point(verts + (vb + faces[lo * 3]) * 3, verts + (vb + faces[lo * 3 + 1]) * 3, verts + (vb + faces[lo * 3 + 2]) * 3, u1, u2, out + i * 3);
}

static bool mc_setup(McArgs& m, const float* grids, long S, int R0, int R1, int R2, float level, int pad, float pad_value) {
    if (!grids || !sg_mc_grid(m.grid, S, R0, R1, R2, level, pad, pad_value, m.cells)) return false;
    m.grids = grids;
    m.S = S;
    m.blocks = (int)((m.cells + kMcBlock - 1) / kMcBlock);
    return true;
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
