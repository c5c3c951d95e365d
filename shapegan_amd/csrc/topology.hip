// shapegan_amd/csrc/topology.hip — connected components of packed meshes, their statistics, and the compaction that keeps some (K12b).
//
// Replaces what the reference's callers took from trimesh (split, body_count, is_watertight, volume, euler_number), one mesh at a time
// on the host, with a handful of launches for a whole MeshBatch:
//   label    parent[v] = v; one lane per triangle hooks the roots of its corners, the larger index under the smaller, by compare-and-
//            swap; a flatten pass; an exclusive scan of the root flags (per-workgroup totals, one scanning workgroup, the offsets: the
//            way sg_mc_count builds its own) numbers the components by their lowest vertex;
//   keys     per triangle its component, per side its half-edge key: the Python layer sorts both (torch.sort);
//   stats    counts by integer atomics (one per wave where a wave agrees on the component), areas and volumes by the header's tiles;
//   keep     two scans (kept vertices, kept triangles), then the copy.
//
// Visibility of parent[] across the 8 L2s of the chip: inside the hooking kernel EVERY read of parent[] is a relaxed agent-scope
// atomic load or the value an atomic returned, a root is only ever changed by a compare-and-swap against the word itself, and the
// shortcuts are atomic minima (an entry only ever decreases, toward an ancestor).  A stale ancestor therefore costs steps, never a
// wrong hook.  Initialisation, hooking and flattening are separate kernels, so the flatten pass reads parent[] with plain loads.
#include "common.h"
#include "../../include/shapegan_hip.h"

// areas and volumes are compared with the twin bit for bit
#pragma clang fp contract(off)
#include "topology_core.h"

namespace sg {

constexpr int kTopoBlock = 256;
static_assert(kTopoBlock == 256 && SG_TOPO_TILE == 256, "sg_block_exclusive_256 scans four waves; a tile is one workgroup");

struct TopoMesh {
    const int64_t* faces;
    const int64_t* vert_offsets;
    const int64_t* tri_offsets;
    long S, V, F;
};

// the corners of triangle f as global vertex indices; false when the triangle is skipped
__device__ __forceinline__ bool topo_corners(const TopoMesh& m, long f, long& s, long& a, long& b, long& c) {
    s = sg_topo_shape_of(m.tri_offsets, m.S, f);
    const long vbase = m.vert_offsets[s];
    return sg_topo_triangle(m.faces + f * 3, vbase, m.vert_offsets[s + 1] - vbase, m.V, a, b, c);
}

__device__ __forceinline__ int topo_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x as far as this lane can see; halves the path on the way (an entry moves to a smaller ancestor, never elsewhere)
__device__ __forceinline__ int topo_find(int* parent, int x) {
    int p = topo_load(parent + x);
    while (p != x) {
        const int g = topo_load(parent + p);
        if (g != p) atomicMin(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void topo_union(int* parent, int a, int b) {
    int ra = topo_find(parent, a), rb = topo_find(parent, b);
    while (ra != rb) {
        if (ra < rb) {
            const int t = ra;
            ra = rb;
            rb = t;
        }
        const int old = atomicCAS(parent + ra, ra, rb);      // hooks only a word that still is a root
        if (old == ra) break;
        ra = topo_find(parent, old);
        rb = topo_find(parent, rb);
    }
}

__global__ void __launch_bounds__(kTopoBlock) topo_init_kernel(int* __restrict__ parent, int* __restrict__ named, long V) {
    const long v = (long)blockIdx.x * kTopoBlock + threadIdx.x;
    if (v >= V) return;
    parent[v] = (int)v;
    named[v] = 0;
}

__global__ void __launch_bounds__(kTopoBlock) topo_hook_kernel(TopoMesh m, int* parent, int* named) {
    const long f = (long)blockIdx.x * kTopoBlock + threadIdx.x;
    if (f >= m.F) return;
    long s, a, b, c;
    if (!topo_corners(m, f, s, a, b, c)) return;
    named[a] = 1;
    named[b] = 1;
    named[c] = 1;
    topo_union(parent, (int)a, (int)b);
    topo_union(parent, (int)b, (int)c);
}

__global__ void __launch_bounds__(kTopoBlock) topo_flatten_kernel(const int* __restrict__ parent, const int* __restrict__ named,
                                                                  int* __restrict__ root, int* __restrict__ is_root, long V) {
    const long v = (long)blockIdx.x * kTopoBlock + threadIdx.x;
    if (v >= V) return;
    int r = (int)v, p = parent[r];
    while (p != r) {
        r = p;
        p = parent[r];
    }
    root[v] = r;
    is_root[v] = (r == (int)v && named[v]) ? 1 : 0;
}

// ---- exclusive scan of n flags: per-workgroup totals, one scanning workgroup, the positions ----------------------------------------
__global__ void __launch_bounds__(kTopoBlock) topo_scan_totals_kernel(const int* __restrict__ flag, long n, int* __restrict__ block_tot) {
    __shared__ int lds[kTopoBlock / 64];
    const long i = (long)blockIdx.x * kTopoBlock + threadIdx.x;
    int total;
    sg_block_exclusive_256(i < n ? flag[i] : 0, lds, total);
    if (threadIdx.x == 0) block_tot[blockIdx.x] = total;
}

// one workgroup of 1024: thread i scans a contiguous range of the nb totals; block_off[nb] = the grand total
__global__ void __launch_bounds__(1024) topo_scan_blocks_kernel(const int* __restrict__ block_tot, int* __restrict__ block_off, long nb) {
    __shared__ int part[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long per = (nb + 1023) / 1024;
    const long i0 = threadIdx.x * per < nb ? threadIdx.x * per : nb, i1 = i0 + per < nb ? i0 + per : nb;
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
    if (threadIdx.x == 0) block_off[nb] = all;
}

__global__ void __launch_bounds__(kTopoBlock) topo_scan_positions_kernel(const int* __restrict__ flag, long n,
                                                                         const int* __restrict__ block_off, int* __restrict__ excl) {
    __shared__ int lds[kTopoBlock / 64];
    const long i = (long)blockIdx.x * kTopoBlock + threadIdx.x;
    int total;
    const int e = sg_block_exclusive_256(i < n ? flag[i] : 0, lds, total);
    if (i < n) excl[i] = block_off[blockIdx.x] + e;
}

// out[t] = the position of the first element of shape t (t = S: the total)
__global__ void __launch_bounds__(kTopoBlock) topo_offsets_kernel(const int64_t* __restrict__ offsets, long S, long n,
                                                                  const int* __restrict__ excl, const int* __restrict__ total,
                                                                  int64_t* __restrict__ out) {
    const long t = (long)blockIdx.x * kTopoBlock + threadIdx.x;
    if (t > S) return;
    const long o = offsets[t];
    out[t] = t == S || o >= n ? *total : (o < 0 ? 0 : excl[o]);
}

__global__ void __launch_bounds__(kTopoBlock) topo_number_kernel(const int64_t* __restrict__ vert_offsets, long S, long V,
                                                                 const int* __restrict__ named, const int* __restrict__ root,
                                                                 const int* __restrict__ excl, const int64_t* __restrict__ comp_offsets,
                                                                 int* __restrict__ vertex_component) {
    const long v = (long)blockIdx.x * kTopoBlock + threadIdx.x;
    if (v >= V) return;
    int label = -1;
    if (named[v]) label = (int)((long)excl[root[v]] - comp_offsets[sg_topo_shape_of(vert_offsets, S, v)]);
    vertex_component[v] = label;
}

// ---- keys -----------------------------------------------------------------------------------------------------------------------------
// the component (batch-wide number) of global vertex v, -1 when it has none or the labels do not fit the offsets
__device__ __forceinline__ long topo_component_of(const int64_t* vert_offsets, long S, long v, const int* vertex_component,
                                                  const int64_t* comp_offsets, long C) {
    const int label = vertex_component[v];
    if (label < 0) return -1;
    const long c = comp_offsets[sg_topo_shape_of(vert_offsets, S, v)] + label;
    return c < C ? c : -1;
}

__global__ void __launch_bounds__(kTopoBlock) topo_keys_kernel(TopoMesh m, const int* __restrict__ vertex_component,
                                                               const int64_t* __restrict__ comp_offsets, long C,
                                                               int* __restrict__ tri_keys, int64_t* __restrict__ edge_keys) {
    const long f = (long)blockIdx.x * kTopoBlock + threadIdx.x;
    if (f >= m.F) return;
    long s, a, b, c;
    long comp = -1;
    if (topo_corners(m, f, s, a, b, c)) comp = topo_component_of(m.vert_offsets, m.S, a, vertex_component, comp_offsets, C);
    tri_keys[f] = comp < 0 ? SG_TOPO_NO_COMPONENT : (int)comp;
    edge_keys[3 * f] = comp < 0 ? SG_TOPO_NO_EDGE : sg_topo_edge_key(a, b);
    edge_keys[3 * f + 1] = comp < 0 ? SG_TOPO_NO_EDGE : sg_topo_edge_key(b, c);
    edge_keys[3 * f + 2] = comp < 0 ? SG_TOPO_NO_EDGE : sg_topo_edge_key(c, a);
}

// ---- statistics -----------------------------------------------------------------------------------------------------------------------
// counts[comp] += 1 for every active lane: one atomic for the wave when its active lanes agree on the component (the usual case: a
// large component fills whole waves), one per lane otherwise.  Called by all 64 lanes.
__device__ __forceinline__ void topo_count(int* counts, long comp, bool active) {
    const unsigned long long mask = __ballot(active);
    if (!mask) return;
    const int leader = __ffsll((long long)mask) - 1;
    const long c0 = __shfl((int)comp, leader, 64);
    if (__all(!active || comp == c0)) {
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(counts + c0, __popcll(mask));
    } else if (active) {
        atomicAdd(counts + comp, 1);
    }
}

__global__ void __launch_bounds__(kTopoBlock) topo_zero_counts_kernel(int* __restrict__ n_vertices, int* __restrict__ n_edges,
                                                                      int* __restrict__ n_open, long C) {
    const long c = (long)blockIdx.x * kTopoBlock + threadIdx.x;
    if (c >= C) return;
    n_vertices[c] = 0;
    n_edges[c] = 0;
    n_open[c] = 0;
}

__global__ void __launch_bounds__(kTopoBlock) topo_count_vertices_kernel(const int64_t* __restrict__ vert_offsets, long S, long V,
                                                                         const int* __restrict__ vertex_component,
                                                                         const int64_t* __restrict__ comp_offsets, long C,
                                                                         int* n_vertices) {
    const long v = (long)blockIdx.x * kTopoBlock + threadIdx.x;
    const long comp = v < V ? topo_component_of(vert_offsets, S, v, vertex_component, comp_offsets, C) : -1;
    topo_count(n_vertices, comp, comp >= 0);
}

// one lane per sorted half-edge; the first of a run of one undirected edge counts the sides in both directions
__global__ void __launch_bounds__(kTopoBlock) topo_count_edges_kernel(const int64_t* __restrict__ edge_sorted, long n,
                                                                      const int64_t* __restrict__ vert_offsets, long S, long V,
                                                                      const int* __restrict__ vertex_component,
                                                                      const int64_t* __restrict__ comp_offsets, long C, int* n_edges,
                                                                      int* n_open) {
    const long i = (long)blockIdx.x * kTopoBlock + threadIdx.x;
    long comp = -1;
    bool open = false;
    if (i < n) {
        const int64_t key = edge_sorted[i];
        if (key != SG_TOPO_NO_EDGE && key >= 0 && (i == 0 || !sg_topo_same_edge(edge_sorted[i - 1], key))) {
            long forward = 0, backward = 0;
            for (long j = i; j < n; ++j) {
                const int64_t k = edge_sorted[j];
                if (!sg_topo_same_edge(k, key)) break;
                if (k & 1)
                    ++backward;
                else
                    ++forward;
            }
            const long low = sg_topo_edge_low(key);
            if (low < V) comp = topo_component_of(vert_offsets, S, low, vertex_component, comp_offsets, C);
            open = !(forward == 1 && backward == 1);
        }
    }
    topo_count(n_edges, comp, comp >= 0);
    topo_count(n_open, comp, comp >= 0 && open);
}

// one workgroup per tile of SG_TOPO_TILE triangles of ONE component: the header's tree
__global__ void __launch_bounds__(kTopoBlock) topo_tile_sums_kernel(TopoMesh m, const float* __restrict__ vertices, long C,
                                                                    const int64_t* __restrict__ tri_order,
                                                                    const int64_t* __restrict__ seg_offsets,
                                                                    const int64_t* __restrict__ tile_offsets, double* __restrict__ sums) {
    __shared__ double lds[2][kTopoBlock / 64];
    const long tile = blockIdx.x;
    if (tile >= tile_offsets[C]) return;
    const long c = sg_topo_shape_of(tile_offsets, C, tile);
    const long i = seg_offsets[c] + (tile - tile_offsets[c]) * SG_TOPO_TILE + threadIdx.x;
    double area = 0.0, volume = 0.0;
    if (i < seg_offsets[c + 1] && i >= 0 && i < m.F) {
        const long f = tri_order[i];
        long s, a, b, cc;
        if (f >= 0 && f < m.F && topo_corners(m, f, s, a, b, cc)) sg_topo_terms(vertices + a * 3, vertices + b * 3, vertices + cc * 3, area, volume);
    }
    area = sg_wave_sum_d(area);
    volume = sg_wave_sum_d(volume);
    if ((threadIdx.x & 63) == 0) {
        lds[0][threadIdx.x >> 6] = area;
        lds[1][threadIdx.x >> 6] = volume;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sums[2 * tile] = ((lds[0][0] + lds[0][1]) + lds[0][2]) + lds[0][3];
        sums[2 * tile + 1] = ((lds[1][0] + lds[1][1]) + lds[1][2]) + lds[1][3];
    }
}

// one wave per component: its tiles added in increasing order
__global__ void __launch_bounds__(kTopoBlock) topo_finish_kernel(long C, const int64_t* __restrict__ seg_offsets,
                                                                 const int64_t* __restrict__ tile_offsets,
                                                                 const double* __restrict__ sums, long max_tiles,
                                                                 int* __restrict__ n_triangles,
                                                                 double* __restrict__ area, double* __restrict__ volume) {
    const long c = (long)blockIdx.x * (kTopoBlock / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (c >= C) return;
    const long t0 = tile_offsets[c] > 0 ? tile_offsets[c] : 0;
    const long t1 = tile_offsets[c + 1] < max_tiles ? tile_offsets[c + 1] : max_tiles;      // sums[] holds max_tiles pairs
    double sa = 0.0, sv = 0.0;
    for (long base = t0; base < t1; base += 64) {
        const bool mine = base + lane < t1;
        const double xa = mine ? sums[2 * (base + lane)] : 0.0, xv = mine ? sums[2 * (base + lane) + 1] : 0.0;
        const int count = t1 - base < 64 ? (int)(t1 - base) : 64;
        for (int j = 0; j < count; ++j) {
            sa += __shfl(xa, j, 64);
            sv += __shfl(xv, j, 64);
        }
    }
    if (lane == 0) {
        n_triangles[c] = (int)(seg_offsets[c + 1] - seg_offsets[c]);
        area[c] = sa;
        volume[c] = sv;
    }
}

// ---- compaction -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTopoBlock) topo_keep_vertices_kernel(const int64_t* __restrict__ vert_offsets, long S, long V,
                                                                        const int* __restrict__ vertex_component,
                                                                        const int64_t* __restrict__ comp_offsets, long C,
                                                                        const uint8_t* __restrict__ keep, int* __restrict__ kept) {
    const long v = (long)blockIdx.x * kTopoBlock + threadIdx.x;
    if (v >= V) return;
    const long comp = topo_component_of(vert_offsets, S, v, vertex_component, comp_offsets, C);
    kept[v] = comp >= 0 && keep[comp] ? 1 : 0;
}

__global__ void __launch_bounds__(kTopoBlock) topo_keep_triangles_kernel(TopoMesh m, const int* __restrict__ kept_vertex,
                                                                         int* __restrict__ kept) {
    const long f = (long)blockIdx.x * kTopoBlock + threadIdx.x;
    if (f >= m.F) return;
    long s, a, b, c;
    kept[f] = topo_corners(m, f, s, a, b, c) && kept_vertex[a] ? 1 : 0;
}

__global__ void __launch_bounds__(kTopoBlock) topo_emit_vertices_kernel(const uint32_t* __restrict__ vertices,
                                                                        const uint32_t* __restrict__ normals, long V,
                                                                        const int* __restrict__ kept, const int* __restrict__ pos,
                                                                        uint32_t* __restrict__ out_vertices,
                                                                        uint32_t* __restrict__ out_normals, long max_verts) {
    const long v = (long)blockIdx.x * kTopoBlock + threadIdx.x;
    if (v >= V || !kept[v]) return;
    const long o = pos[v];
    if (o >= max_verts) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out_vertices[o * 3 + k] = vertices[v * 3 + k];
        out_normals[o * 3 + k] = normals[v * 3 + k];
    }
}

__global__ void __launch_bounds__(kTopoBlock) topo_emit_faces_kernel(TopoMesh m, const int* __restrict__ kept,
                                                                     const int* __restrict__ pos, const int* __restrict__ vertex_pos,
                                                                     const int64_t* __restrict__ new_vert_offsets,
                                                                     int64_t* __restrict__ out_faces, long max_tris) {
    const long f = (long)blockIdx.x * kTopoBlock + threadIdx.x;
    if (f >= m.F || !kept[f]) return;
    const long o = pos[f];
    long s, a, b, c;
    if (o >= max_tris || !topo_corners(m, f, s, a, b, c)) return;
    const long base = new_vert_offsets[s];
    out_faces[o * 3] = vertex_pos[a] - base;
    out_faces[o * 3 + 1] = vertex_pos[b] - base;
    out_faces[o * 3 + 2] = vertex_pos[c] - base;
}

static inline long topo_blocks(long n) { return (n + kTopoBlock - 1) / kTopoBlock; }

// positions of the set flags and, per shape, the position of its first element; tot / off: topo_blocks(n) and topo_blocks(n) + 1 ints
static void topo_scan(const int* flag, long n, int* excl, int* tot, int* off, const int64_t* offsets, long S, int64_t* out,
                      hipStream_t stream) {
    const long nb = topo_blocks(n);
    if (nb) hipLaunchKernelGGL(topo_scan_totals_kernel, dim3((unsigned)nb), dim3(kTopoBlock), 0, stream, flag, n, tot);
    hipLaunchKernelGGL(topo_scan_blocks_kernel, dim3(1), dim3(1024), 0, stream, (const int*)tot, off, nb);
    if (nb) hipLaunchKernelGGL(topo_scan_positions_kernel, dim3((unsigned)nb), dim3(kTopoBlock), 0, stream, flag, n, (const int*)off, excl);
    hipLaunchKernelGGL(topo_offsets_kernel, dim3((unsigned)topo_blocks(S + 1)), dim3(kTopoBlock), 0, stream, offsets, S, n,
                       (const int*)excl, (const int*)(off + nb), out);
}

static bool topo_sizes(long S, long V, long F) { return S >= 1 && S < 2147483647L && V >= 0 && F >= 0 && V <= 2147483647L && F <= 2147483647L; }

}  // namespace sg

using namespace sg;

extern "C" {

size_t sg_topo_label_workspace_bytes(long S, long V) {
    if (!topo_sizes(S, V, 0)) return 0;
    return (size_t)(5 * V + 2 * topo_blocks(V) + 2) * sizeof(int);
}

int sg_topo_label(const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                  int* vertex_component, int64_t* comp_offsets, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    SG_CHECK_ARG(topo_sizes(S, V, F));
    SG_CHECK_ARG(vert_offsets && tri_offsets && comp_offsets && workspace && (V == 0 || vertex_component) && (F == 0 || faces));
    if (workspace_bytes < sg_topo_label_workspace_bytes(S, V)) SG_FAIL(SG_ERR_WORKSPACE, "sg_topo_label: workspace too small");
    const long nb = topo_blocks(V);
    int* parent = (int*)workspace;
    int* named = parent + V;
    int* root = named + V;
    int* is_root = root + V;
    int* excl = is_root + V;
    int* tot = excl + V;
    int* off = tot + nb;
    const TopoMesh m = {faces, vert_offsets, tri_offsets, S, V, F};
    if (nb) hipLaunchKernelGGL(topo_init_kernel, dim3((unsigned)nb), dim3(kTopoBlock), 0, stream, parent, named, V);
    if (F && nb) hipLaunchKernelGGL(topo_hook_kernel, dim3((unsigned)topo_blocks(F)), dim3(kTopoBlock), 0, stream, m, parent, named);
    if (nb) hipLaunchKernelGGL(topo_flatten_kernel, dim3((unsigned)nb), dim3(kTopoBlock), 0, stream, (const int*)parent, (const int*)named, root, is_root, V);
    topo_scan(is_root, V, excl, tot, off, vert_offsets, S, comp_offsets, stream);
    if (nb) hipLaunchKernelGGL(topo_number_kernel, dim3((unsigned)nb), dim3(kTopoBlock), 0, stream, vert_offsets, S, V, (const int*)named, (const int*)root, (const int*)excl, (const int64_t*)comp_offsets, vertex_component);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_topo_keys(const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                 const int* vertex_component, const int64_t* comp_offsets, long C, int* tri_keys, int64_t* edge_keys,
                 hipStream_t stream) {
    SG_CHECK_ARG(topo_sizes(S, V, F) && C >= 0 && C <= V);
    SG_CHECK_ARG(vert_offsets && tri_offsets && comp_offsets && (V == 0 || vertex_component) && (F == 0 || (faces && tri_keys && edge_keys)));
    const TopoMesh m = {faces, vert_offsets, tri_offsets, S, V, F};
    if (F) hipLaunchKernelGGL(topo_keys_kernel, dim3((unsigned)topo_blocks(F)), dim3(kTopoBlock), 0, stream, m, vertex_component, comp_offsets, C, tri_keys, edge_keys);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

size_t sg_topo_stats_workspace_bytes(long F, long C) {
    if (F < 0 || C < 0 || F > 2147483647L || C > 2147483647L) return 0;
    return (size_t)(F / SG_TOPO_TILE + C + 1) * 2 * sizeof(double);
}

int sg_topo_stats(const float* vertices, const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V,
                  long F, const int* vertex_component, const int64_t* comp_offsets, long C, const int64_t* tri_order,
                  const int64_t* seg_offsets, const int64_t* tile_offsets, const int64_t* edge_sorted, int* n_vertices,
                  int* n_triangles, int* n_edges, int* n_open, double* area, double* volume, void* workspace, size_t workspace_bytes,
                  hipStream_t stream) {
    SG_CHECK_ARG(topo_sizes(S, V, F) && C >= 0 && C <= V);
    SG_CHECK_ARG(vert_offsets && tri_offsets && comp_offsets && seg_offsets && tile_offsets && workspace);
    SG_CHECK_ARG((V == 0 || (vertices && vertex_component)) && (F == 0 || (faces && tri_order && edge_sorted)));
    SG_CHECK_ARG(C == 0 || (n_vertices && n_triangles && n_edges && n_open && area && volume));
    if (workspace_bytes < sg_topo_stats_workspace_bytes(F, C)) SG_FAIL(SG_ERR_WORKSPACE, "sg_topo_stats: workspace too small");
    if (C == 0) return SG_OK;
    const TopoMesh m = {faces, vert_offsets, tri_offsets, S, V, F};
    const unsigned cb = (unsigned)topo_blocks(C);
    double* sums = (double*)workspace;
    hipLaunchKernelGGL(topo_zero_counts_kernel, dim3(cb), dim3(kTopoBlock), 0, stream, n_vertices, n_edges, n_open, C);
    hipLaunchKernelGGL(topo_count_vertices_kernel, dim3((unsigned)topo_blocks(V)), dim3(kTopoBlock), 0, stream, vert_offsets, S, V, vertex_component, comp_offsets, C, n_vertices);
    if (F) hipLaunchKernelGGL(topo_count_edges_kernel, dim3((unsigned)topo_blocks(3 * F)), dim3(kTopoBlock), 0, stream, edge_sorted, 3 * F, vert_offsets, S, V, vertex_component, comp_offsets, C, n_edges, n_open);
    // every component has at most F / TILE full tiles in all plus one ragged tile of its own
    hipLaunchKernelGGL(topo_tile_sums_kernel, dim3((unsigned)(F / SG_TOPO_TILE + C)), dim3(kTopoBlock), 0, stream, m, vertices, C, tri_order, seg_offsets, tile_offsets, sums);
    hipLaunchKernelGGL(topo_finish_kernel, dim3((unsigned)((C + 3) / 4)), dim3(kTopoBlock), 0, stream, C, seg_offsets, tile_offsets, (const double*)sums, F / SG_TOPO_TILE + C, n_triangles, area, volume);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

size_t sg_topo_keep_workspace_bytes(long S, long V, long F) {
    if (!topo_sizes(S, V, F)) return 0;
    return (size_t)(2 * V + 2 * F + 2 * topo_blocks(V) + 2 * topo_blocks(F) + 4) * sizeof(int);
}

namespace sg {
struct TopoKeepScratch {
    int *kept_v, *pos_v, *kept_t, *pos_t, *tot_v, *off_v, *tot_t, *off_t;
};
static TopoKeepScratch topo_keep_scratch(void* workspace, long V, long F) {
    TopoKeepScratch k;
    k.kept_v = (int*)workspace;
    k.pos_v = k.kept_v + V;
    k.kept_t = k.pos_v + V;
    k.pos_t = k.kept_t + F;
    k.tot_v = k.pos_t + F;
    k.off_v = k.tot_v + topo_blocks(V);
    k.tot_t = k.off_v + topo_blocks(V) + 1;
    k.off_t = k.tot_t + topo_blocks(F);
    return k;
}
}  // namespace sg

int sg_topo_keep_count(const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                       const int* vertex_component, const int64_t* comp_offsets, long C, const uint8_t* keep,
                       int64_t* new_vert_offsets, int64_t* new_tri_offsets, void* workspace, size_t workspace_bytes,
                       hipStream_t stream) {
    SG_CHECK_ARG(topo_sizes(S, V, F) && C >= 0 && C <= V);
    SG_CHECK_ARG(vert_offsets && tri_offsets && comp_offsets && new_vert_offsets && new_tri_offsets && workspace);
    SG_CHECK_ARG((V == 0 || vertex_component) && (F == 0 || faces) && (C == 0 || keep));
    if (workspace_bytes < sg_topo_keep_workspace_bytes(S, V, F)) SG_FAIL(SG_ERR_WORKSPACE, "sg_topo_keep_count: workspace too small");
    const TopoKeepScratch k = topo_keep_scratch(workspace, V, F);
    const TopoMesh m = {faces, vert_offsets, tri_offsets, S, V, F};
    if (V) hipLaunchKernelGGL(topo_keep_vertices_kernel, dim3((unsigned)topo_blocks(V)), dim3(kTopoBlock), 0, stream, vert_offsets, S, V, vertex_component, comp_offsets, C, keep, k.kept_v);
    if (F) hipLaunchKernelGGL(topo_keep_triangles_kernel, dim3((unsigned)topo_blocks(F)), dim3(kTopoBlock), 0, stream, m, (const int*)k.kept_v, k.kept_t);
    topo_scan(k.kept_v, V, k.pos_v, k.tot_v, k.off_v, vert_offsets, S, new_vert_offsets, stream);
    topo_scan(k.kept_t, F, k.pos_t, k.tot_t, k.off_t, tri_offsets, S, new_tri_offsets, stream);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_topo_keep_emit(const float* vertices, const float* normals, const int64_t* faces, const int64_t* vert_offsets,
                      const int64_t* tri_offsets, long S, long V, long F, const int64_t* new_vert_offsets, float* out_vertices,
                      float* out_normals, int64_t* out_faces, long max_verts, long max_tris, void* workspace, size_t workspace_bytes,
                      hipStream_t stream) {
    SG_CHECK_ARG(topo_sizes(S, V, F) && max_verts >= 0 && max_tris >= 0);
    SG_CHECK_ARG(vert_offsets && tri_offsets && new_vert_offsets && workspace);
    SG_CHECK_ARG((V == 0 || (vertices && normals)) && (F == 0 || faces));
    SG_CHECK_ARG((max_verts == 0 || (out_vertices && out_normals)) && (max_tris == 0 || out_faces));
    if (workspace_bytes < sg_topo_keep_workspace_bytes(S, V, F)) SG_FAIL(SG_ERR_WORKSPACE, "sg_topo_keep_emit: workspace too small");
    const TopoKeepScratch k = topo_keep_scratch(workspace, V, F);
    const TopoMesh m = {faces, vert_offsets, tri_offsets, S, V, F};
    if (V && max_verts) hipLaunchKernelGGL(topo_emit_vertices_kernel, dim3((unsigned)topo_blocks(V)), dim3(kTopoBlock), 0, stream, (const uint32_t*)vertices, (const uint32_t*)normals, V, (const int*)k.kept_v, (const int*)k.pos_v, (uint32_t*)out_vertices, (uint32_t*)out_normals, max_verts);
    if (F && max_tris) hipLaunchKernelGGL(topo_emit_faces_kernel, dim3((unsigned)topo_blocks(F)), dim3(kTopoBlock), 0, stream, m, (const int*)k.kept_t, (const int*)k.pos_t, (const int*)k.pos_v, new_vert_offsets, out_faces, max_tris);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

}  // extern "C"
