// shapegan_amd/csrc/simplify.hip — mesh simplification by quadric vertex clustering on packed meshes (K12c).
//
// What trimesh users take from simplify_*: a MeshBatch made smaller in one pass, without a priority queue or a data-dependent
// iteration.  csrc/simplify_core.h states the contract and the order of every sum; the stages, each its own entry point:
//   bounds    one workgroup per shape: the bounding box of its finite coordinates (integer images of the floats: no order matters);
//   keys      one lane per vertex: its cell key;                       the Python layer sorts the keys stably (torch.sort);
//   count     one lane per triangle: the survivors per shape from the keys alone, by integer atomics (the target search);
//   clusters  one lane per sorted key: run heads, their exclusive scan = the cluster numbers, the clusters per shape;
//   corners   one lane per triangle: up to three records cluster << 31 | triangle;           the Python layer sorts them;
//   place     one WAVE per cluster: finds its vertex run and its corner run by bisection, adds both in the header's tiles of 64
//             (a tile is one step of the wave, the butterfly is the header's tree), lane 0 solves and stores;
//   faces     marks the clusters a surviving triangle names (plain stores of 1), two scans, the compaction.
// No floating-point atomic anywhere; every phase that needs memory settled ends at a kernel boundary.
#include "common.h"
#include "../../include/shapegan_hip.h"

// positions and normals are compared with the twin bit for bit
#pragma clang fp contract(off)
#include "simplify_core.h"

namespace sg {

constexpr int kSimpBlock = 256;
static_assert(kSimpBlock == 256 && SG_SIMPLIFY_TILE == 64, "sg_block_exclusive_256 scans four waves; a tile of the sums is one wave");

struct SimpMesh {
    const int64_t* faces;
    const int64_t* vert_offsets;
    const int64_t* tri_offsets;
    long S, V, F;
};

// the corners of triangle f as global vertex indices; false when the triangle is skipped
__device__ __forceinline__ bool simp_corners(const SimpMesh& m, long f, long& s, long& a, long& b, long& c) {
    s = sg_topo_shape_of(m.tri_offsets, m.S, f);
    const long vbase = m.vert_offsets[s];
    return sg_topo_triangle(m.faces + f * 3, vbase, m.vert_offsets[s + 1] - vbase, m.V, a, b, c);
}

// ---- bounds ---------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSimpBlock) simp_bounds_kernel(const float* __restrict__ vertices, const int64_t* __restrict__ vert_offsets,
                                                                 long V, float* __restrict__ lo, float* __restrict__ hi) {
    __shared__ int lds[6][kSimpBlock / 64];
    const long s = blockIdx.x;
    long v0 = vert_offsets[s], v1 = vert_offsets[s + 1];
    v0 = v0 < 0 ? 0 : v0;
    v1 = v1 > V ? V : v1;
    const int kmax = sg_float_key(3.4028234663852886e38f), kmin = sg_float_key(-3.4028234663852886e38f);
    int mn[3] = {kmax, kmax, kmax}, mx[3] = {kmin, kmin, kmin};
    for (long v = v0 + threadIdx.x; v < v1; v += kSimpBlock) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float x = vertices[v * 3 + k];
            if (fabsf(x) <= 3.4028234663852886e38f) {      // finite
                const int key = sg_float_key(x);
                mn[k] = key < mn[k] ? key : mn[k];
                mx[k] = key > mx[k] ? key : mx[k];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int a = __shfl_xor(mn[k], off, 64), b = __shfl_xor(mx[k], off, 64);
            mn[k] = a < mn[k] ? a : mn[k];
            mx[k] = b > mx[k] ? b : mx[k];
        }
        if ((threadIdx.x & 63) == 0) {
            lds[k][threadIdx.x >> 6] = mn[k];
            lds[3 + k][threadIdx.x >> 6] = mx[k];
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = threadIdx.x;
        int a = lds[k][0], b = lds[3 + k][0];
#pragma unroll
        for (int w = 1; w < kSimpBlock / 64; ++w) {
            a = lds[k][w] < a ? lds[k][w] : a;
            b = lds[3 + k][w] > b ? lds[3 + k][w] : b;
        }
        // an axis without a finite coordinate (a shape without vertices): [0, 0]
        lo[s * 3 + k] = a <= b ? sg_key_float(a) : 0.0f;
        hi[s * 3 + k] = a <= b ? sg_key_float(b) : 0.0f;
    }
}

// ---- keys -----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSimpBlock) simp_keys_kernel(const float* __restrict__ vertices, const int64_t* __restrict__ vert_offsets,
                                                               long S, long V, const float* __restrict__ origin,
                                                               const float* __restrict__ cell, const int* __restrict__ cells,
                                                               int64_t* __restrict__ keys) {
    const long v = (long)blockIdx.x * kSimpBlock + threadIdx.x;
    if (v >= V) return;
    const long s = sg_topo_shape_of(vert_offsets, S, v);
    const float p[3] = {vertices[v * 3], vertices[v * 3 + 1], vertices[v * 3 + 2]};
    const float o[3] = {origin[s * 3], origin[s * 3 + 1], origin[s * 3 + 2]};
    keys[v] = sg_simplify_key(s, p, o, cell[s * 2 + 1], cells[s]);
}

// ---- count: the survivors per shape from the keys alone --------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSimpBlock) simp_zero_kernel(int* __restrict__ x, long n) {
    const long i = (long)blockIdx.x * kSimpBlock + threadIdx.x;
    if (i < n) x[i] = 0;
}

// counts[s] += 1 for every active lane: one atomic for the wave when its active lanes agree on the shape (the usual case)
__device__ __forceinline__ void simp_count(int* counts, long s, bool active) {
    const unsigned long long mask = __ballot(active);
    if (!mask) return;
    const int leader = __ffsll((long long)mask) - 1;
    const long s0 = __shfl((int)s, leader, 64);
    if (__all(!active || s == s0)) {
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(counts + s0, __popcll(mask));
    } else if (active) {
        atomicAdd(counts + s, 1);
    }
}

__global__ void __launch_bounds__(kSimpBlock) simp_count_kernel(SimpMesh m, const int64_t* __restrict__ keys, int* counts) {
    const long f = (long)blockIdx.x * kSimpBlock + threadIdx.x;
    long s = 0, a, b, c;
    bool survives = false;
    if (f < m.F && simp_corners(m, f, s, a, b, c)) {
        const int64_t ka = keys[a], kb = keys[b], kc = keys[c];
        survives = ka != kb && kb != kc && ka != kc;
    }
    simp_count(counts, s, survives);
}

// ---- exclusive scan of n flags: per-workgroup totals, one scanning workgroup, the positions (the scheme of csrc/topology.hip) ----------
__global__ void __launch_bounds__(kSimpBlock) simp_scan_totals_kernel(const int* __restrict__ flag, long n, int* __restrict__ block_tot) {
    __shared__ int lds[kSimpBlock / 64];
    const long i = (long)blockIdx.x * kSimpBlock + threadIdx.x;
    int total;
    sg_block_exclusive_256(i < n ? flag[i] : 0, lds, total);
    if (threadIdx.x == 0) block_tot[blockIdx.x] = total;
}

// one workgroup of 1024: thread i scans a contiguous range of the nb totals; block_off[nb] = the grand total
__global__ void __launch_bounds__(1024) simp_scan_blocks_kernel(const int* __restrict__ block_tot, int* __restrict__ block_off, long nb) {
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

__global__ void __launch_bounds__(kSimpBlock) simp_scan_positions_kernel(const int* __restrict__ flag, long n,
                                                                         const int* __restrict__ block_off, int* __restrict__ excl) {
    __shared__ int lds[kSimpBlock / 64];
    const long i = (long)blockIdx.x * kSimpBlock + threadIdx.x;
    int total;
    const int e = sg_block_exclusive_256(i < n ? flag[i] : 0, lds, total);
    if (i < n) excl[i] = block_off[blockIdx.x] + e;
}

// out[t] = the position of the first element of shape t (t = S: the total)
__global__ void __launch_bounds__(kSimpBlock) simp_offsets_kernel(const int64_t* __restrict__ offsets, long S, long n,
                                                                  const int* __restrict__ excl, const int* __restrict__ total,
                                                                  int64_t* __restrict__ out) {
    const long t = (long)blockIdx.x * kSimpBlock + threadIdx.x;
    if (t > S) return;
    const long o = offsets[t];
    out[t] = t == S || o >= n ? *total : (o < 0 ? 0 : excl[o]);
}

// ---- clusters -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSimpBlock) simp_heads_kernel(const int64_t* __restrict__ sorted_keys, long V, int* __restrict__ head) {
    const long i = (long)blockIdx.x * kSimpBlock + threadIdx.x;
    if (i < V) head[i] = i == 0 || sorted_keys[i] != sorted_keys[i - 1] ? 1 : 0;
}

__global__ void __launch_bounds__(kSimpBlock) simp_number_kernel(const int64_t* __restrict__ order, long V, const int* __restrict__ head,
                                                                 const int* __restrict__ excl, int* __restrict__ sorted_cluster,
                                                                 int* __restrict__ vertex_cluster) {
    const long i = (long)blockIdx.x * kSimpBlock + threadIdx.x;
    if (i >= V) return;
    const int c = excl[i] + head[i] - 1;
    sorted_cluster[i] = c;
    const long v = order[i];
    if (v >= 0 && v < V) vertex_cluster[v] = c;      // `order` is a permutation: every vertex is written once
}

// ---- corners --------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSimpBlock) simp_corners_kernel(SimpMesh m, const int* __restrict__ vertex_cluster,
                                                                  int64_t* __restrict__ corner_keys) {
    const long f = (long)blockIdx.x * kSimpBlock + threadIdx.x;
    if (f >= m.F) return;
    long s, a, b, c, ca = 0, cb = 0, cc = 0;
    const bool counts = simp_corners(m, f, s, a, b, c);
    if (counts) {
        ca = vertex_cluster[a];
        cb = vertex_cluster[b];
        cc = vertex_cluster[c];
    }
    int64_t out[3];
    sg_simplify_corner_keys(counts, ca, cb, cc, f, out);
    corner_keys[3 * f] = out[0];
    corner_keys[3 * f + 1] = out[1];
    corner_keys[3 * f + 2] = out[2];
}

// ---- place ----------------------------------------------------------------------------------------------------------------------------
// the first position of a non-decreasing array whose element is >= x
__device__ __forceinline__ long simp_lower_int(const int* a, long n, long x) {
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = lo + (hi - lo) / 2;
        if (a[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
__device__ __forceinline__ long simp_lower_i64(const int64_t* a, long n, int64_t x) {
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = lo + (hi - lo) / 2;
        if (a[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// one wave per cluster; lane 0 holds the header's sums (the butterfly leaves s[0] of the header's tree there)
__global__ void __launch_bounds__(kSimpBlock) simp_place_kernel(SimpMesh m, const float* __restrict__ vertices,
                                                                const float* __restrict__ normals,
                                                                const int64_t* __restrict__ sorted_keys,
                                                                const int64_t* __restrict__ order,
                                                                const int* __restrict__ sorted_cluster,
                                                                const int64_t* __restrict__ corner_sorted, long C,
                                                                const float* __restrict__ origin, const float* __restrict__ cell,
                                                                int placement, float* __restrict__ cluster_vertices,
                                                                float* __restrict__ cluster_normals) {
    const long c = (long)blockIdx.x * (kSimpBlock / 64) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (c >= C) return;      // whole waves leave: no barrier follows
    const long v0 = simp_lower_int(sorted_cluster, m.V, c), v1 = simp_lower_int(sorted_cluster, m.V, c + 1);
    if (v0 >= v1) {          // the cluster numbers do not fit the count: written, never used
        if (lane < 3) cluster_vertices[c * 3 + lane] = cluster_normals[c * 3 + lane] = 0.0f;
        return;
    }
    const int64_t key = sorted_keys[v0];
    long s = sg_simplify_key_shape(key);
    s = s < 0 ? 0 : (s >= m.S ? m.S - 1 : s);
    const float o[3] = {origin[s * 3], origin[s * 3 + 1], origin[s * 3 + 2]};
    const float h = cell[s * 2];
    double p0[3];
    sg_simplify_centre(key, o, h, p0);

    double vsum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long base = v0; base < v1; base += SG_SIMPLIFY_TILE) {
        double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const long i = base + lane;
        if (i < v1) {
            const long v = order[i];
            if (v >= 0 && v < m.V) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    x[k] = vertices[v * 3 + k];
                    x[3 + k] = normals[v * 3 + k];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) vsum[k] += sg_wave_sum_d(x[k]);
    }

    double q[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (placement == SG_SIMPLIFY_QUADRIC) {
        const long n3 = 3 * m.F;
        const long c0 = simp_lower_i64(corner_sorted, n3, (int64_t)c << 31), c1 = simp_lower_i64(corner_sorted, n3, (int64_t)(c + 1) << 31);
        for (long base = c0; base < c1; base += SG_SIMPLIFY_TILE) {
            double x[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            const long i = base + lane;
            if (i < c1) {
                const long f = sg_simplify_corner_triangle(corner_sorted[i]);
                long ts, a, b, cc;
                if (f < m.F && simp_corners(m, f, ts, a, b, cc)) sg_simplify_quadric(vertices + a * 3, vertices + b * 3, vertices + cc * 3, p0, x);
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) q[k] += sg_wave_sum_d(x[k]);
        }
    }
    if (lane == 0) {
        const double count = (double)(v1 - v0);
        const double mean[3] = {vsum[0] / count, vsum[1] / count, vsum[2] / count};
        float x[3], nrm[3];
        sg_simplify_place(q, mean, p0, h, placement, x);
        sg_simplify_normal(vsum + 3, nrm);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            cluster_vertices[c * 3 + k] = x[k];
            cluster_normals[c * 3 + k] = nrm[k];
        }
    }
}

// ---- faces ----------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSimpBlock) simp_mark_kernel(SimpMesh m, const int* __restrict__ vertex_cluster, long C,
                                                               int* __restrict__ kept, int* named) {
    const long f = (long)blockIdx.x * kSimpBlock + threadIdx.x;
    if (f >= m.F) return;
    long s, a, b, c;
    int survives = 0;
    if (simp_corners(m, f, s, a, b, c)) {
        const long ca = vertex_cluster[a], cb = vertex_cluster[b], cc = vertex_cluster[c];
        if (ca != cb && cb != cc && ca != cc && ca >= 0 && cb >= 0 && cc >= 0 && ca < C && cb < C && cc < C) {
            survives = 1;
            named[ca] = 1;      // plain stores of one value: whoever comes last writes the same
            named[cb] = 1;
            named[cc] = 1;
        }
    }
    kept[f] = survives;
}

__global__ void __launch_bounds__(kSimpBlock) simp_emit_vertices_kernel(const uint32_t* __restrict__ cluster_vertices,
                                                                        const uint32_t* __restrict__ cluster_normals, long C,
                                                                        const int* __restrict__ named, const int* __restrict__ pos,
                                                                        uint32_t* __restrict__ out_vertices,
                                                                        uint32_t* __restrict__ out_normals, long max_verts) {
    const long c = (long)blockIdx.x * kSimpBlock + threadIdx.x;
    if (c >= C || !named[c]) return;
    const long o = pos[c];
    if (o >= max_verts) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out_vertices[o * 3 + k] = cluster_vertices[c * 3 + k];
        out_normals[o * 3 + k] = cluster_normals[c * 3 + k];
    }
}

__global__ void __launch_bounds__(kSimpBlock) simp_emit_faces_kernel(SimpMesh m, const int* __restrict__ vertex_cluster,
                                                                     const int* __restrict__ kept, const int* __restrict__ pos,
                                                                     const int* __restrict__ cluster_pos,
                                                                     const int64_t* __restrict__ new_vert_offsets,
                                                                     int64_t* __restrict__ out_faces, long max_tris) {
    const long f = (long)blockIdx.x * kSimpBlock + threadIdx.x;
    if (f >= m.F || !kept[f]) return;
    const long o = pos[f];
    long s, a, b, c;
    if (o >= max_tris || !simp_corners(m, f, s, a, b, c)) return;
    const long base = new_vert_offsets[s];
    out_faces[o * 3] = cluster_pos[vertex_cluster[a]] - base;
    out_faces[o * 3 + 1] = cluster_pos[vertex_cluster[b]] - base;
    out_faces[o * 3 + 2] = cluster_pos[vertex_cluster[c]] - base;
}

static inline long simp_blocks(long n) { return (n + kSimpBlock - 1) / kSimpBlock; }

// positions of the set flags and, per shape, the position of its first element; tot / off: simp_blocks(n) and simp_blocks(n) + 1 ints
static void simp_scan(const int* flag, long n, int* excl, int* tot, int* off, const int64_t* offsets, long S, int64_t* out,
                      hipStream_t stream) {
    const long nb = simp_blocks(n);
    if (nb) hipLaunchKernelGGL(simp_scan_totals_kernel, dim3((unsigned)nb), dim3(kSimpBlock), 0, stream, flag, n, tot);
    hipLaunchKernelGGL(simp_scan_blocks_kernel, dim3(1), dim3(1024), 0, stream, (const int*)tot, off, nb);
    if (nb) hipLaunchKernelGGL(simp_scan_positions_kernel, dim3((unsigned)nb), dim3(kSimpBlock), 0, stream, flag, n, (const int*)off, excl);
    hipLaunchKernelGGL(simp_offsets_kernel, dim3((unsigned)simp_blocks(S + 1)), dim3(kSimpBlock), 0, stream, offsets, S, n,
                       (const int*)excl, (const int*)(off + nb), out);
}

static bool simp_sizes(long S, long V, long F) {
    return S >= 1 && S < SG_SIMPLIFY_MAX_SHAPES && V >= 0 && F >= 0 && V <= 2147483647L && F <= 2147483647L;
}

struct SimpFaceScratch {
    int *named, *pos_c, *kept, *pos_t, *tot_c, *off_c, *tot_t, *off_t;
};
static SimpFaceScratch simp_face_scratch(void* workspace, long C, long F) {
    SimpFaceScratch k;
    k.named = (int*)workspace;
    k.pos_c = k.named + C;
    k.kept = k.pos_c + C;
    k.pos_t = k.kept + F;
    k.tot_c = k.pos_t + F;
    k.off_c = k.tot_c + simp_blocks(C);
    k.tot_t = k.off_c + simp_blocks(C) + 1;
    k.off_t = k.tot_t + simp_blocks(F);
    return k;
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_simplify_bounds(const float* vertices, const int64_t* vert_offsets, long S, long V, float* lo, float* hi, hipStream_t stream) {
    SG_CHECK_ARG(simp_sizes(S, V, 0));
    SG_CHECK_ARG(vert_offsets && lo && hi && (V == 0 || vertices));
    hipLaunchKernelGGL(simp_bounds_kernel, dim3((unsigned)S), dim3(kSimpBlock), 0, stream, vertices, vert_offsets, V, lo, hi);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_simplify_keys(const float* vertices, const int64_t* vert_offsets, long S, long V, const float* origin, const float* cell,
                     const int* cells, int64_t* keys, hipStream_t stream) {
    SG_CHECK_ARG(simp_sizes(S, V, 0));
    SG_CHECK_ARG(vert_offsets && origin && cell && cells && (V == 0 || (vertices && keys)));
    if (V) hipLaunchKernelGGL(simp_keys_kernel, dim3((unsigned)simp_blocks(V)), dim3(kSimpBlock), 0, stream, vertices, vert_offsets, S, V, origin, cell, cells, keys);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_simplify_count(const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                      const int64_t* keys, int* counts, hipStream_t stream) {
    SG_CHECK_ARG(simp_sizes(S, V, F));
    SG_CHECK_ARG(vert_offsets && tri_offsets && counts && (V == 0 || keys) && (F == 0 || faces));
    const SimpMesh m = {faces, vert_offsets, tri_offsets, S, V, F};
    hipLaunchKernelGGL(simp_zero_kernel, dim3((unsigned)simp_blocks(S)), dim3(kSimpBlock), 0, stream, counts, S);
    if (F) hipLaunchKernelGGL(simp_count_kernel, dim3((unsigned)simp_blocks(F)), dim3(kSimpBlock), 0, stream, m, keys, counts);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

size_t sg_simplify_clusters_workspace_bytes(long S, long V) {
    if (!simp_sizes(S, V, 0)) return 0;
    return (size_t)(2 * V + 2 * simp_blocks(V) + 2) * sizeof(int);
}

int sg_simplify_clusters(const int64_t* sorted_keys, const int64_t* order, const int64_t* vert_offsets, long S, long V,
                         int* sorted_cluster, int* vertex_cluster, int64_t* cluster_offsets, void* workspace, size_t workspace_bytes,
                         hipStream_t stream) {
    SG_CHECK_ARG(simp_sizes(S, V, 0));
    SG_CHECK_ARG(vert_offsets && cluster_offsets && workspace && (V == 0 || (sorted_keys && order && sorted_cluster && vertex_cluster)));
    if (workspace_bytes < sg_simplify_clusters_workspace_bytes(S, V)) SG_FAIL(SG_ERR_WORKSPACE, "sg_simplify_clusters: workspace too small");
    const long nb = simp_blocks(V);
    int* head = (int*)workspace;
    int* excl = head + V;
    int* tot = excl + V;
    int* off = tot + nb;
    if (nb) hipLaunchKernelGGL(simp_heads_kernel, dim3((unsigned)nb), dim3(kSimpBlock), 0, stream, sorted_keys, V, head);
    simp_scan(head, V, excl, tot, off, vert_offsets, S, cluster_offsets, stream);
    if (nb) hipLaunchKernelGGL(simp_number_kernel, dim3((unsigned)nb), dim3(kSimpBlock), 0, stream, order, V, (const int*)head, (const int*)excl, sorted_cluster, vertex_cluster);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_simplify_corners(const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                        const int* vertex_cluster, int64_t* corner_keys, hipStream_t stream) {
    SG_CHECK_ARG(simp_sizes(S, V, F));
    SG_CHECK_ARG(vert_offsets && tri_offsets && (V == 0 || vertex_cluster) && (F == 0 || (faces && corner_keys)));
    const SimpMesh m = {faces, vert_offsets, tri_offsets, S, V, F};
    if (F) hipLaunchKernelGGL(simp_corners_kernel, dim3((unsigned)simp_blocks(F)), dim3(kSimpBlock), 0, stream, m, vertex_cluster, corner_keys);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_simplify_place(const float* vertices, const float* normals, const int64_t* faces, const int64_t* vert_offsets,
                      const int64_t* tri_offsets, long S, long V, long F, const int64_t* sorted_keys, const int64_t* order,
                      const int* sorted_cluster, const int64_t* corner_sorted, long C, const float* origin, const float* cell,
                      int placement, float* cluster_vertices, float* cluster_normals, hipStream_t stream) {
    SG_CHECK_ARG(simp_sizes(S, V, F) && C >= 0 && C <= V);
    SG_CHECK_ARG(placement == SG_SIMPLIFY_QUADRIC || placement == SG_SIMPLIFY_MEAN);
    SG_CHECK_ARG(vert_offsets && tri_offsets && origin && cell);
    SG_CHECK_ARG(V == 0 || (vertices && normals && sorted_keys && order && sorted_cluster));
    SG_CHECK_ARG(F == 0 || placement == SG_SIMPLIFY_MEAN || (faces && corner_sorted));      // the mean reads no corner record
    SG_CHECK_ARG(C == 0 || (cluster_vertices && cluster_normals));
    const SimpMesh m = {faces, vert_offsets, tri_offsets, S, V, F};
    if (C) hipLaunchKernelGGL(simp_place_kernel, dim3((unsigned)((C + 3) / 4)), dim3(kSimpBlock), 0, stream, m, vertices, normals, sorted_keys, order, sorted_cluster, corner_sorted, C, origin, cell, placement, cluster_vertices, cluster_normals);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

size_t sg_simplify_faces_workspace_bytes(long S, long C, long F) {
    if (!simp_sizes(S, C, F)) return 0;
    return (size_t)(2 * C + 2 * F + 2 * simp_blocks(C) + 2 * simp_blocks(F) + 4) * sizeof(int);
}

int sg_simplify_faces_count(const int64_t* faces, const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F,
                            const int* vertex_cluster, const int64_t* cluster_offsets, long C, int64_t* new_vert_offsets,
                            int64_t* new_tri_offsets, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    SG_CHECK_ARG(simp_sizes(S, V, F) && C >= 0 && C <= V);
    SG_CHECK_ARG(vert_offsets && tri_offsets && cluster_offsets && new_vert_offsets && new_tri_offsets && workspace);
    SG_CHECK_ARG((V == 0 || vertex_cluster) && (F == 0 || faces));
    if (workspace_bytes < sg_simplify_faces_workspace_bytes(S, C, F)) SG_FAIL(SG_ERR_WORKSPACE, "sg_simplify_faces_count: workspace too small");
    const SimpFaceScratch k = simp_face_scratch(workspace, C, F);
    const SimpMesh m = {faces, vert_offsets, tri_offsets, S, V, F};
    if (C) hipLaunchKernelGGL(simp_zero_kernel, dim3((unsigned)simp_blocks(C)), dim3(kSimpBlock), 0, stream, k.named, C);
    if (F) hipLaunchKernelGGL(simp_mark_kernel, dim3((unsigned)simp_blocks(F)), dim3(kSimpBlock), 0, stream, m, vertex_cluster, C, k.kept, k.named);
    simp_scan(k.named, C, k.pos_c, k.tot_c, k.off_c, cluster_offsets, S, new_vert_offsets, stream);
    simp_scan(k.kept, F, k.pos_t, k.tot_t, k.off_t, tri_offsets, S, new_tri_offsets, stream);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_simplify_faces_emit(const float* cluster_vertices, const float* cluster_normals, const int64_t* faces,
                           const int64_t* vert_offsets, const int64_t* tri_offsets, long S, long V, long F, const int* vertex_cluster,
                           long C, const int64_t* new_vert_offsets, float* out_vertices, float* out_normals, int64_t* out_faces,
                           long max_verts, long max_tris, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    SG_CHECK_ARG(simp_sizes(S, V, F) && C >= 0 && C <= V && max_verts >= 0 && max_tris >= 0);
    SG_CHECK_ARG(vert_offsets && tri_offsets && new_vert_offsets && workspace);
    SG_CHECK_ARG((C == 0 || (cluster_vertices && cluster_normals)) && (V == 0 || vertex_cluster) && (F == 0 || faces));
    SG_CHECK_ARG((max_verts == 0 || (out_vertices && out_normals)) && (max_tris == 0 || out_faces));
    if (workspace_bytes < sg_simplify_faces_workspace_bytes(S, C, F)) SG_FAIL(SG_ERR_WORKSPACE, "sg_simplify_faces_emit: workspace too small");
    const SimpFaceScratch k = simp_face_scratch(workspace, C, F);
    const SimpMesh m = {faces, vert_offsets, tri_offsets, S, V, F};
    if (C && max_verts) hipLaunchKernelGGL(simp_emit_vertices_kernel, dim3((unsigned)simp_blocks(C)), dim3(kSimpBlock), 0, stream, (const uint32_t*)cluster_vertices, (const uint32_t*)cluster_normals, C, (const int*)k.named, (const int*)k.pos_c, (uint32_t*)out_vertices, (uint32_t*)out_normals, max_verts);
    if (F && max_tris) hipLaunchKernelGGL(simp_emit_faces_kernel, dim3((unsigned)simp_blocks(F)), dim3(kSimpBlock), 0, stream, m, vertex_cluster, (const int*)k.kept, (const int*)k.pos_t, (const int*)k.pos_c, new_vert_offsets, out_faces, max_tris);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

}  // extern "C"
