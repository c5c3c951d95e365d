// shapegan_amd/csrc/raymarch.hip — sphere tracing of SDFNet shapes (rendering/raymarching.py:render_image) on the device.
//
// The reference marches with a host loop: per step a gather of the active points, SDFNet.evaluate_in_batches, a clamp, a scatter
// and two boolean compactions (raymarching.py:104-122, :44-58 for the shadow rays), up to 1000 + 2 x 200 round trips per image.
// Here one launch is one step over a compacted list of active rays: raymarch_step_kernel stages the ray positions into the
// MLP tile of sdfnet_tile.h (the same eight layers, the same MFMA code as sg_sdfnet_fwd), and its epilogue moves the ray,
// classifies it (hit / miss / survives) and appends survivors to the next list (one global atomic per wave and shape).  A
// point's MLP arithmetic does not depend on its tile, so the order in which the atomics compact the lists changes no result:
// renders are bit-reproducible.
//
// Rays live in segments (one per image, or per image and kind for the shadow rays); a segment's active list sits at
// active[buf][seg_off[seg] ...] and its count at counts[iter % 3][seg].  Step `iter` reads list iter & 1 and counts iter % 3,
// appends to list / counts (iter + 1), and zeroes counts (iter + 2) for the step after it.  A segment whose previous step left
// fewer than two rays is finished (raymarching.py:119-120, :57-58): its remaining ray is marked as a hit and the segment stays
// empty, so launches behind the last live segment are no-ops and a batch of images gives every image what it gets alone.
#include "common.h"
#include "sdfnet_tile.h"
#include "../../include/shapegan_hip.h"

// positions, directions and pixels are compared with the twin: no contraction of a * b + c into one rounding.  The pragma stays BELOW
// the sdfnet_tile.h include: above it, it would change the MLP arithmetic of raymarch_step_kernel.
#pragma clang fp contract(off)
#include "raymarch_core.h"  // the per-ray and per-pixel arithmetic, shared with the twin

namespace sg {

constexpr int kMarchTile = 64;
constexpr int kMaxSegments = 256;
constexpr int kScanBlock = 256;
static_assert(kScanBlock == 256, "sg_block_exclusive_256 scans four waves");

struct MarchArgs {
    float* pos;               // [nrays][3]
    const float* dir;         // [dir_period or nrays][3]
    long dir_period;          // > 0: ray r uses dir[r % dir_period] (one camera for all images)
    unsigned char* status;    // [nrays]: 1 = hit (primary) / shadowed (shadow rays)
    int* active;              // [2][nrays]
    long nrays;
    int* counts;              // [3][nseg]
    const int64_t* seg_off;   // [nseg + 1]
    int nseg, nshapes;        // segment s marches image s % nshapes
    long iter;
    float clampv, threshold, offset, radius0, radius1;   // radius0: segments < nshapes, radius1: the others
    int shadow;               // miss test: pos.y > radius (shadow rays) or |pos| > radius (camera rays)
    unsigned long long* evals;
};

// the tile's points are active rays: rid / rseg (LDS) name the ray and segment of point p0 + i
struct MarchIo {
    const MarchArgs* m;
    long p0;
    const int* rid;
    const int* rseg;
    __device__ __forceinline__ float coord(const SdfFwdArgs&, long gp, int c) const { return m->pos[(long)rid[gp - p0] * 3 + c]; }
    __device__ __forceinline__ bool ragged(const SdfFwdArgs&) const { return true; }
    __device__ __forceinline__ int shape(const SdfFwdArgs&, long gp) const { return rseg[gp - p0] % m->nshapes; }
    __device__ void store(const SdfFwdArgs& a, long gp, float v) const {
        // raymarching.py:106-117 (:47-55): sdf = clamp(tanh(v) + offset, -c, c); points += dir * sdf; hit / miss
        const int lane = threadIdx.x;
        const int ray = rid[lane], seg = rseg[lane];
        bool surv = false;
        if (gp < a.N) {
            float s = tanhf(v) + m->offset;
            s = fminf(fmaxf(s, -m->clampv), m->clampv);
            const long di = m->dir_period > 0 ? ray % m->dir_period : ray;
            float* p = m->pos + (long)ray * 3;
            sg_rm_move(p, m->dir + di * 3, s);
            if (sg_rm_hit(s, m->threshold)) m->status[ray] = 1;
            else surv = !sg_rm_left(p, seg < m->nshapes ? m->radius0 : m->radius1, m->shadow);
        }
        // append the survivors: per distinct segment in the wave one atomic (ballot + mbcnt)
        int* next = m->active + ((m->iter + 1) & 1) * m->nrays;
        int* cw = m->counts + ((m->iter + 1) % 3) * m->nseg;
        unsigned long long left = __ballot(surv);
        while (left) {
            const int l = __builtin_ctzll(left);
            const int s0 = __shfl(seg, l, 64);
            const bool mine = surv && seg == s0;
            const unsigned long long mm = __ballot(mine);
            int base = 0;
            if (lane == l) base = atomicAdd(cw + s0, (int)__popcll(mm));
            base = __shfl(base, l, 64);
            const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mm, 0u));
            if (mine) next[m->seg_off[s0] + base + rank] = ray;
            left &= ~mm;
        }
    }
};

// One march step: workgroup b takes rays [64 b, 64 b + 64) of the live segments' lists laid end to end.  The count is read here, on
// the device; the grid only has to cover it (sg_raymarch_steps: max_rays), the workgroups beyond it return at once.  (A
// persistent form — 512 workgroups looping over the tiles — keeps the tile's loop-invariant addresses live across the whole MLP
// and spills 63 VGPRs at the 128 of two workgroups per CU; one tile per workgroup needs 119 and spills none.)
__global__ void __launch_bounds__(512, 4) raymarch_step_kernel(SdfFwdArgs a, MarchArgs m) {
    __shared__ int s_pref[kMaxSegments + 1];
    __shared__ int s_rid[kMarchTile], s_rseg[kMarchTile];
    const int tid = threadIdx.x;
    const int* cr = m.counts + (m.iter % 3) * m.nseg;
    const int* cur = m.active + (m.iter & 1) * m.nrays;
    if (tid == 0) {
        int acc = 0;
        for (int s = 0; s < m.nseg; ++s) {
            s_pref[s] = acc;
            const int c = cr[s];
            acc += (m.iter > 0 && c < 2) ? 0 : c;
        }
        s_pref[m.nseg] = acc;
    }
    if (blockIdx.x == 0 && tid < m.nseg) {
        m.counts[((m.iter + 2) % 3) * m.nseg + tid] = 0;
        if (m.iter > 0 && cr[tid] == 1) m.status[cur[m.seg_off[tid]]] = 1;   // fewer than 2 left: the rest is a hit
    }
    __syncthreads();
    const int total = s_pref[m.nseg];
    if (blockIdx.x == 0 && tid == 0 && m.evals && total > 0) atomicAdd(m.evals, (unsigned long long)total);
    const long p0 = (long)blockIdx.x * kMarchTile;
    if (p0 >= total) return;
    SdfFwdArgs at = a;
    at.N = total;
    {
        if (tid < kMarchTile) {
            const long gp = p0 + tid;
            int seg = 0, ray = 0;
            if (gp < total) {
                int lo = 0, hi = m.nseg - 1;   // the last segment that starts at or before gp (it is not empty)
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (s_pref[mid] <= gp) lo = mid;
                    else hi = mid - 1;
                }
                seg = lo;
                ray = cur[m.seg_off[seg] + (gp - s_pref[seg])];
            }
            s_rid[tid] = ray;
            s_rseg[tid] = seg;
        }
        __syncthreads();
        const MarchIo io{&m, p0, s_rid, s_rseg};
        sdfnet_fwd_tile<kMarchTile, true, false, false>(at, p0, io);
    }
}

// the rays still active after the last step are hits (raymarching.py:124, :60)
__global__ void __launch_bounds__(256) raymarch_finish_kernel(MarchArgs m) {
    const int seg = blockIdx.y;
    const int c = m.counts[(m.iter % 3) * m.nseg + seg];
    const int* cur = m.active + (m.iter & 1) * m.nrays + m.seg_off[seg];
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < c; k += (long)gridDim.x * 256) m.status[cur[k]] = 1;
}

// ---- camera rays (raymarching.py:65-102) ----
struct Camera {
    double v[13], c;   // position, right, up, forward, focal length; c = |position|^2 - radius^2
    float posf[3];
};

__global__ void __launch_bounds__(256) raymarch_rays_kernel(Camera cam, int W, long M, int S, float* __restrict__ dir,
                                                            float* __restrict__ pos, unsigned char* __restrict__ status,
                                                            int* __restrict__ active, int* __restrict__ counts) {
    const long pix = (long)blockIdx.x * 256 + threadIdx.x;
    bool inside = false;
    float p[3] = {cam.posf[0], cam.posf[1], cam.posf[2]};
    if (pix < M) {
        float d[3];
        inside = sg_rm_camera_ray(cam.v, cam.c, W, pix, d, p);
#pragma unroll
        for (int c = 0; c < 3; ++c) dir[pix * 3 + c] = d[c];
    }
    const unsigned long long mm = __ballot(inside);
    const int lane = threadIdx.x & 63;
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mm, 0u));
    const int first = mm ? __builtin_ctzll(mm) : 0;
    for (int s = 0; s < S; ++s) {
        if (pix < M) {
            const long r = (long)s * M + pix;
#pragma unroll
            for (int c = 0; c < 3; ++c) pos[r * 3 + c] = p[c];
            status[r] = 0;
        }
        if (mm) {
            int base = 0;
            if (lane == first) base = atomicAdd(counts + s, (int)__popcll(mm));
            base = __shfl(base, first, 64);
            if (inside) active[(long)s * M + base + rank] = (int)(s * M + pix);
        }
    }
}

// ---- hits, ground plane, ground rays (raymarching.py:126-130, :159-165) ----
struct Scene {
    unsigned char* status;   // [S][M]
    const float* pos;        // [S][M][3]
    const float* dir;        // [M][3]
    long M;
    int S;
    int cutoff;              // vertical_cutoff given
    float vcut;
    const float* ground;     // [S]: the ground plane (min y of the hits)
    const int64_t* hit_off;  // [S + 1]
};

// the ground point of a non-hit pixel looking down, if image s has a ground plane at all (without a hit the image stays white)
__device__ __forceinline__ bool ground_point(const Scene& sc, int s, long pix, float q[3]) {
    if (sc.hit_off[s + 1] == sc.hit_off[s]) return false;
    const long r = (long)s * sc.M + pix;
    return sg_rm_ground_point(sc.status[r], sc.pos + r * 3, sc.dir + pix * 3, sc.ground[s], q);
}

// pass 0: vertical cutoff (raymarching.py:126-128), hits per block and the block's minimum hit y; pass 1: ground rays per block
__global__ void __launch_bounds__(kScanBlock) raymarch_count_kernel(Scene sc, int pass, int* __restrict__ block_tot,
                                                                     int* __restrict__ block_min) {
    __shared__ int lds[kScanBlock / 64];
    const int s = blockIdx.y;
    const long pix = (long)blockIdx.x * kScanBlock + threadIdx.x;
    const long blocks = gridDim.x;
    int x = 0, key = 0x7fffffff;
    if (pix < sc.M) {
        const long r = (long)s * sc.M + pix;
        if (pass == 0) {
            if (sc.status[r]) {
                const float y = sc.pos[r * 3 + 1];
                if (sc.cutoff && (y > sc.vcut || y < -sc.vcut)) sc.status[r] = 0;
                else {
                    x = 1;
                    key = sg_float_key(y);
                }
            }
        } else {
            float q[3];
            x = ground_point(sc, s, pix, q) ? 1 : 0;
        }
    }
    int tot;
    sg_block_exclusive_256(x, lds, tot);
    if (pass == 0) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) key = min(key, __shfl_xor(key, off, 64));
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = key;
        __syncthreads();
        if (threadIdx.x == 0) {
            int k = lds[0];
            for (int w = 1; w < kScanBlock / 64; ++w) k = min(k, lds[w]);
            block_min[s * blocks + blockIdx.x] = k;
        }
    }
    if (threadIdx.x == 0) block_tot[s * blocks + blockIdx.x] = tot;
}

// one workgroup of 1024: exclusive offsets of the S x blocks totals, per-image offsets [S+1]; with block_min also the per-image
// minimum (the ground plane)
__global__ void __launch_bounds__(1024) raymarch_scan_kernel(const int* __restrict__ block_tot, int* __restrict__ block_off, long blocks,
                                                             int S, int64_t* __restrict__ offsets, const int* __restrict__ block_min,
                                                             float* __restrict__ ground) {
    __shared__ long long part[16];
    __shared__ int smin[kMaxSegments];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long n = blocks * S;
    const long per = (n + 1023) / 1024;
    const long i0 = threadIdx.x * per, i1 = i0 + per < n ? i0 + per : n;
    if (block_min)
        for (int s = threadIdx.x; s < S; s += 1024) smin[s] = 0x7fffffff;
    long long sv = 0;
    for (long i = i0; i < i1; ++i) sv += block_tot[i];
    long long iv = sv;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long y = __shfl_up(iv, off, 64);
        if (lane >= off) iv += y;
    }
    if (lane == 63) part[wave] = iv;
    __syncthreads();
    long long bv = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        bv += w < wave ? part[w] : 0;
        all += part[w];
    }
    long long rv = bv + iv - sv;
    int key = 0x7fffffff, ks = -1;
    for (long i = i0; i < i1; ++i) {
        const int s = (int)(i / blocks);
        if (i % blocks == 0) offsets[s] = rv;
        block_off[i] = (int)(rv - (long long)0);   // global offset (< 2^31, checked on the host)
        rv += block_tot[i];
        if (block_min) {
            if (s != ks) {
                if (ks >= 0) atomicMin(smin + ks, key);
                ks = s;
                key = 0x7fffffff;
            }
            key = min(key, block_min[i]);
        }
    }
    if (block_min && ks >= 0) atomicMin(smin + ks, key);
    if (threadIdx.x == 0) offsets[S] = all;
    if (block_min) {
        __syncthreads();
        // (an image without hits keeps the initial key, a NaN pattern: the minimum over nothing is +inf)
        for (int s = threadIdx.x; s < S; s += 1024) ground[s] = smin[s] == 0x7fffffff ? INFINITY : sg_key_float(smin[s]);
    }
}

struct Emit {
    const int* hit_boff;        // block offsets of the hits (global)
    const int* gnd_boff;        // ... of the ground rays (global, behind all hits)
    const int64_t* gnd_off;     // [S + 1]
    double light[3];
    float* hit_pos;             // [H][3]
    int* hit_sid;               // [H]
    int* slot;                  // [S][M]: hit index, -2 - ground index, or -1
    float* spos;                // [H + G][3]: shadow ray starts
    float* sdir;                // [H + G][3]
    int* sactive;               // [2][H + G]
    int* scounts;               // [3][2S]
    int64_t* sseg;              // [2S + 1]
};

__global__ void __launch_bounds__(kScanBlock) raymarch_emit_kernel(Scene sc, Emit e) {
    __shared__ int lds[kScanBlock / 64];
    const int s = blockIdx.y;
    const long pix = (long)blockIdx.x * kScanBlock + threadIdx.x;
    const long bi = (long)s * gridDim.x + blockIdx.x;
    const long H = sc.hit_off[sc.S];
    const long r = (long)s * sc.M + pix;
    bool hit = false, gnd = false;
    float q[3];
    if (pix < sc.M) {
        hit = sc.status[r] != 0;
        if (!hit) gnd = ground_point(sc, s, pix, q);
    }
    int tot;
    const int hr = sg_block_exclusive_256(hit ? 1 : 0, lds, tot);
    const int gr = sg_block_exclusive_256(gnd ? 1 : 0, lds, tot);
    if (pix < sc.M) {
        if (hit) {
            const long h = e.hit_boff[bi] + hr;
#pragma unroll
            for (int c = 0; c < 3; ++c) q[c] = e.hit_pos[h * 3 + c] = sc.pos[r * 3 + c];
            e.hit_sid[h] = s;
            e.slot[r] = (int)h;
            sg_rm_shadow_ray(e.light, q, e.sdir + h * 3, e.spos + h * 3);
            e.sactive[h] = (int)h;
        } else if (gnd) {
            const long g = e.gnd_boff[bi] + gr;
            e.slot[r] = -2 - (int)g;
            sg_rm_shadow_ray(e.light, q, e.sdir + (H + g) * 3, e.spos + (H + g) * 3);
            e.sactive[H + g] = (int)(H + g);
        } else {
            e.slot[r] = -1;
        }
    }
    // the shadow segments: the hits of image s, then its ground rays (two get_shadows calls, raymarching.py:136,165)
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        for (int j = threadIdx.x; j <= 2 * sc.S; j += kScanBlock) {
            const long o = j <= sc.S ? sc.hit_off[j] : H + e.gnd_off[j - sc.S];
            e.sseg[j] = o;
            if (j < 2 * sc.S) {
                const long o1 = j + 1 <= sc.S ? sc.hit_off[j + 1] : H + e.gnd_off[j + 1 - sc.S];
                e.scounts[j] = (int)(o1 - o);
                e.scounts[2 * sc.S + j] = 0;
                e.scounts[4 * sc.S + j] = 0;
            }
        }
    }
}

// ---- shading ----
struct Shade {
    const int* slot;
    const float* hit_pos;
    const float* grad;            // [H][3] d sdf / d p (normalised here)
    const unsigned char* shadow;  // [H + G]
    const float* dir;
    long M, H;
    int S;
    double light[3], color[3];
    unsigned char* image;         // [S][M][3]
};

__global__ void __launch_bounds__(256) raymarch_shade_kernel(Shade sh) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= (long)sh.S * sh.M) return;
    sg_rm_shade(sh.slot[r], sh.dir + (r % sh.M) * 3, sh.hit_pos, sh.grad, sh.shadow, sh.H, sh.light, sh.color, sh.image + r * 3);
}

static MarchArgs march_args(float* pos, const float* dir, long dir_period, unsigned char* status, int* active, long nrays,
                            int* counts, const int64_t* seg_off, long nseg, long nshapes, long iter) {
    MarchArgs m{};
    m.pos = pos;
    m.dir = dir;
    m.dir_period = dir_period;
    m.status = status;
    m.active = active;
    m.nrays = nrays;
    m.counts = counts;
    m.seg_off = seg_off;
    m.nseg = (int)nseg;
    m.nshapes = (int)nshapes;
    m.iter = iter;
    return m;
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_raymarch_rays(const double* camera, int width, long nshapes, double radius, float* dir, float* pos, unsigned char* status,
                     int* active, int* counts, hipStream_t stream) {
    SG_CHECK_ARG(camera && dir && pos && status && active && counts && width > 0 && nshapes > 0 && radius > 0.0);
    const long M = (long)width * width;
    SG_CHECK_ARG(nshapes * M < (1L << 31));
    Camera cam;
    for (int i = 0; i < 13; ++i) cam.v[i] = camera[i];
    for (int c = 0; c < 3; ++c) cam.posf[c] = (float)camera[c];
    cam.c = (camera[0] * camera[0] + camera[1] * camera[1] + camera[2] * camera[2]) - radius * radius;
    hipLaunchKernelGGL(raymarch_rays_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream, cam, width, M, (int)nshapes, dir,
                       pos, status, active, counts);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_raymarch_steps(const float* packed, const float* zb1, const float* zb5, float* pos, const float* dir, long dir_period,
                      unsigned char* status, int* active, long nrays, int* counts, const int64_t* seg_off, long nseg, long nshapes,
                      long max_rays, long first_iter, int steps, float clampv, float threshold, float sdf_offset, float radius0, float radius1,
                      int shadow, unsigned long long* evals, hipStream_t stream) {
    SG_CHECK_ARG(packed && zb1 && zb5 && pos && dir && status && active && counts && seg_off && steps >= 0 && first_iter >= 0);
    SG_CHECK_ARG(nseg > 0 && nseg <= kMaxSegments && nshapes > 0 && nseg % nshapes == 0 && nrays > 0 && nrays < (1L << 31));
    SG_CHECK_ARG(max_rays >= 0 && max_rays <= nrays);
    if (max_rays == 0 || steps == 0) return SG_OK;
    SdfFwdArgs a{};
    a.packed = packed;
    a.lay = make_layout(3);
    a.zb1 = zb1;
    a.zb5 = zb5;
    a.pps = 1;
    const size_t lds = sdf_fwd_lds_bytes(kMarchTile, a.lay.KUp);
    static SgPerDeviceOnce once;
    if (const int rc = sg_reserve_lds(once, raymarch_step_kernel, lds, "sg_raymarch_steps")) return rc;
    MarchArgs m = march_args(pos, dir, dir_period, status, active, nrays, counts, seg_off, nseg, nshapes, first_iter);
    m.clampv = clampv;
    m.threshold = threshold;
    m.offset = sdf_offset;
    m.radius0 = radius0;
    m.radius1 = radius1;
    m.shadow = shadow;
    m.evals = evals;
    for (int i = 0; i < steps; ++i) {
        m.iter = first_iter + i;
        hipLaunchKernelGGL(raymarch_step_kernel, dim3((unsigned)((max_rays + kMarchTile - 1) / kMarchTile)), dim3(512), lds, stream, a, m);
    }
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_raymarch_finish(unsigned char* status, const int* active, long nrays, const int* counts, const int64_t* seg_off, long nseg,
                       long iter, hipStream_t stream) {
    SG_CHECK_ARG(status && active && counts && seg_off && nseg > 0 && nseg <= kMaxSegments && iter >= 0 && nrays > 0);
    MarchArgs m = march_args(nullptr, nullptr, 0, status, const_cast<int*>(active), nrays, const_cast<int*>(counts), seg_off, nseg,
                             nseg, iter);
    hipLaunchKernelGGL(raymarch_finish_kernel, dim3(64, (unsigned)nseg), dim3(256), 0, stream, m);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

size_t sg_raymarch_workspace_bytes(long M, long nshapes) {
    if (M <= 0 || nshapes <= 0) return 0;
    const long blocks = (M + kScanBlock - 1) / kScanBlock;
    return (size_t)(5 * blocks * nshapes) * sizeof(int);
}

int sg_raymarch_classify(unsigned char* status, const float* pos, const float* dir, long M, long nshapes, int use_cutoff,
                         float vertical_cutoff, float* ground, int64_t* hit_off, int64_t* gnd_off, void* workspace,
                         size_t workspace_bytes, hipStream_t stream) {
    SG_CHECK_ARG(status && pos && dir && ground && hit_off && gnd_off && workspace && M > 0 && nshapes > 0);
    SG_CHECK_ARG(2 * nshapes <= kMaxSegments && nshapes * M < (1L << 31));
    if (workspace_bytes < sg_raymarch_workspace_bytes(M, nshapes)) SG_FAIL(SG_ERR_WORKSPACE, "sg_raymarch_classify: workspace too small");
    const long blocks = (M + kScanBlock - 1) / kScanBlock;
    int* w = (int*)workspace;
    int *htot = w, *hoff = w + blocks * nshapes, *hmin = w + 2 * blocks * nshapes, *gtot = w + 3 * blocks * nshapes,
        *goff = w + 4 * blocks * nshapes;
    Scene sc{status, pos, dir, M, (int)nshapes, use_cutoff, vertical_cutoff, ground, hit_off};
    const dim3 grid((unsigned)blocks, (unsigned)nshapes);
    hipLaunchKernelGGL(raymarch_count_kernel, grid, dim3(kScanBlock), 0, stream, sc, 0, htot, hmin);
    hipLaunchKernelGGL(raymarch_scan_kernel, dim3(1), dim3(1024), 0, stream, htot, hoff, blocks, (int)nshapes, hit_off,
                       (const int*)hmin, ground);
    hipLaunchKernelGGL(raymarch_count_kernel, grid, dim3(kScanBlock), 0, stream, sc, 1, gtot, (int*)nullptr);
    hipLaunchKernelGGL(raymarch_scan_kernel, dim3(1), dim3(1024), 0, stream, gtot, goff, blocks, (int)nshapes, gnd_off,
                       (const int*)nullptr, (float*)nullptr);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_raymarch_emit(const unsigned char* status, const float* pos, const float* dir, long M, long nshapes, const float* ground,
                     const int64_t* hit_off, const int64_t* gnd_off, const double* light, float* hit_pos, int* hit_sid, int* slot,
                     float* shadow_pos, float* shadow_dir, int* shadow_active, int* shadow_counts, int64_t* shadow_seg,
                     const void* workspace, size_t workspace_bytes, hipStream_t stream) {
    SG_CHECK_ARG(status && pos && dir && ground && hit_off && gnd_off && light && slot && shadow_counts && shadow_seg && workspace);
    SG_CHECK_ARG(M > 0 && nshapes > 0 && 2 * nshapes <= kMaxSegments && nshapes * M < (1L << 31));
    if (workspace_bytes < sg_raymarch_workspace_bytes(M, nshapes)) SG_FAIL(SG_ERR_WORKSPACE, "sg_raymarch_emit: workspace too small");
    const long blocks = (M + kScanBlock - 1) / kScanBlock;
    const int* w = (const int*)workspace;
    Scene sc{const_cast<unsigned char*>(status), pos, dir, M, (int)nshapes, 0, 0.f, ground, hit_off};
    Emit e{};
    e.hit_boff = w + blocks * nshapes;
    e.gnd_boff = w + 4 * blocks * nshapes;
    e.gnd_off = gnd_off;
    for (int c = 0; c < 3; ++c) e.light[c] = light[c];
    e.hit_pos = hit_pos;
    e.hit_sid = hit_sid;
    e.slot = slot;
    e.spos = shadow_pos;
    e.sdir = shadow_dir;
    e.sactive = shadow_active;
    e.scounts = shadow_counts;
    e.sseg = shadow_seg;
    hipLaunchKernelGGL(raymarch_emit_kernel, dim3((unsigned)blocks, (unsigned)nshapes), dim3(kScanBlock), 0, stream, sc, e);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_raymarch_shade(const int* slot, const float* hit_pos, const float* grad, const unsigned char* shadow, const float* dir, long M,
                      long nshapes, long nhits, const double* light, const double* color, unsigned char* image, hipStream_t stream) {
    SG_CHECK_ARG(slot && dir && light && color && image && M > 0 && nshapes > 0 && nhits >= 0);
    SG_CHECK_ARG(nhits == 0 || (hit_pos && grad && shadow));
    Shade sh{};
    sh.slot = slot;
    sh.hit_pos = hit_pos;
    sh.grad = grad;
    sh.shadow = shadow;
    sh.dir = dir;
    sh.M = M;
    sh.H = nhits;
    sh.S = (int)nshapes;
    for (int c = 0; c < 3; ++c) {
        sh.light[c] = light[c];
        sh.color[c] = color[c];
    }
    sh.image = image;
    const long n = nshapes * M;
    hipLaunchKernelGGL(raymarch_shade_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, sh);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

}  // extern "C"
