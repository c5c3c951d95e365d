// shapegan_amd/csrc/emd.hip — earth mover's distance between point clouds (K15): Bertsekas' forward auction with eps-scaling.
//
// One workgroup of 256 lanes per pair of clouds; everything the auction touches between its first and its last round sits in LDS
// (62 KB at any P: the points of b as three planes, the prices, one packed (bid, bidder) word and the owner per object, two lists
// of unassigned bidders) or in registers.  The costs are recomputed in every round from the coordinates: a 2048^2 table fits
// nowhere, and a cost is 3 subtractions, 3 multiply-adds, one square root and one division.
//
// A round has two halves with a barrier between them:
//   bid      every entry of the current list of unassigned bidders finds its best and second-best object and bids with ONE
//            ds_max_u64 on the object's word ((bid << 32) | (65535 - bidder): the highest bid, the lowest bidder of a tie).  Prices
//            only rise and a bid is above the price, so the word of an earlier round never has to be cleared.
//   resolve  an entry whose word stands has won: it writes price and owner and appends the owner it displaced to the NEXT list;
//            an entry that lost appends itself.  The order inside a list is the order the LDS counter hands out slots in; no result
//            depends on it (include/shapegan_hip.h: every bid of a round is computed from the prices at its start).
// All the work of a round is proportional to the number of bidders, and there are three forms of the first half:
//   lanes    one lane per entry (up to 8 entries per lane at 2048 bidders, scanned together so that a point of b read from LDS, a
//            broadcast, serves all of them): the early rounds of a phase;
//   waves    one wave per entry, 64 lanes x P/64 objects and a butterfly of the (best, index, second) triples: the long tail of
//            rounds with a handful of bidders, where one lane per bidder would leave the workgroup idle behind one lane's 2048
//            steps;
//   block    the whole workgroup per entry, 256 lanes x P/256 objects, the four waves' triples merged through LDS: rounds with one
//            or two bidders, which are most rounds (a price war between two bidders for one object is a run of them).
// DESIGN 3.11 has the shares of the rounds and the measurements behind the switch points.
#include "common.h"
#include "../../include/shapegan_hip.h"

// the costs are compared bit for bit with the twin: d2 is K13's, with its two explicit fmaf
#pragma clang fp contract(off)
#include "pointcloud_core.h"   // distance, integer cost, unit and the argument predicate, shared with the twin

namespace sg {

constexpr int kEmdBlock = 256;
constexpr int kEmdWaves = kEmdBlock / 64;
constexpr int kEmdMaxP = SG_EMD_MAX_POINTS;
constexpr int kEmdSlots = kEmdMaxP / kEmdBlock;       // entries per lane when every point bids
constexpr int kEmdWaveScanMax = 64 * kEmdWaves;       // one lane of the wave keeps each of its entries until the resolve half
constexpr int kEmdWaveScanDefault = 160;
constexpr int kEmdBlockScanMax = 16;                  // sh.red holds the partial triples of that many entries
constexpr int kEmdBlockScanDefault = 2;
constexpr int kEmdNone = 0xFFFF;
constexpr int kEmdMin = -2147483647 - 1;              // below every value -k - p (k <= 2^22, p < 2^28)

struct EmdShared {
    float b[3][kEmdMaxP];
    int price[kEmdMaxP];
    unsigned long long bid[kEmdMaxP];
    unsigned short owner[kEmdMaxP];
    unsigned short list[2][kEmdMaxP];
    double red[kEmdBlock];
    int cnt[2];
    int kmax;
    int too_small;
};
static_assert(sizeof(EmdShared) <= 64 * 1024, "static LDS");
static_assert(kEmdBlockScanMax * kEmdWaves * 3 * sizeof(int) <= sizeof(double) * kEmdBlock, "the partial triples fit sh.red");

// (w1, j1, w2) of the header; objects arrive in increasing j, the strict comparison keeps the lowest j of a tie
struct EmdTop {
    int w1, j1, w2;
    __device__ __forceinline__ void take(int v, int j) {
        const bool gt = v > w1;
        w2 = gt ? w1 : (v > w2 ? v : w2);
        j1 = gt ? j : j1;
        w1 = gt ? v : w1;
    }
};

// the triple of the union of two sets of objects; (w1, j1) is a strict order, so the result does not depend on the grouping
__device__ __forceinline__ void emd_merge(EmdTop& top, const EmdTop& o) {
    const bool mine = top.w1 > o.w1 || (top.w1 == o.w1 && top.j1 < o.j1);
    const int other_best = mine ? o.w1 : top.w1, kept_second = mine ? top.w2 : o.w2;
    top.w1 = mine ? top.w1 : o.w1;
    top.j1 = mine ? top.j1 : o.j1;
    top.w2 = other_best > kept_second ? other_best : kept_second;
}

__device__ __forceinline__ void emd_wave_reduce(EmdTop& top) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        EmdTop o;
        o.w1 = __shfl_xor(top.w1, off, 64);
        o.j1 = __shfl_xor(top.j1, off, 64);
        o.w2 = __shfl_xor(top.w2, off, 64);
        emd_merge(top, o);
    }
}

__device__ __forceinline__ unsigned long long emd_word(const EmdShared& sh, const EmdTop& t, int e, int bidder) {
    const int w2 = t.w2 == kEmdMin ? t.w1 : t.w2;      // P = 1
    return ((unsigned long long)(unsigned)(sh.price[t.j1] + (t.w1 - w2) + e) << 32) | (unsigned)(kEmdNone - bidder);
}

// one lane per entry: this lane's entries are tid, tid + 256, .. < n; M = the slots scanned together
template <int M>
__device__ __forceinline__ void emd_bid_lanes(EmdShared& sh, const float* __restrict__ a, int P, float u, int e, int n,
                                              const unsigned short* list, int (&ei)[kEmdSlots], int (&ej)[kEmdSlots],
                                              unsigned long long (&ew)[kEmdSlots]) {
    const int tid = threadIdx.x;
    float ax[M], ay[M], az[M];
    EmdTop top[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int ent = tid + m * kEmdBlock;
        ei[m] = list[ent < n ? ent : 0];               // a slot beyond the list computes on its first entry and bids nothing
        ax[m] = a[ei[m] * 3];
        ay[m] = a[ei[m] * 3 + 1];
        az[m] = a[ei[m] * 3 + 2];
        top[m].w1 = top[m].w2 = kEmdMin;
        top[m].j1 = 0;
    }
    const int P4 = P & ~3;
    for (int q = 0; q < P4; q += 4) {
        const f32x4 bx = *(const f32x4*)&sh.b[0][q], by = *(const f32x4*)&sh.b[1][q], bz = *(const f32x4*)&sh.b[2][q];
        const int4 pr = *(const int4*)&sh.price[q];
        const int prs[4] = {pr.x, pr.y, pr.z, pr.w};
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int m = 0; m < M; ++m) top[m].take(-sg_emd_cost(sg_emd_dist(ax[m], ay[m], az[m], bx[t], by[t], bz[t]), u) - prs[t], q + t);
    }
    for (int q = P4; q < P; ++q) {
        const float bx = sh.b[0][q], by = sh.b[1][q], bz = sh.b[2][q];
        const int pr = sh.price[q];
#pragma unroll
        for (int m = 0; m < M; ++m) top[m].take(-sg_emd_cost(sg_emd_dist(ax[m], ay[m], az[m], bx, by, bz), u) - pr, q);
    }
#pragma unroll
    for (int m = 0; m < M; ++m)
        if (tid + m * kEmdBlock < n) {
            ej[m] = top[m].j1;
            ew[m] = emd_word(sh, top[m], e, ei[m]);
            atomicMax(&sh.bid[ej[m]], ew[m]);
        }
}

// one wave per entry: wave w takes the entries w, w + 4, ..; lane t of the wave keeps its t-th entry in slot 0
__device__ __forceinline__ void emd_bid_waves(EmdShared& sh, const float* __restrict__ a, int P, float u, int e, int n,
                                              const unsigned short* list, int& ei, int& ej, unsigned long long& ew) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int t = 0;
    for (int ent = wave; ent < n; ent += kEmdWaves, ++t) {
        const int i = __builtin_amdgcn_readfirstlane((int)list[ent]);
        const float ax = a[i * 3], ay = a[i * 3 + 1], az = a[i * 3 + 2];
        EmdTop top;
        top.w1 = top.w2 = kEmdMin;
        top.j1 = kEmdMaxP + lane;                      // a lane without objects loses every merge
        for (int j = lane; j < P; j += 64) top.take(-sg_emd_cost(sg_emd_dist(ax, ay, az, sh.b[0][j], sh.b[1][j], sh.b[2][j]), u) - sh.price[j], j);
        emd_wave_reduce(top);
        if (lane == t) {
            ei = i;
            ej = top.j1;
            ew = emd_word(sh, top, e, i);
        }
    }
    if (lane < t) atomicMax(&sh.bid[ej], ew);
}

// the whole workgroup per entry, one entry after the other: 256 lanes x P/256 objects, a butterfly per wave, the four partial triples
// through LDS (sh.red is free until the final sum); lane `ent` of the workgroup merges them and keeps the entry in slot 0
__device__ __forceinline__ void emd_bid_block(EmdShared& sh, const float* __restrict__ a, int P, float u, int e, int n,
                                              const unsigned short* list, int& ei, int& ej, unsigned long long& ew) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* part = (int*)sh.red;
    for (int ent = 0; ent < n; ++ent) {
        const int i = __builtin_amdgcn_readfirstlane((int)list[ent]);
        const float ax = a[i * 3], ay = a[i * 3 + 1], az = a[i * 3 + 2];
        EmdTop top;
        top.w1 = top.w2 = kEmdMin;
        top.j1 = kEmdMaxP + tid;
        for (int j = tid; j < P; j += kEmdBlock) top.take(-sg_emd_cost(sg_emd_dist(ax, ay, az, sh.b[0][j], sh.b[1][j], sh.b[2][j]), u) - sh.price[j], j);
        emd_wave_reduce(top);
        if (lane == 0) {
            int* slot = part + (ent * kEmdWaves + wave) * 3;
            slot[0] = top.w1;
            slot[1] = top.j1;
            slot[2] = top.w2;
        }
    }
    __syncthreads();
    if (tid < n) {
        EmdTop top;
        top.w1 = part[tid * kEmdWaves * 3], top.j1 = part[tid * kEmdWaves * 3 + 1], top.w2 = part[tid * kEmdWaves * 3 + 2];
#pragma unroll
        for (int w = 1; w < kEmdWaves; ++w) {
            const int* slot = part + (tid * kEmdWaves + w) * 3;
            EmdTop o;
            o.w1 = slot[0], o.j1 = slot[1], o.w2 = slot[2];
            emd_merge(top, o);
        }
        ei = list[tid];
        ej = top.j1;
        ew = emd_word(sh, top, e, ei);
        atomicMax(&sh.bid[ej], ew);
    }
}

// mode 0: matched batches (blockIdx.x = pair); 1: matrix (blockIdx.y = cloud of A, blockIdx.x = cloud of B); 2: symmetric matrix
__global__ void __launch_bounds__(kEmdBlock) emd_auction_kernel(const float* __restrict__ A, const float* __restrict__ B, int P, float u,
                                                               int mode, int wave_scan_at, int block_scan_at, int* __restrict__ match,
                                                               double* __restrict__ emd, int* __restrict__ rounds,
                                                               int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) EmdShared sh;
    const int tid = threadIdx.x;
    const long ci = mode == 0 ? blockIdx.x : blockIdx.y, cj = blockIdx.x, Sb = gridDim.x;
    const long out = mode == 0 ? ci : ci * Sb + cj;
    if (mode == 2 && ci >= cj) {
        if (ci == cj && tid == 0) {
            emd[out] = 0.0;
            status[out] = 0;
            rounds[out] = 0;
        }
        return;                                        // [j][i] is written by the workgroup of [i][j]
    }
    const float* __restrict__ a = A + ci * P * 3;
    const float* __restrict__ b = B + cj * P * 3;

    for (int j = tid; j < P; j += kEmdBlock) {
        sh.b[0][j] = b[j * 3];
        sh.b[1][j] = b[j * 3 + 1];
        sh.b[2][j] = b[j * 3 + 2];
        sh.price[j] = 0;
        sh.bid[j] = 0ull;
    }
    if (tid == 0) sh.kmax = 0, sh.too_small = 0;
    __syncthreads();

    // the largest cost of the pair, and whether a finite distance is beyond the integer range
    {
        int kmax = 0, too_small = 0;
        for (int i = tid; i < P; i += kEmdBlock) {
            const float ax = a[i * 3], ay = a[i * 3 + 1], az = a[i * 3 + 2];
            for (int j = 0; j < P; ++j) {
                const float d = sg_emd_dist(ax, ay, az, sh.b[0][j], sh.b[1][j], sh.b[2][j]);
                const int k = sg_emd_cost(d, u);
                too_small |= sg_emd_too_small(d, u) ? 1 : 0;
                kmax = k > kmax ? k : kmax;
            }
        }
        atomicMax(&sh.kmax, kmax);
        if (too_small) atomicOr(&sh.too_small, 1);
    }
    __syncthreads();

    int st = sh.too_small ? SG_EMD_STATUS_EPS : 0, total = 0;
    if (st == 0) {
        const int kmax = sh.kmax;
        for (int e = kmax >> 4 > 1 ? kmax >> 4 : 1;; e = e >> 2 > 1 ? e >> 2 : 1) {
            __syncthreads();                           // every lane has seen the end of the previous phase
            for (int j = tid; j < P; j += kEmdBlock) {
                sh.owner[j] = (unsigned short)kEmdNone;
                sh.list[0][j] = (unsigned short)j;
            }
            if (tid == 0) sh.cnt[0] = P;
            __syncthreads();
            int cur = 0;
            for (int r = 0;; ++r) {
                const int n = sh.cnt[cur];             // the same in every lane: written before the last barrier
                if (n == 0) break;
                if (r == SG_EMD_ROUND_CAP) {
                    st = SG_EMD_STATUS_ROUND_CAP;
                    break;
                }
                ++total;
                if (tid == 0) sh.cnt[cur ^ 1] = 0;     // last read two barriers ago
                int ei[kEmdSlots], ej[kEmdSlots], ne;
                unsigned long long ew[kEmdSlots];
                const unsigned short* list = sh.list[cur];
                if (n <= block_scan_at) {
                    emd_bid_block(sh, a, P, u, e, n, list, ei[0], ej[0], ew[0]);
                    ne = tid < n ? 1 : 0;
                } else if (n <= wave_scan_at) {
                    emd_bid_waves(sh, a, P, u, e, n, list, ei[0], ej[0], ew[0]);
                    const int wave = tid >> 6;
                    ne = (tid & 63) < (n - wave + kEmdWaves - 1) / kEmdWaves ? 1 : 0;
                } else {
                    if (n <= kEmdBlock) emd_bid_lanes<1>(sh, a, P, u, e, n, list, ei, ej, ew);
                    else if (n <= 2 * kEmdBlock) emd_bid_lanes<2>(sh, a, P, u, e, n, list, ei, ej, ew);
                    else if (n <= 4 * kEmdBlock) emd_bid_lanes<4>(sh, a, P, u, e, n, list, ei, ej, ew);
                    else emd_bid_lanes<8>(sh, a, P, u, e, n, list, ei, ej, ew);
                    ne = tid < n ? (n - tid + kEmdBlock - 1) / kEmdBlock : 0;
                }
                __syncthreads();
                unsigned short* next = sh.list[cur ^ 1];
#pragma unroll
                for (int m = 0; m < kEmdSlots; ++m)
                    if (m < ne) {
                        int back = ei[m];
                        if (sh.bid[ej[m]] == ew[m]) {   // the word carries the bidder: it stands for one entry only
                            back = sh.owner[ej[m]];
                            sh.owner[ej[m]] = (unsigned short)ei[m];
                            sh.price[ej[m]] = (int)(ew[m] >> 32);
                        }
                        if (back != kEmdNone) next[atomicAdd(&sh.cnt[cur ^ 1], 1)] = (unsigned short)back;
                    }
                __syncthreads();
                cur ^= 1;
            }
            if (st != 0 || e == 1) break;
        }
    }
    __syncthreads();

    // match[i] by bidder (the auction keeps owners by object), the distances of the matching, their float64 sum in K13's order
    unsigned short* asg = sh.list[0];
    for (int i = tid; i < P; i += kEmdBlock) asg[i] = (unsigned short)i;      // what a pair without a result reports
    __syncthreads();
    if (st == 0)
        for (int j = tid; j < P; j += kEmdBlock) asg[sh.owner[j]] = (unsigned short)j;
    __syncthreads();
    double s = 0.0;
    for (int i = tid; i < P; i += kEmdBlock) {
        const int j = asg[i];
        if (match) match[ci * P + i] = j;
        s += (double)sg_emd_dist(a[i * 3], a[i * 3 + 1], a[i * 3 + 2], sh.b[0][j], sh.b[1][j], sh.b[2][j]);
    }
    sh.red[tid] = s;
    __syncthreads();
#pragma unroll
    for (int off = kEmdBlock / 2; off > 0; off >>= 1) {
        if (tid < off) sh.red[tid] += sh.red[tid + off];
        __syncthreads();
    }
    if (tid == 0) {
        const double value = st == 0 ? sh.red[0] / (double)P : (double)__builtin_nanf("");
        emd[out] = value;
        status[out] = st;
        if (rounds) rounds[out] = total;
        if (mode == 2) {
            const long mirror = cj * Sb + ci;
            emd[mirror] = value;
            status[mirror] = st;
            rounds[mirror] = total;
        }
    }
}

static int emd_check(long S, long P, double eps, const char* who) {
    const int refused = sg_emd_refused(S, P, eps);
    if (refused == 1)
        SG_FAIL(SG_ERR_ARG, "%s: 1 <= P <= %d points per cloud and at most 65535 clouds per call, got P = %ld", who, SG_EMD_MAX_POINTS, P);
    if (refused) SG_FAIL(SG_ERR_ARG, "%s: eps must be a finite number of at least 4.8e-38, got %g", who, eps);
    return SG_OK;
}

static int emd_wave_scan_at(int requested) {
    return requested < 0 ? kEmdWaveScanDefault : (requested > kEmdWaveScanMax ? kEmdWaveScanMax : requested);
}

static int emd_block_scan_at(int requested) {
    return requested < 0 ? kEmdBlockScanDefault : (requested > kEmdBlockScanMax ? kEmdBlockScanMax : requested);
}

}  // namespace sg

using namespace sg;

extern "C" {

int sg_emd_match_impl(const float* A, const float* B, long S, long P, double eps, int* match, double* emd, int* rounds, int* status,
                      int wave_scan_at, int block_scan_at, hipStream_t stream) {
    SG_CHECK_ARG(A && B && emd && status);
    if (int rc = emd_check(S, P, eps, __func__)) return rc;
    hipLaunchKernelGGL(emd_auction_kernel, dim3((unsigned)S), dim3(kEmdBlock), 0, stream, A, B, (int)P, sg_emd_unit(eps), 0,
                       emd_wave_scan_at(wave_scan_at), emd_block_scan_at(block_scan_at), match, emd, rounds, status);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

int sg_emd_match(const float* A, const float* B, long S, long P, double eps, int* match, double* emd, int* rounds, int* status,
                 hipStream_t stream) {
    return sg_emd_match_impl(A, B, S, P, eps, match, emd, rounds, status, -1, -1, stream);
}

size_t sg_emd_matrix_workspace_bytes(long Sa, long Sb, long P) {
    if (Sa < 1 || Sb < 1 || Sa > 65535 || Sb > 65535 || P < 1 || P > SG_EMD_MAX_POINTS) return 0;
    return (size_t)(Sa * Sb) * sizeof(int);
}

int sg_emd_matrix(const float* A, const float* B, long Sa, long Sb, long P, double eps, int symmetric, double* emd, int* status,
                  void* workspace, size_t workspace_bytes, hipStream_t stream) {
    SG_CHECK_ARG(A && B && emd && status && workspace && Sb >= 1 && Sb <= 65535 && (!symmetric || Sa == Sb));
    if (int rc = emd_check(Sa, P, eps, __func__)) return rc;
    if (workspace_bytes < sg_emd_matrix_workspace_bytes(Sa, Sb, P)) SG_FAIL(SG_ERR_WORKSPACE, "sg_emd_matrix: workspace too small");
    hipLaunchKernelGGL(emd_auction_kernel, dim3((unsigned)Sb, (unsigned)Sa), dim3(kEmdBlock), 0, stream, A, B, (int)P, sg_emd_unit(eps),
                       symmetric ? 2 : 1, emd_wave_scan_at(-1), emd_block_scan_at(-1), (int*)nullptr, emd, (int*)workspace, status);
    SG_CHECK_LAUNCH();
    return SG_OK;
}

}  // extern "C"
