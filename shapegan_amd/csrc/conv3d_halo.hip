// shapegan_amd/csrc/conv3d_halo.hip — LDS-halo implicit GEMM for the channel-heavy Conv3d(k4,s2,p1) forward.
//
// Same math as conv3d.hip's `fwd` form (nn.Conv3d forward: model/gan.py:49-53, model/autoencoder.py:16-24,
// model/progressive_gan.py:38; nn.ConvTranspose3d input-gradient), different data movement:
//
//   * a workgroup owns 64 output positions of ONE sample (a TD x TH x TW box) x 64*TM output channels;
//   * per stage it copies the input HALO box (2TD+2)(2TH+2)(2TW+2) of CC channels into LDS with row-coalesced
//     global loads — every input voxel is fetched once per workgroup instead of once per tap (8x less TA/L1
//     traffic than the gather kernel) — W columns de-interleaved by parity so that the stride-2 window walk of
//     the 32 positions of a half-wave is conflict-free;
//   * MFMA B fragments (v_mfma_f32_32x32x2_f32: lane = position, k-pair) are read straight from that box: the tap
//     offset is uniform per k-step, so a read is one ds_read_b32 with an immediate offset — no staging copy of B;
//   * MFMA A fragments come from a pre-packed weight image in global memory (L2-resident), one coalesced
//     global_load_dwordx4 per lane per 4 k-steps, prefetched one group ahead — no LDS and no staging for A either
//     (the same scheme as the fused SDFNet kernel).
//   Per stage of CC=8 channels a wave issues 256*TM MFMAs (16K-32K matrix-pipe cycles) against ~70 loads and
//   ~70 LDS writes per thread of staging.
#include "conv_common.h"

#ifndef SG_RING
#define SG_RING 8
#endif
#ifndef SG_ABLATE
#define SG_ABLATE 0   // tuning experiments only (scripts/ablate.sh of rounds 1-3: git history): 1 no copy loads, 2 no copy, 4 no weight loads
#endif

namespace sg {

// Fixed tile: 1 x 8 x 8 output positions (one D slice, 8 rows, 8 columns) -> halo box 4 x 18 x 18 input voxels.
constexpr int kHD = 4, kHH = 18, kHWF = 18;  // halo extent in D, H, W
constexpr int kHWH = 10;                      // W halves per parity (9 used, padded so that 4*kHWH = 8 mod 32)
constexpr int kROWH = 2 * kHWH;               // one H row = [even columns | odd columns]
constexpr int kROWD = kHH * kROWH;            // 360
constexpr int kHS = kHD * kROWD;              // 1440 floats per channel
constexpr int kCC = 4;                        // channels per stage; LDS = 2 buffers x 4 x 1440 x 4 B = 46 KB

struct HaloFwdArgs {
    const float* x;
    const float4* wp;
    const float* bias;
    float* y;
    ConvGeom g;
    int Cin, Cout;
    int nth, ntw;  // tiles per H / W (one tile per D slice)
    FastDiv dntw, dnth, dOD;
    int act;
    float slope;
    // conv_fwd_halo4_kernel with the input channels split over `csplit` workgroups (grid z): raw partial sums
    // partial[(z * Cout + co) * npos + n * 64 + p], finished (sum, bias, activation) by the gather kernel's split-K finalize
    int csplit;
    float* partial;
    long npos;
};

// Element e of a forward weight image.
// mode 0 (32x32x2 kernels): Wp[(mt*G + g)*64 + lane] = float4{ W[mt*32 + (lane&31)][8g + 2j + (lane>>5)] , j = 0..3 }   (G = Cin*8 groups)
// mode 1 (conv_fwd_halo4_dskip_kernel, 16x16x4): 16-row tiles, G = Cin*4 groups g = (ci, kd):
//         Wp[(mt*G + g)*64 + lane] = float4{ W[mt*16 + (lane&15)][ci][kd][kh = j][kw = lane>>4] , j = 0..3 }
// Both images have ntile32 * Cin * 8 * 64 float4 (a 32-row tile = two 16-row tiles).
__device__ __forceinline__ float4 fwd_image_element(const float* __restrict__ w, long e, int Cout, int Cin_total, int Cin, int mode) {
    const int lane = (int)(e & 63);
    const long q = e >> 6;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mode == 0) {
        const long G = (long)Cin * 8;
        const long g = q % G;
        const int mt = (int)(q / G);
        const int co = mt * 32 + (lane & 31);
        if (co < Cout) {
            const float* src = w + (long)co * Cin_total * 64 + g * 8 + (lane >> 5);
            v = make_float4(src[0], src[2], src[4], src[6]);
        }
    } else {
        const long G = (long)Cin * 4;
        const long g = q % G;
        const int mt = (int)(q / G);
        const int co = mt * 16 + (lane & 15);
        if (co < Cout) {
            const float* src = w + (long)co * Cin_total * 64 + g * 16 + (lane >> 4);
            v = make_float4(src[0], src[4], src[8], src[12]);
        }
    }
    return v;
}
// ntile counts 32-row tiles in both modes
__global__ void __launch_bounds__(256) pack_fwd_weights_kernel(const float* __restrict__ w, float4* __restrict__ wp,
                                                               int Cout, int Cin_total, int Cin, int ntile, int mode) {
    const long total = (long)ntile * Cin * 8 * 64;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256)
        wp[e] = fwd_image_element(w, e, Cout, Cin_total, Cin, mode);
}

// ---- addressing helpers shared by the three halo kernels ---------------------------------------------------------
// Every non-MFMA VALU instruction in the stage loop takes an issue slot away from the matrix pipe (measured: ~1 VALU op
// per MFMA costs ~10 %), so the loops are written to need none:
//   * global loads are raw BUFFER loads: scalar resource + a per-thread byte offset that never changes + a scalar
//     offset that carries everything that does (channel, k-group) — no 64-bit vector address arithmetic; an element
//     outside the tensor gets an offset beyond num_records and the hardware returns 0 (no select on the way to LDS);
//   * LDS addresses are per-thread constants held in registers, everything else is an immediate offset: the stage loop
//     is unrolled by two so that the double-buffer index is a compile-time constant.
// Software pipeline per stage (4 input channels = 32 k-groups of 8 k, 4*TN MFMAs each).  The loop body is ONE basic
// block (no data-dependent branches), so that the compiler's s_waitcnt counts are exact and nothing drains the queues:
//   * the MFMAs of stage s read halo buffer s&1 while the SAME waves copy stage s+1's box into buffer (s+1)&1: the copy
//     loads are spread over the first 24 k-groups (all workgroups run in lock-step: a burst at the top of the stage is a
//     chip-wide traffic jam once per stage, measured -8 %), each value goes to LDS 8 groups after its load.
//     Threads outside the box store to an unused pad slot of the channel; the last stage re-copies its own channels
//     into the idle buffer — no branch anywhere;
//   * B fragments of group g+1 are read from LDS while the MFMAs of group g run; A fragments (packed weights, L2) sit in
//     a ring of 8 groups; one barrier per stage.
// Wave tile: 32 output channels x TN*32 positions (TN = 2: 4 waves cover 128 channels x 64 positions, two independent
// accumulators per wave; TN = 1: 8 or 4 waves as rows x position halves).
template <int TN, int NW>
__global__ void __launch_bounds__(NW * 64) conv_fwd_halo_kernel(HaloFwdArgs a) {
    constexpr int kFR = NW * 2;                          // halo rows copied per pass (one per half-wave)
    constexpr int kNF = (kHD * kHH + kFR - 1) / kFR;     // fill elements per thread per channel (72 rows)
    constexpr int WN = 2 / TN;                           // waves along the 64 positions
    constexpr int ROWS = (NW / WN) * 32;                 // output channels per workgroup
    constexpr int kRing = SG_RING;
    constexpr int kBUF = kCC * kHS;                      // floats per LDS buffer
    extern __shared__ __attribute__((aligned(16))) float halo[];  // [2][kCC][kHD][kHH][2][kHWH]
    lds_float* const hl = (lds_float*)halo;

    uint32_t twi, thi, od, n, q1, q2;
    a.dntw.divmod(blockIdx.x, q1, twi);
    a.dnth.divmod(q1, q2, thi);
    a.dOD.divmod(q2, n, od);
    const int oh0 = thi * 8, ow0 = twi * 8;
    const int co0 = blockIdx.y * ROWS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN, r = lane & 31, kpar = lane >> 5;
    // position inside the 8x8 tile of column tile u: p = (wn*TN + u)*32 + r -> ph = p >> 3, pw = p & 7
    const int lanebase = 2 * (wn * TN * 4 + (r >> 3)) * kROWH + kpar * kHWH + (r & 7);
    constexpr int kTNOFF = 2 * 4 * kROWH;  // LDS offset between the two column tiles of a wave (4 tile rows)

    f32x16 acc[TN];
#pragma unroll
    for (int u = 0; u < TN; ++u)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[u][q] = 0.f;

    // B-fragment read addresses: one register per (buffer, channel, kd); kh pair and column tile are immediates
    const lds_float* bb[2][kCC][4];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int c = 0; c < kCC; ++c)
#pragma unroll
            for (int kd = 0; kd < 4; ++kd) {
                bb[b][c][kd] = hl + b * kBUF + c * kHS + kd * kROWD + lanebase;
                pin_vgpr(bb[b][c][kd]);
            }

    // packed weights of this wave's 32 rows: buffer resource on the row tile, lane offset fixed, k-group in the scalar offset
    const int G = a.Cin * 8;
    const __amdgpu_buffer_rsrc_t wres = make_rsrc(a.wp + ((long)(co0 / 32 + wm) * G) * 64);
    const unsigned wvoff = lane * 16;

    // ---- fill bookkeeping: element f of a channel is halo row kFR*f + tid/32, column tid%32 ----
    const int I3 = a.g.ID * a.g.IH * a.g.IW;
    const __amdgpu_buffer_rsrc_t xres = make_rsrc(a.x + (long)n * a.g.Cx * I3);
    const int fl_w = tid & 31, frow = tid >> 5;
    const int iw = 2 * ow0 - 1 + fl_w;
    const bool wok = fl_w < kHWF && (unsigned)iw < (unsigned)a.g.IW;
    const int lds_w = (fl_w & 1) * kHWH + (fl_w >> 1);
    const int pad = (tid % (kHD * kHH * 2)) * kHWH + (kHWH - 1);  // column 9 of a half row: never read
    unsigned goff[kNF];   // byte offset inside a channel, kBufOutside for padding voxels (the load returns 0)
    lds_float* sdst[kNF];  // LDS destination inside (buffer 0, channel 0)
#pragma unroll
    for (int f = 0; f < kNF; ++f) {
        const int row = kFR * f + frow, hd = row / kHH, hh = row - hd * kHH;
        const int id = 2 * (int)od - 1 + hd, ih = 2 * oh0 - 1 + hh;
        const bool inbox = fl_w < kHWF && row < kHD * kHH;
        const bool ok = inbox && wok && (unsigned)id < (unsigned)a.g.ID && (unsigned)ih < (unsigned)a.g.IH;
        goff[f] = ok ? (unsigned)((id * a.g.IH + ih) * a.g.IW + iw) * 4u : kBufOutside;
        sdst[f] = hl + (inbox ? hd * kROWD + hh * kROWH + lds_w : pad);
        pin_vgpr(goff[f]);
        pin_vgpr(sdst[f]);
    }
    float fv[kCC][kNF];
    const unsigned chan_bytes = (unsigned)I3 * 4u;

    // ---- prologue: box of stage 0 into buffer 0, first kRing weight groups ----
#pragma unroll
    for (int c = 0; c < kCC; ++c)
#pragma unroll
        for (int f = 0; f < kNF; ++f) fv[c][f] = buf_load(xres, goff[f], c * chan_bytes);
    float4 aring[kRing];
#pragma unroll
    for (int u = 0; u < kRing; ++u) aring[u] = buf_load4(wres, wvoff, (unsigned)(u < G ? u : G - 1) * 1024u);
#pragma unroll
    for (int c = 0; c < kCC; ++c)
#pragma unroll
        for (int f = 0; f < kNF; ++f) sdst[f][c * kHS] = fv[c][f];
    __syncthreads();

    const int nstage = a.Cin / kCC;
    int gbase = kRing;  // first group index to prefetch in this stage

    auto stage = [&](auto tag, int s) {
        constexpr int CUR = decltype(tag)::value, NXT = CUR ^ 1;
        int cnext = (s + 1) * kCC;
        cnext = cnext > a.Cin - kCC ? a.Cin - kCC : cnext;
        const unsigned xs = (unsigned)cnext * chan_bytes;
        float bq[TN][4];  // B fragments of the first group
#pragma unroll
        for (int u = 0; u < TN; ++u) {
            const lds_float* hb = bb[CUR][0][0] + u * kTNOFF;
            bq[u][0] = hb[0];
            bq[u][1] = hb[1];
            bq[u][2] = hb[kROWH];
            bq[u][3] = hb[kROWH + 1];
        }
        // sched_barrier(0): the machine scheduler otherwise sinks every load to just before its use (to save registers),
        // which turns the ring / the early copy loads into load -> s_waitcnt vmcnt(0) -> use
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ci = 0; ci < kCC; ++ci) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {  // k-group j of channel ci: kd = j >> 1, kh pair = j & 1
                const float4 a_cur = aring[(ci * 8 + j) % kRing];
                int gi = gbase + ci * 8 + j;
                gi = gi < G ? gi : G - 1;
                if (!(SG_ABLATE & 4)) aring[(ci * 8 + j) % kRing] = buf_load4(wres, wvoff, (unsigned)gi * 1024u);
                {  // copy of the next box: element e is loaded in group e*24/NE and stored 8 groups later
                    constexpr int NE = kCC * kNF;
                    const int gidx = ci * 8 + j;
#pragma unroll
                    for (int e = 0; e < NE; ++e) {
                        const int c = e / kNF, f = e % kNF;
                        if (e * 24 / NE + 8 == gidx && !(SG_ABLATE & 2)) sdst[f][NXT * kBUF + c * kHS] = fv[c][f];
                        if (e * 24 / NE == gidx && !(SG_ABLATE & 3)) fv[c][f] = buf_load(xres, goff[f], xs + c * chan_bytes);
                    }
                }
                float b[TN][4];
#pragma unroll
                for (int u = 0; u < TN; ++u)
#pragma unroll
                    for (int k = 0; k < 4; ++k) b[u][k] = bq[u][k];
                if (!(ci == kCC - 1 && j == 7) && !(SG_ABLATE & 16)) {  // B fragments of the next group of this stage
                    const int jn = (j + 1) & 7, cin = ci + ((j + 1) >> 3);
                    const lds_float* hb = bb[CUR][cin][jn >> 1] + (2 * (jn & 1)) * kROWH;
#pragma unroll
                    for (int u = 0; u < TN; ++u) {
                        bq[u][0] = hb[u * kTNOFF];
                        bq[u][1] = hb[u * kTNOFF + 1];
                        bq[u][2] = hb[u * kTNOFF + kROWH];
                        bq[u][3] = hb[u * kTNOFF + kROWH + 1];
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int u = 0; u < TN; ++u) {
                        const float av = k == 0 ? a_cur.x : (k == 1 ? a_cur.y : (k == 2 ? a_cur.z : a_cur.w));
                        acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[u][k], acc[u], 0, 0, 0);
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        gbase += 8 * kCC;
        __syncthreads();  // next box complete and visible; everyone is done reading the current one
    };
    for (int s = 0; s + 1 < nstage; s += 2) {   // stages in pairs: the buffer index is a compile-time constant
        stage(IntTag<0>(), s);
        stage(IntTag<1>(), s + 1);
    }
    if (nstage & 1) stage(IntTag<0>(), nstage - 1);

    // epilogue: y[n][co][od][oh0+ph][ow0+pw] = act(acc + bias[co]); all bias loads are issued before the first use
    const long O3 = (long)a.g.OD * a.g.OH * a.g.OW;
    float bv[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int co = co0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * kpar;
        bv[q] = a.bias ? a.bias[co < a.Cout ? co : a.Cout - 1] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < TN; ++u) {
        const int ph = (wn * TN + u) * 4 + (r >> 3), pw = r & 7;
        float* yo = a.y + (long)n * a.Cout * O3 + ((long)od * a.g.OH + (oh0 + ph)) * a.g.OW + (ow0 + pw);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int co = co0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * kpar;
            if (co < a.Cout) yo[(long)co * O3] = sg_apply_act(acc[u][q] + bv[q], a.act, a.slope);
        }
    }
}

// ---- forward form on 4^3 output grids (8^3 inputs: Conv3d 128 -> 256 of the discriminators) ------------------------
// The 1x8x8 tiling does not exist here; instead the WHOLE zero-padded sample (10^3 per channel) is the box and the 64
// output voxels of the sample are the 64 columns of the workgroup.  The padding never changes, so it is written once
// (zero fill of both buffers) and a stage copies only the 8^3 real voxels of its channels with fully coalesced loads.
// Layout per channel: [10 d][10 h][even w | odd w] with the plane stride padded to 104 floats, which makes the 32-lane
// fragment read (2 od x 4 oh x 4 ow, strides 208 / 20 / 1) conflict-free.
// 8 waves: (K half) x (row tile pair) x (position half): waves 0-3 take channels 0-3 of every 8-channel stage, waves 4-7
// channels 4-7 — a sample has only 64 output positions, so the second wave group comes from splitting K; the two
// partial accumulators meet in LDS at the end.  Grid = batch x Cout/64 (x csplit: small batches — 16 samples are 64 workgroups, and
// one workgroup's walk over 128 channels is 130 us however few there are — split the input channels over 2 - 8 workgroups
// that write raw partial sums; round 6, it was the gather GEMM at 0.44 of the matrix peak below 160 workgroups).
constexpr int k4HALF = 5, k4ROW = 10, k4PLANE = 104, k4CH = 10 * k4PLANE;   // 1040 floats per channel
constexpr int k4CC = 8;                                                      // channels per stage
constexpr int k4BUF = k4CC * k4CH;                                           // 8320 floats = 33 KB per buffer

__global__ void __launch_bounds__(512) conv_fwd_halo4_kernel(HaloFwdArgs a) {
    constexpr int kRing = 8;
    extern __shared__ __attribute__((aligned(16))) float halo[];  // [2][k4CC][k4CH]
    lds_float* const hl = (lds_float*)halo;
    const int n = blockIdx.x, co0 = blockIdx.y * 64;
    const int cpw = a.Cin / a.csplit, cb = blockIdx.z * cpw;      // this workgroup's input channels [cb, cb + cpw)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kh = wave >> 2, wm = (wave >> 1) & 1, wn = wave & 1, r = lane & 31, kpar = lane >> 5;
    const int p = wn * 32 + r, od = p >> 4, oh = (p >> 2) & 3, ow = p & 3;
    const int lanebase = 2 * od * k4PLANE + 2 * oh * k4ROW + kpar * k4HALF + ow;

    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;

    // zero both buffers once: the halo padding is never written again
    for (int e = tid; e < 2 * k4BUF; e += 512) hl[e] = 0.f;

    const lds_float* bb[2][4][4];   // (buffer, own channel, kd)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int kd = 0; kd < 4; ++kd) {
                bb[b][c][kd] = hl + b * k4BUF + (kh * 4 + c) * k4CH + kd * k4PLANE + lanebase;
                pin_vgpr(bb[b][c][kd]);
            }
    const int G = a.Cin * 8;
    const __amdgpu_buffer_rsrc_t wres = make_rsrc(a.wp + ((long)(co0 / 32 + wm) * G) * 64);
    const unsigned wvoff = lane * 16;

    // copy: a channel is 512 contiguous floats; thread t moves element t of each of the stage's 8 channels
    const int I3 = 512;
    const __amdgpu_buffer_rsrc_t xres = make_rsrc(a.x + ((long)n * a.g.Cx + cb) * I3);
    unsigned xvoff = tid * 4;
    lds_float* sdst = hl + ((tid >> 6) + 1) * k4PLANE + (((tid >> 3) & 7) + 1) * k4ROW + (((tid & 7) + 1) & 1) * k4HALF +
                      (((tid & 7) + 1) >> 1);
    pin_vgpr(xvoff);
    pin_vgpr(sdst);
    float fv[k4CC];
    __syncthreads();   // zero fill done before the first real voxels land
#pragma unroll
    for (int c = 0; c < k4CC; ++c) fv[c] = buf_load(xres, xvoff, c * (I3 * 4));
    // weight groups of this wave in order: stage s, own channel c, j -> group (s*8 + kh*4 + c)*8 + j = s*64 + kh*32 + (c*8+j)
    const int nstage = cpw / k4CC, nq = nstage * 32, s0 = cb / k4CC;
    auto group_of = [&](int q) {
        q = q < nq ? q : nq - 1;
        return ((q >> 5) + s0) * 64 + kh * 32 + (q & 31);
    };
    float4 aring[kRing];
#pragma unroll
    for (int u = 0; u < kRing; ++u) aring[u] = buf_load4(wres, wvoff, (unsigned)group_of(u) * 1024u);
#pragma unroll
    for (int c = 0; c < k4CC; ++c) sdst[c * k4CH] = fv[c];
    __syncthreads();

    int qbase = kRing;
    auto stage = [&](auto tag, int s) {
        constexpr int CUR = decltype(tag)::value, NXT = CUR ^ 1;
        int cnext = (s + 1) * k4CC;
        cnext = cnext > cpw - k4CC ? cpw - k4CC : cnext;
        const unsigned xs = (unsigned)cnext * (I3 * 4);
        float bq[4];
        {
            const lds_float* hb = bb[CUR][0][0];
            bq[0] = hb[0];
            bq[1] = hb[1];
            bq[2] = hb[k4ROW];
            bq[3] = hb[k4ROW + 1];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ci = 0; ci < 4; ++ci) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int gidx = ci * 8 + j;
                const float4 a_cur = aring[gidx % kRing];
                aring[gidx % kRing] = buf_load4(wres, wvoff, (unsigned)group_of(qbase + gidx) * 1024u);
                // copy of the next box: channel c is loaded in group 2c and stored in group 2c + 8
#pragma unroll
                for (int c = 0; c < k4CC; ++c) {
                    if (2 * c + 8 == gidx) sdst[NXT * k4BUF + c * k4CH] = fv[c];
                    if (2 * c == gidx) fv[c] = buf_load(xres, xvoff, xs + c * (I3 * 4));
                }
                float b[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) b[k] = bq[k];
                if (gidx + 1 < 32) {
                    const int jn = (j + 1) & 7, cin = ci + ((j + 1) >> 3);
                    const lds_float* hb = bb[CUR][cin][jn >> 1] + (2 * (jn & 1)) * k4ROW;
                    bq[0] = hb[0];
                    bq[1] = hb[1];
                    bq[2] = hb[k4ROW];
                    bq[3] = hb[k4ROW + 1];
                }
                __builtin_amdgcn_sched_barrier(0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.x, b[0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.y, b[1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.z, b[2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur.w, b[3], acc, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        qbase += 32;
        __syncthreads();
    };
    for (int s = 0; s + 1 < nstage; s += 2) {
        stage(IntTag<0>(), s);
        stage(IntTag<1>(), s + 1);
    }
    if (nstage & 1) stage(IntTag<0>(), nstage - 1);

    // the K halves meet in LDS (the boxes are dead after the last barrier): waves 4-7 park, waves 0-3 add and store
    float* red = halo + ((wave & 3) * 16) * 64;
    if (kh == 1) {
#pragma unroll
        for (int q = 0; q < 16; ++q) red[q * 64 + lane] = acc[q];
    }
    __syncthreads();
    if (kh == 1) return;
    if (a.csplit > 1) {      // raw partial sums, row-major [co][sample * 64 + p] per channel split
        float* po = a.partial + (long)blockIdx.z * a.Cout * a.npos + (long)n * 64 + p;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int co = co0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * kpar;
            if (co < a.Cout) po[(long)co * a.npos] = acc[q] + red[q * 64 + lane];
        }
        return;
    }
    // y[n][co][p], p = od*16 + oh*4 + ow: 32 consecutive floats per (co, position half)
    float* yo = a.y + (long)n * a.Cout * 64 + p;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int co = co0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * kpar;
        if (co < a.Cout) {
            const float bv = a.bias ? a.bias[co] : 0.f;
            yo[(long)co * 64] = sg_apply_act(acc[q] + red[q * 64 + lane] + bv, a.act, a.slope);
        }
    }
}

// ---- depth-skip form of conv_fwd_halo4_kernel ---------------------------------------------------------------------------------
// Same workgroup (one sample x 64 output channels, the two K halves of every 8-channel stage, the whole padded sample as the
// box), on v_mfma_f32_16x16x4_f32: a 16-column tile is ONE output depth plane od (4 x 4 positions), k = 4 is the four kw of one
// (kd, kh).  8 waves = (K half) x (four 16-row blocks); a wave holds all four planes of its rows, 4 accumulators of 4 registers.
//   The B fragment of (od, kd, kh) is the padded plane d' = 2 od + kd at row 2 oh + kh.  d' = 0 (od 0, kd 0) and d' = 9 (od 3,
//   kd 3) are padding for every sample, stage and wave: those two tiles of the 16 per kh are not issued and not read — 14 MFMAs
//   and 14 LDS reads per (channel, kh) instead of 16 and 16, a static and balanced skip.
//   16 rows per wave (not 32 with a shared B fragment): 32 rows would leave 4 waves of one K half or a four-way K split with a
//   four-way reduction; with 16 rows the LDS reads per MFMA cycle are those of conv_fwd_halo4_kernel (one ds_read_b32 per 32 MFMA
//   cycles: a quarter of the LDS issue with four waves per SIMD) and the weight loads per workgroup are halved (every wave
//   loads its own rows once).
//   Box layout per channel: [10 d][5 row pairs][even h: even w | odd h: even w | even h: odd w | odd h: odd w], a half row of 5
//   every 6 floats, 24 per row pair, plane = 120: word(h', w') = (h' >> 1) * 24 + (h' & 1) * 6 + (w' & 1) * 12 + (w' >> 1).  The
//   lane's k index (lane >> 4) is kw, in the order of conv_fwd_halo4_kernel's k-pairs, so that the sum of every output runs over
//   (ci, kd, kh, kw) in the same order there and here: for finite inputs the two forms agree bit for bit (the skipped products are
//   exact zeros).  A read of (od, kd, kh) is h' = 2 oh + kh, w' = 2 ow + kw: the lanes 0 - 31 (kw 0, 1) read the words
//   24 oh + 12 kw + ow (+ const) = banks 0 - 3, 12 - 15 | 24 - 27, 4 - 7 | 16 - 19, 28 - 31 | 8 - 11, 20 - 23 for oh = 0 .. 3: each
//   of the 32 banks once (ds_read_b32: two groups of 32 lanes); the lanes 32 - 63 (kw 2, 3) the same one word on.  With the
//   [even w | odd w] rows of 10 of conv_fwd_halo4_kernel the same read is 20 oh + 5 kw + ow: two-way conflicts on five banks.
//   Accumulator of plane od, register v, lane l: channel co0 + 16 wr + 4 (l >> 4) + v at position (od, (l >> 2) & 3, l & 3).
//   LDS 2 x 8 x 1200 x 4 B = 75 KB: two workgroups per CU as before.  Channel splits (csplit > 1) stay with conv_fwd_halo4_kernel.
// Semantics: the skipped products are weight x (zero padding of x beyond the depth range): for finite weights the value of the
// same sum with the zeros added; a non-finite weight on such a tap gives NaN in conv_fwd_halo4_kernel and the sum over the
// in-range positions here.  The h / w padding is multiplied as before.
constexpr int k4sHODD = 6, k4sWODD = 12, k4sPAIR = 24, k4sPLANE = 120, k4sCH = 10 * k4sPLANE;   // 1200 floats per channel
__host__ __device__ constexpr int k4s_row(int h) { return (h >> 1) * k4sPAIR + (h & 1) * k4sHODD; }   // word of padded row h'
constexpr int k4sBUF = k4CC * k4sCH;                                             // 9600 floats = 37.5 KB per buffer

__global__ void __launch_bounds__(512) conv_fwd_halo4_dskip_kernel(HaloFwdArgs a) {
    constexpr int kRing = 8;
    extern __shared__ __attribute__((aligned(16))) float halo[];  // [2][k4CC][k4sCH]
    lds_float* const hl = (lds_float*)halo;
    const int n = blockIdx.x, co0 = blockIdx.y * 64;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kh2 = wave >> 2, wr = wave & 3, col = lane & 15, kq = lane >> 4;
    const int oh = col >> 2, ow = col & 3;
    const int lanebase = oh * k4sPAIR + (kq & 1) * k4sWODD + (kq >> 1) + ow;   // + (2 od + kd) * PLANE + k4s_row(kh)

    f32x4 acc[4];
#pragma unroll
    for (int od = 0; od < 4; ++od)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[od][v] = 0.f;

    // zero both buffers once: the halo padding is never written again
    for (int e = tid; e < 2 * k4sBUF; e += 512) hl[e] = 0.f;

    const lds_float* bb[2][4];   // (buffer, own channel)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            bb[b][c] = hl + b * k4sBUF + (kh2 * 4 + c) * k4sCH + lanebase;
            pin_vgpr(bb[b][c]);
        }
    const int G = a.Cin * 4;   // groups (ci, kd) of one 16-row tile
    const __amdgpu_buffer_rsrc_t wres = make_rsrc(a.wp + ((long)(co0 / 16 + wr) * G) * 64);
    const unsigned wvoff = lane * 16;

    // copy: a channel is 512 contiguous floats; thread t moves element t of each of the stage's 8 channels
    const int I3 = 512;
    const __amdgpu_buffer_rsrc_t xres = make_rsrc(a.x + ((long)n * a.g.Cx) * I3);
    unsigned xvoff = tid * 4;
    lds_float* sdst = hl + ((tid >> 6) + 1) * k4sPLANE + k4s_row(((tid >> 3) & 7) + 1) + (((tid & 7) + 1) & 1) * k4sWODD +
                      (((tid & 7) + 1) >> 1);
    pin_vgpr(xvoff);
    pin_vgpr(sdst);
    float fv[k4CC];
    __syncthreads();   // zero fill done before the first real voxels land
#pragma unroll
    for (int c = 0; c < k4CC; ++c) fv[c] = buf_load(xres, xvoff, c * (I3 * 4));
    // weight groups of this wave in order: stage s, own channel c, kd -> group (s*8 + kh2*4 + c)*4 + kd = s*32 + kh2*16 + (c*4 + kd)
    const int nstage = a.Cin / k4CC, nq = nstage * 16;
    auto group_of = [&](int q) {
        q = q < nq ? q : nq - 1;
        return (q >> 4) * 32 + kh2 * 16 + (q & 15);
    };
    float4 aring[kRing];
#pragma unroll
    for (int u = 0; u < kRing; ++u) aring[u] = buf_load4(wres, wvoff, (unsigned)group_of(u) * 1024u);
#pragma unroll
    for (int c = 0; c < k4CC; ++c) sdst[c * k4sCH] = fv[c];
    __syncthreads();

    int qbase = kRing;
    // B fragments of step (c, kd, kh): plane od at bb[c][(2 od + kd) * PLANE + k4s_row(kh)], read one step ahead; the dead tile's
    // register is never loaded and never used
    auto stage = [&](auto tag, int s) __attribute__((always_inline)) {
        constexpr int CUR = decltype(tag)::value, NXT = CUR ^ 1;
        int cnext = (s + 1) * k4CC;
        cnext = cnext > a.Cin - k4CC ? a.Cin - k4CC : cnext;
        const unsigned xs = (unsigned)cnext * (I3 * 4);
        float bq[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int od = 1; od < 4; ++od) bq[od] = bb[CUR][0][(2 * od) * k4sPLANE];   // step (0, kd 0, kh 0): od 0 is dead
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int gidx = 0; gidx < 16; ++gidx) {
            const int kd = gidx & 3;
            const float4 a_cur = aring[gidx % kRing];
            aring[gidx % kRing] = buf_load4(wres, wvoff, (unsigned)group_of(qbase + gidx) * 1024u);
            // copy of the next box: channel c is loaded in group c and stored in group c + 8
#pragma unroll
            for (int c = 0; c < k4CC; ++c) {
                if (c + 8 == gidx) sdst[NXT * k4sBUF + c * k4sCH] = fv[c];
                if (c == gidx) fv[c] = buf_load(xres, xvoff, xs + c * (I3 * 4));
            }
            const float av[4] = {a_cur.x, a_cur.y, a_cur.z, a_cur.w};   // kh
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float b[4];
#pragma unroll
                for (int od = 0; od < 4; ++od) b[od] = bq[od];
                const int tn = gidx * 4 + k + 1;   // the next step
                if (tn < 64) {
                    const int kdn = (tn >> 2) & 3, kn = tn & 3;
                    const lds_float* hb = bb[CUR][tn >> 4];
#pragma unroll
                    for (int od = 0; od < 4; ++od) {
                        if ((od == 0 && kdn == 0) || (od == 3 && kdn == 3)) continue;
                        bq[od] = hb[(2 * od + kdn) * k4sPLANE + k4s_row(kn)];
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                // consecutive MFMAs go to different accumulators (40-cycle dependent latency against a 32-cycle issue)
#pragma unroll
                for (int od = 0; od < 4; ++od) {
                    if ((od == 0 && kd == 0) || (od == 3 && kd == 3)) continue;
                    acc[od] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[k], b[od], acc[od], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        qbase += 16;
        __syncthreads();
    };
    for (int s = 0; s + 1 < nstage; s += 2) {
        stage(IntTag<0>(), s);
        stage(IntTag<1>(), s + 1);
    }
    if (nstage & 1) stage(IntTag<0>(), nstage - 1);

    // the K halves meet in LDS (the boxes are dead after the last barrier): waves 4-7 park, waves 0-3 add and store
    float* red = halo + (wr * 16) * 64;
    if (kh2 == 1) {
#pragma unroll
        for (int od = 0; od < 4; ++od)
#pragma unroll
            for (int v = 0; v < 4; ++v) red[(od * 4 + v) * 64 + lane] = acc[od][v];
    }
    __syncthreads();
    if (kh2 == 1) return;
    // y[n][co][p], p = od*16 + oh*4 + ow: 16 consecutive floats per (co, plane)
    float* yo = a.y + (long)n * a.Cout * 64 + col;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int co = co0 + wr * 16 + 4 * kq + v;
        if (co < a.Cout) {
            const float bv = a.bias ? a.bias[co] : 0.f;
#pragma unroll
            for (int od = 0; od < 4; ++od)
                yo[(long)co * 64 + od * 16] = sg_apply_act(acc[od][v] + red[(od * 4 + v) * 64 + lane] + bv, a.act, a.slope);
        }
    }
}

size_t halo_fwd_workspace_bytes(int Cin, int Cout) { return (size_t)((Cout + 127) / 128) * 128 * Cin * 64 * sizeof(float); }

HaloFwdForm halo_fwd_form_decode(int debug) {
    HaloFwdForm f;
    f.forced = true;
    f.variant = (debug >> 4) & 3;
    f.keep_lds = (debug & 64) != 0;
    f.keep_rows128 = (debug & 128) != 0;
    f.dskip = (debug & 256) != 0;
    return f;
}

// 4^3 outputs: the whole-sample box kernel (8-channel stages, 64-row tiles)
static HaloFwdPlan halo_fwd4_plan(int batch, int Cin, int Cout, const ConvGeom& g, size_t workspace_bytes, const HaloFwdForm& form) {
    HaloFwdPlan p = HaloFwdPlan();
    const size_t image_bytes = halo_fwd_workspace_bytes(Cin, Cout);
    if (Cin % k4CC != 0 || Cin < 2 * k4CC || Cout < 32) return p;
    if (workspace_bytes < image_bytes) return p;
    if ((long)g.Cx * 512 * 4 >= (long)kBufRange || (long)Cin * 8 * 1024 >= (long)kBufRange || batch > 65535 * 16) return p;
    const int mtiles = sg_cdiv(Cout, 64);
    // (one round of workgroups costs ~130 us at 128 -> 256 channels whatever its size; the split-K gather kernel is faster
    // below ~160 of them: 113 vs 132 us at 32 samples, 195 vs 129 us at 48 — scripts/small_batch_ab2.py, round 4)
    // Below that, the input channels are split over 2 - 8 workgroups per (sample, row tile) that write partial sums behind the image
    // (finished by the caller with the gather kernel's split-K finalize): 256 workgroups of 4+ stages each
    int csplit = 1;
    if (!form.forced && (long)batch * mtiles < 160) {
        while (csplit < kHaloFwd4MaxSplit && (long)batch * mtiles * csplit < 256 && (Cin / (2 * csplit)) % k4CC == 0 &&
               Cin / (2 * csplit) >= 2 * k4CC)
            csplit *= 2;
        if (csplit == 1) return p;
        if (workspace_bytes < image_bytes + (size_t)csplit * Cout * batch * 64 * sizeof(float)) return p;
    }
    // Depth-skip form (conv_fwd_halo4_dskip_kernel) or conv_fwd_halo4_kernel: they read different weight images (job kinds 2, 0).
    // Forced calls (tests, A/B) get the depth-skip form only where they ask for it.  The dispatch takes it wherever the input channels
    // are not split over workgroups (csplit > 1: small batches) — measured faster at 64 and 128 samples.
    const bool dskip = (form.dskip || !form.forced) && csplit == 1;
    if (form.dskip && !dskip) return p;
    p.served = true;
    p.kernel = dskip ? HaloFwdKernel::halo4_dskip : HaloFwdKernel::halo4;
    p.grid = dskip ? dim3((unsigned)batch, mtiles) : dim3((unsigned)batch, mtiles, csplit);
    p.block = 512;
    p.lds = dskip ? (size_t)2 * k4sBUF * sizeof(float)      // 75 KB
                  : (size_t)2 * k4BUF * sizeof(float);      // 66.5 KB: both above the default dynamic-LDS limit
    p.image = ImageJob{dskip ? 2 : 0, mtiles * 2, 0};
    p.nth = p.ntw = 1;
    p.csplit = csplit;
    p.partial_offset = image_bytes;
    p.workspace_need = image_bytes + (csplit > 1 ? (size_t)csplit * Cout * batch * 64 * sizeof(float) : 0);
    return p;
}

HaloFwdPlan halo_fwd_plan(int batch, int Cin, int Cout, const ConvGeom& g, size_t workspace_bytes, HaloFwdForm form) {
    if (g.OD == 4 && g.OH == 4 && g.OW == 4) return halo_fwd4_plan(batch, Cin, Cout, g, workspace_bytes, form);
    HaloFwdPlan p = HaloFwdPlan();
    if (form.dskip) return p;   // the depth-skip form exists for 4^3 outputs only
    // eligible: 8x8 position tiles exist, whole stages of 4 channels, enough output channels to fill 64-row MFMA tiles
    if (g.OW % 8 != 0 || g.OH % 8 != 0 || Cin % kCC != 0 || Cin < 8 || Cout < 32) return p;
    if ((long)g.Cx * g.ID * g.IH * g.IW * 4 >= (long)kBufRange || (long)Cin * 8 * 1024 >= (long)kBufRange) return p;
    if (workspace_bytes < halo_fwd_workspace_bytes(Cin, Cout)) return p;
    if ((long)batch * g.Cx * g.ID * g.IH * g.IW >= (1L << 31)) return p;
    // configuration: 128 output channels per workgroup as 8 waves x 1 tile (variant 0, more waves per SIMD to hide the
    // copy / weight-load latency) or 4 waves x 2 tiles (variant 1); 64 channels as 4 waves x 1 tile
    // measured (scripts/halo_bench.py of rounds 1-3: git history): 4 waves x 2 tiles wins below ~1024 workgroups, 8 waves x 1 tile above
    int variant = form.variant;
    int rows = (Cout > 64 && variant != 3) ? 128 : 64;   // variant 3: 64-row tiles, twice the workgroups
    const int ntw = g.OW / 8, nth = g.OH / 8;
    const long tiles = (long)batch * g.OD * nth * ntw;
    // Small grids (round 4, scripts/small_batch_ab2.py; the critics of the hybrid GANs see 16 - 32 samples): a round of <= 256
    // workgroups costs the same whatever its size (64 -> 128 channels at 16^3: ~125 us with 128-row tiles, ~70 us with 64-row
    // tiles), so with 128-row tiles at most half a round (W <= 128) or just over one (256 < W <= 384) the 64-row tiles are chosen:
    // 16 samples 125 -> 71 us (the gather kernel: 104), 40 samples 238 -> 186 us.  Same weight image (row tiles of 32).
    if (rows == 128 && variant == 0 && !form.keep_rows128) {
        const long w128 = tiles * sg_cdiv(Cout, 128);
        if (w128 <= 128 || (w128 > 256 && w128 <= 384)) rows = 64;
    }
    const int mtiles = sg_cdiv(Cout, rows);
    // auto-dispatch only where it wins (A/B on MI355X): from three quarters of a round of workgroups on; below that the
    // split-K gather kernel is faster (8 samples at 64 -> 128 channels, 16^3: 63 vs 70 us; 12 samples: 103 vs 70 us; with 128-row
    // tiles, 20 samples = 160 workgroups: 126 vs 156 us)
    if (!form.forced && tiles * mtiles < (rows == 128 ? 144 : 192)) return p;
    if (tiles >= (1L << 31)) return p;
    if (variant == 0) variant = 2;   // 1 = 4 waves x (32 rows x 64 positions), 2 = 8 waves x (32 x 32): measured 143-146 vs 139-143 TF
    p.lds = (size_t)2 * kCC * kHS * sizeof(float);
    // Registers and LDS would admit 3 workgroups per CU; with fewer than ~4 rounds of workgroups that leaves a mostly
    // idle last round (1024 workgroups: 768 + 256), so ask for enough LDS to cap the CU at 2 (form.keep_lds: don't)
    if (tiles * mtiles < 256 * 3 * 4 && !form.keep_lds && p.lds < 56 * 1024) p.lds = 56 * 1024;
    p.served = true;
    p.kernel = rows == 64 ? HaloFwdKernel::rows64 : (variant == 2 ? HaloFwdKernel::rows128_w8 : HaloFwdKernel::rows128_w4);
    p.grid = dim3((unsigned)tiles, mtiles);
    p.block = p.kernel == HaloFwdKernel::rows128_w8 ? 512 : 256;
    p.image = ImageJob{0, mtiles * rows / 32, 0};  // every row tile a workgroup may touch exists (zero rows beyond Cout)
    p.nth = nth;
    p.ntw = ntw;
    p.csplit = 1;
    p.partial_offset = p.workspace_need = halo_fwd_workspace_bytes(Cin, Cout);
    return p;
}

void halo_fwd_pack(const HaloFwdPlan& p, const float* w, int Cin, int Cin_total, int Cout, void* workspace, hipStream_t stream) {
    const long total = (long)p.image.nt * Cin * 8 * 64;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pack_fwd_weights_kernel, dim3(blocks), dim3(256), 0, stream, w, workspace_at<float4>(workspace, p.image.offset), Cout,
                       Cin_total, Cin, p.image.nt, p.image.kind >> 1);
}

static HaloFwdArgs halo_fwd_args(const HaloFwdPlan& p, const float* x, const float* bias, float* y, int batch, int Cin, int Cout,
                                 const ConvGeom& g, int act, float slope, void* workspace) {
    const bool box4 = p.kernel == HaloFwdKernel::halo4 || p.kernel == HaloFwdKernel::halo4_dskip;
    HaloFwdArgs a;
    a.x = x;
    a.wp = workspace_at<float4>(workspace, p.image.offset);
    a.bias = bias;
    a.y = y;
    a.g = g;
    a.Cin = Cin;
    a.Cout = Cout;
    a.nth = p.nth;
    a.ntw = p.ntw;
    a.dntw = FastDiv(p.ntw);
    a.dnth = FastDiv(p.nth);
    a.dOD = FastDiv(box4 ? 1 : g.OD);
    a.act = act;
    a.slope = slope;
    a.csplit = p.csplit;
    a.partial = workspace_at<float>(workspace, p.partial_offset);
    a.npos = (long)batch * g.O3();
    return a;
}

void halo_fwd_launch(const HaloFwdPlan& p, const float* x, const float* bias, float* y, int batch, int Cin, int Cout, const ConvGeom& g,
                     int act, float slope, void* workspace, hipStream_t stream) {
    const HaloFwdArgs a = halo_fwd_args(p, x, bias, y, batch, Cin, Cout, g, act, slope, workspace);
    if (p.kernel == HaloFwdKernel::halo4 || p.kernel == HaloFwdKernel::halo4_dskip) {
        static SgPerDeviceOnce attr_once;   // > 48 KB of dynamic LDS needs the attribute once per DEVICE
        if (attr_once.begin()) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_fwd_halo4_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)2 * k4BUF * sizeof(float)));
            attr_once.end();
        }
    }
    switch (p.kernel) {
    case HaloFwdKernel::halo4_dskip: {
        static SgPerDeviceOnce attr_once_s;
        if (attr_once_s.begin()) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv_fwd_halo4_dskip_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
            attr_once_s.end();
        }
        hipLaunchKernelGGL(conv_fwd_halo4_dskip_kernel, p.grid, dim3(p.block), p.lds, stream, a);
        break;
    }
    case HaloFwdKernel::halo4:
        hipLaunchKernelGGL(conv_fwd_halo4_kernel, p.grid, dim3(p.block), p.lds, stream, a);
        break;
    case HaloFwdKernel::rows128_w8:
        hipLaunchKernelGGL((conv_fwd_halo_kernel<1, 8>), p.grid, dim3(p.block), p.lds, stream, a);
        break;
    case HaloFwdKernel::rows128_w4:
        hipLaunchKernelGGL((conv_fwd_halo_kernel<2, 4>), p.grid, dim3(p.block), p.lds, stream, a);
        break;
    case HaloFwdKernel::rows64:
        hipLaunchKernelGGL((conv_fwd_halo_kernel<1, 4>), p.grid, dim3(p.block), p.lds, stream, a);
        break;
    }
}



// ================================================================================================================
// dgrad form (nn.Conv3d input-gradient, nn.ConvTranspose3d forward) with the same data movement.
//   dx[n,ci,2q+p] = sum_{co,t in {0,1}^3} W[co,ci,tap(p,t)] * dy[n,co,q+p-t],   tap = 1 - p + 2t per dimension
// One workgroup = one output parity p (grid z) x 64 input channels x a 2x8x8 box of q (128 positions).  Per stage it
// copies the (2+1)x9x9 box of dy it needs for 16 output channels into LDS (dense, index = copy index), B fragments are
// read from the box with immediate offsets (the tap shift (1-td)*81 + (1-th)*9 is a compile-time constant per k-step),
// A fragments come from a per-parity packed weight image.  K per channel is 8 = one k-group.
// MODE 0: one sample, q box 2x8x8 -> dy box 3x9x9 per channel (O >= 8).  MODE 1: O = 4: the whole 4x4x4 grid of TWO
// samples -> dy box 2 x 5x5x5 per channel.  Both give 128 positions and ~245 box floats per channel.
template <int MODE>
struct DBox;
template <>
struct DBox<0> {
    static constexpr int BH = 9, BW = 9, PL = 81, CH = 243, TNOFF = 36, WNOFF = 81;
};
template <>
struct DBox<1> {
    static constexpr int BH = 5, BW = 5, PL = 25, CH = 250, TNOFF = 50, WNOFF = 125;
};
// 16 channels per stage (32 measured 3 % slower): a stage copies 16 * ~245 box floats = 16 elements per thread into an
// LDS buffer of 16*256 floats.

struct HaloDgradArgs {
    const float* dy;
    const float4* wp;   // [8 parities][Cin_pad/32][Cout][64 lanes] float4
    const float* bias;
    float* dx;
    ConvGeom g;
    int Cin, Cout, mtiles, batch;  // mtiles = row tiles (of 64) per parity
    int ppw;                       // output parities per workgroup (1, 2, 4, 8)
    FastDiv dntw, dnth, dntd;
    int act;
    float slope;
};

// Element e of an input-gradient weight image, tap(p, t) = 1 - p + 2t per dimension.
// mode 0: wp[((p*MT + mt)*Cout + co)*64 + lane] = float4{ W[co][mt*32 + (lane&31)][tap(p, t = 2j + (lane>>5))], j = 0..3 }
// mode 1 (conv_dgrad_halo_dskip_kernel, 16x16x4): the same index, float4{ W[co][mt*32 + 16*(j&1) + (lane&15)][tap(p, td = j>>1,
//         th = lane>>5, tw = (lane>>4)&1)], j = 0..3 } — the same size
__device__ __forceinline__ float4 dgrad_image_element(const float* __restrict__ w, long e, int Cout, int Cin_total, int Cin, int MT,
                                                      int mode) {
    const int lane = (int)(e & 63);
    long q = e >> 6;
    const int co = (int)(q % Cout);
    q /= Cout;
    const int mt = (int)(q % MT);
    const int p = (int)(q / MT);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ci = mode == 0 ? mt * 32 + (lane & 31) : mt * 32 + 16 * (j & 1) + (lane & 15);
        const int t = mode == 0 ? 2 * j + (lane >> 5) : 4 * (j >> 1) + (lane >> 4);   // t = 4 td + 2 th + tw
        if (ci < Cin) {
            const int kd = 1 - ((p >> 2) & 1) + 2 * ((t >> 2) & 1);
            const int kh = 1 - ((p >> 1) & 1) + 2 * ((t >> 1) & 1);
            const int kw = 1 - (p & 1) + 2 * (t & 1);
            v[j] = w[((long)co * Cin_total + ci) * 64 + kd * 16 + kh * 4 + kw];
        }
    }
    return make_float4(v[0], v[1], v[2], v[3]);
}
__global__ void __launch_bounds__(256) pack_dgrad_frag_kernel(const float* __restrict__ w, float4* __restrict__ wp,
                                                              int Cout, int Cin_total, int Cin, int MT, int mode) {
    const long total = 8L * MT * Cout * 64;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256)
        wp[e] = dgrad_image_element(w, e, Cout, Cin_total, Cin, MT, mode);
}

// ---- several weight images in ONE launch ------------------------------------------------------------------------------------
// A critic update packs four images of two weights (forward and input-gradient form each), one launch of 5 - 7 us apiece: 0.19 ms
// of the 16.8 ms WGAN step in thirty launches.  sg_conv3d_k4s2p1_pack_images (conv3d.hip) takes the image jobs of
// halo_fwd_plan / halo_dgrad_plan — the plans the calls themselves will make — and this kernel does all of them at once
// (grid y = job); the convolutions that follow are told their image is in place.
// Job kinds: 0 / 2 forward image mode 0 / 1, 1 / 3 input-gradient image mode 0 / 1.
__global__ void __launch_bounds__(256) pack_images_kernel(PackJobs jobs) {
    const PackJob& j = jobs.job[blockIdx.y];
    float4* __restrict__ wp = j.wp;
    const float* __restrict__ w = j.w;
    if ((j.kind & 1) == 0) {    // pack_fwd_weights_kernel
        const long total = (long)j.nt * j.Cin * 8 * 64;
        for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256)
            wp[e] = fwd_image_element(w, e, j.Cout, j.Cin_total, j.Cin, j.kind >> 1);
    } else {                    // pack_dgrad_frag_kernel
        const long total = 8L * j.nt * j.Cout * 64;
        for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256)
            wp[e] = dgrad_image_element(w, e, j.Cout, j.Cin_total, j.Cin, j.nt, j.kind >> 1);
    }
}
int halo_pack_jobs_launch(const PackJobs& jobs, hipStream_t stream) {
    if (jobs.n <= 0) return 0;
    hipLaunchKernelGGL(pack_images_kernel, dim3(1024, jobs.n), dim3(256), 0, stream, jobs);
    return jobs.n;
}

// R32 (Cin <= 32: the progressive discriminator's 32-channel stage, model/progressive_gan.py:38): only the first 32 rows of the
// 64-row tile exist, so instead of two waves multiplying an empty row block the four waves share row block 0 and take ONE of the
// workgroup's four column tiles each — half the MFMAs per workgroup, none of them on padding.
template <int MODE, bool R32>
__device__ __forceinline__ void conv_dgrad_halo_body(HaloDgradArgs a) {
    constexpr int NTN = R32 ? 1 : 2;      // column tiles per wave
    constexpr int kDCC = 16, kDNF = 16, kDBUF = kDNF * 256;   // channels per stage = copy elements per thread; floats per LDS buffer
    using BX = DBox<MODE>;
    constexpr int kDB = BX::CH;
    extern __shared__ __attribute__((aligned(16))) float box[];  // [2][kDBUF], a buffer = [kDCC][kDB] + tail
    uint32_t twi = 0, thi = 0, tdi = 0, n, q1, q2;
    if (MODE == 0) {
        a.dntw.divmod(blockIdx.x, q1, twi);
        a.dnth.divmod(q1, q2, thi);
        a.dntd.divmod(q2, n, tdi);
    } else {
        n = blockIdx.x * 2;  // first sample of the pair
    }
    const int qd0 = tdi * 2, qh0 = thi * 8, qw0 = twi * 8;
    const int ci0 = blockIdx.y * (R32 ? 32 : 64);      // (R32: grid y counts 32-row tiles)

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = R32 ? 0 : wave >> 1, wn = wave & 1, r = lane & 31, kpar = lane >> 5;
    const int tnf = R32 ? wave >> 1 : 0;      // R32: this wave's column tile
    // lane -> position inside a 32-position column tile; address of tap (td,th): lanebase + tn*TNOFF + (1-td)*PL + (1-th)*BW
    const int lpart = MODE == 0 ? (r >> 3) * BX::BW + (r & 7) : (r >> 4) * BX::PL + ((r >> 2) & 3) * BX::BW + (r & 3);
    const int lanebase = wn * BX::WNOFF + tnf * BX::TNOFF + lpart + 1 - kpar;

    f32x16 acc[NTN];
#pragma unroll
    for (int t = 0; t < NTN; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;

    // No VALU work in the stage loop (see the addressing helpers above): buffer loads for dy and the weight image, one
    // pinned LDS read address per (buffer, channel), stage loop unrolled by the buffer index.
    lds_float* const bl = (lds_float*)box;
    const lds_float* bb[2][kDCC];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int c = 0; c < kDCC; ++c) {
            bb[b][c] = bl + b * kDBUF + c * kDB + lanebase;
            pin_vgpr(bb[b][c]);
        }
    lds_float* sdst = bl + tid;   // element f of a stage goes to sdst[256 f] (+ buffer)
    pin_vgpr(sdst);

    // A workgroup walks a.ppw output parities back to back (grid z = 8 / ppw): the copy / weight pipelines run straight
    // through the parity boundaries, so only the first box load of the workgroup is exposed and the stores of a parity
    // overlap the next one's MFMAs (one parity is only Cout/16 stages long).
    const int G = a.Cout;  // one k-group per output channel
    const int par0 = blockIdx.z * a.ppw, par_end = par0 + a.ppw;
    const unsigned par_bytes = (unsigned)(a.mtiles * 2) * (unsigned)G * 1024u;   // weight image: [parity][row tile][G][64] float4
    const __amdgpu_buffer_rsrc_t wres = make_rsrc(a.wp + ((long)(R32 ? blockIdx.y : blockIdx.y * 2 + wm) * G) * 64);
    const unsigned wvoff = lane * 16;

    // ---- copy bookkeeping: element f of a stage is box index e = tid + 256 f, dense (ci, [sample,] hd, hh, hw); a buffer
    // holds kDNF*256 floats, so every thread stores all its elements (those beyond the box land in the unread tail).
    // The box of parity p starts at q0 + p - 1 in every dimension: against parity 0 the whole box moves by a SCALAR
    // (it goes into the load's scalar offset), and an element is padding only through three edge conditions per
    // dimension pair (low edge with p = 0, high edge with p = 1).  Each element keeps one word: offset for parity 0
    // (biased so that it is never negative, < 2^26) | its edge classes in bits 26..31; the word AND (parity flags |
    // 0x03ffffff) is the load offset, >= num_records (2^26) exactly for padding: 16 v_and per parity change. ----
    const int O3 = a.g.OD * a.g.OH * a.g.OW;
    const int obias = (a.g.OH + 1) * a.g.OW + 1;   // elements: parity 0 reaches one plane + row + column before q0
    const __amdgpu_buffer_rsrc_t dres = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.dy + (long)n * a.g.Cy * O3 - obias), 0, 1 << 26, 0x00020000);
    const unsigned chan_bytes = (unsigned)O3 * 4u;
    unsigned gword[kDNF], goff[kDNF];
#pragma unroll
    for (int f = 0; f < kDNF; ++f) {
        const int e = tid + 256 * f;
        const int ci = e / kDB;
        int rem = e - ci * kDB, smp = 0;
        if (MODE == 1) {
            smp = rem / 125;
            rem -= smp * 125;
        }
        const int hd = rem / BX::PL, hh = (rem - hd * BX::PL) / BX::BW, hw = rem % BX::BW;
        const int od = qd0 - 1 + hd, oh = qh0 - 1 + hh, ow = qw0 - 1 + hw;   // parity 0; parity bit p adds p
        const bool never = e >= kDCC * kDB || (int)n + smp >= a.batch;
        const unsigned cls = (od < 0 ? 1u << 26 : 0u) | (od + 1 >= a.g.OD ? 1u << 27 : 0u) | (oh < 0 ? 1u << 28 : 0u) |
                             (oh + 1 >= a.g.OH ? 1u << 29 : 0u) | (ow < 0 ? 1u << 30 : 0u) | (ow + 1 >= a.g.OW ? 1u << 31 : 0u);
        const int off0 = (smp * a.g.Cy + ci) * O3 + (od * a.g.OH + oh) * a.g.OW + ow + obias;   // >= 0
        gword[f] = never ? 0xffffffffu : ((unsigned)off0 * 4u) | cls;
        pin_vgpr(gword[f]);
    }
    unsigned pshift = 0;   // scalar byte offset of the current parity's box against parity 0
    auto set_goff = [&](int par) __attribute__((always_inline)) {
        const int pd = (par >> 2) & 1, ph = (par >> 1) & 1, pw = par & 1;
        // low-edge classes (bits 26,28,30) are padding when p = 0, high-edge classes (27,29,31) when p = 1
        const unsigned mask = 0x03ffffffu | (pd ? 1u << 27 : 1u << 26) | (ph ? 1u << 29 : 1u << 28) | (pw ? 1u << 31 : 1u << 30);
#pragma unroll
        for (int f = 0; f < kDNF; ++f) goff[f] = gword[f] & mask;
        pshift = (unsigned)((pd * a.g.OH + ph) * a.g.OW + pw) * 4u;
    };
    const long I3 = (long)a.g.ID * a.g.IH * a.g.IW;
    // stores: buffer resource on the wave's sample, one lane offset per column tile (position of parity 0 + the kpar row),
    // everything else (row block of 4 channels, parity shift) in the scalar offset
    const int nn = MODE == 0 ? (int)n : (int)n + wn;
    const __amdgpu_buffer_rsrc_t ores = make_rsrc(a.dx + (long)(nn < a.batch ? nn : 0) * a.g.Cx * I3);
    const __amdgpu_buffer_rsrc_t bres = make_rsrc(a.bias ? a.bias : a.dx);
    unsigned ovoff[NTN];
#pragma unroll
    for (int tn = 0; tn < NTN; ++tn) {
        int qd, qh, qw;
        if (MODE == 0) {
            qd = qd0 + wn;
            qh = qh0 + (tnf + tn) * 4 + (r >> 3);
            qw = qw0 + (r & 7);
        } else {
            qd = 2 * (tnf + tn) + (r >> 4);
            qh = (r >> 2) & 3;
            qw = r & 3;
        }
        ovoff[tn] = (unsigned)(((2 * qd) * a.g.IH + 2 * qh) * a.g.IW + 2 * qw + 4 * kpar * (int)I3) * 4u;
        pin_vgpr(ovoff[tn]);
    }
    const unsigned bvoff = kpar * 16;
    // Output parities pw = 0 and pw = 1 interleave at 4 bytes in dx: written by two parity passes, every 32-byte sector of dx was
    // half-written twice and the memory side filled each partial write from HBM (round 4 counters: 268 MB written and 379 MB
    // fetched for a 134 MB output).  A workgroup that walks both (ppw >= 2: parities 2k and 2k + 1 are consecutive) keeps the
    // finished values of pw = 0 in registers and completes them with pw = 1 to 8-byte pieces: a row of 8 (4) lanes writes 64
    // (32) contiguous bytes, half as many store instructions.
#ifdef SG_DGRAD_NO_PAIR      // ablation build (scripts/ab_build.sh): the 4-byte stores of rounds 1 - 4
    const bool paired = false;
#else
    const bool paired = a.ppw >= 2;
#endif
    float keep[NTN][16];
#pragma unroll
    for (int t = 0; t < NTN; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) keep[t][q] = 0.f;
    auto write_parity = [&](int par) __attribute__((always_inline)) {   // dx[n'][ci][2q + p] = act(acc + bias[ci]); acc = 0
        const int pd = (par >> 2) & 1, ph = (par >> 1) & 1, pw = par & 1;
        const unsigned oshift = (unsigned)((pd * a.g.IH + ph) * a.g.IW) * 4u;   // of the (pd, ph, pw = 0) element
        if (nn < a.batch) {
            if (paired && pw == 0) {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int cis = ci0 + wm * 32 + (q & 3) + 8 * (q >> 2);
                    const float bv = a.bias && cis < a.Cin ? buf_load(bres, bvoff, (unsigned)cis * 4u) : 0.f;
#pragma unroll
                    for (int tn = 0; tn < NTN; ++tn) keep[tn][q] = sg_apply_act(acc[tn][q] + bv, a.act, a.slope);
                }
            } else if (paired) {
                typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int cis = ci0 + wm * 32 + (q & 3) + 8 * (q >> 2);   // scalar part of the channel; the lane adds 4*kpar
                    if (cis < a.Cin) {   // Cin % 8 == 0: the whole 8-channel block is in or out
                        const float bv = a.bias ? buf_load(bres, bvoff, (unsigned)cis * 4u) : 0.f;
#pragma unroll
                        for (int tn = 0; tn < NTN; ++tn) {
                            u32x2 v;
                            v.x = __builtin_bit_cast(unsigned, keep[tn][q]);
                            v.y = __builtin_bit_cast(unsigned, sg_apply_act(acc[tn][q] + bv, a.act, a.slope));
                            __builtin_amdgcn_raw_buffer_store_b64(v, ores, (int)ovoff[tn], (int)((unsigned)cis * (unsigned)I3 * 4u + oshift), 0);
                        }
                    }
                }
            } else {
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int cis = ci0 + wm * 32 + (q & 3) + 8 * (q >> 2);
                    if (cis < a.Cin) {
                        const float bv = a.bias ? buf_load(bres, bvoff, (unsigned)cis * 4u) : 0.f;
#pragma unroll
                        for (int tn = 0; tn < NTN; ++tn) {
                            const float v = sg_apply_act(acc[tn][q] + bv, a.act, a.slope);
                            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ores, (int)ovoff[tn],
                                                                  (int)((unsigned)cis * (unsigned)I3 * 4u + oshift + 4u * pw), 0);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NTN; ++t)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
    };

    set_goff(par0);
    float fv[kDNF];
    constexpr int kRing = 8;   // <= kDCC: the ring never reaches past the next stage
    float4 aring[kRing];
    unsigned wcur = (unsigned)par0 * par_bytes;   // scalar byte offset of (parity, stage) in the weight image
#pragma unroll
    for (int f = 0; f < kDNF; ++f) fv[f] = buf_load(dres, goff[f], pshift);
#pragma unroll
    for (int u = 0; u < kRing; ++u) aring[u] = buf_load4(wres, wvoff, wcur + (unsigned)u * 1024u);
#pragma unroll
    for (int f = 0; f < kDNF; ++f) sdst[256 * f] = fv[f];
    __syncthreads();

    // The stage loop body is one basic block (no data-dependent branch): copy loads of the next box spread over the first
    // half of the stage, their LDS stores over the second half, packed weights in a ring of 8 groups; sched_barriers keep
    // the machine scheduler from sinking the loads to their uses (see conv_fwd_halo_kernel).
    constexpr int O00 = BX::PL + BX::BW, O01 = BX::PL, O10 = BX::BW, O11 = 0;  // (td,th) -> box offset
    const int nstage = a.Cout / kDCC;
    // dys: byte offset of the channels to copy (into the idle buffer) during this stage; wnext: weight offset of the stage
    // that follows.  Both are scalars computed by the caller, the body itself is branch-free.
    auto stage = [&](auto tag, unsigned dys, unsigned wnext) __attribute__((always_inline)) {
        constexpr int CUR = decltype(tag)::value, NXT = CUR ^ 1;
        float bq[NTN][4];
#pragma unroll
        for (int tn = 0; tn < NTN; ++tn) {
            const lds_float* hb = bb[CUR][0] + tn * BX::TNOFF;
            bq[tn][0] = hb[O00];   // j=0: td=0, th=0
            bq[tn][1] = hb[O01];   // j=1: td=0, th=1
            bq[tn][2] = hb[O10];   // j=2: td=1, th=0
            bq[tn][3] = hb[O11];   // j=3: td=1, th=1
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < kDCC; ++c) {  // one k-group per channel
            const float4 a_cur = aring[c % kRing];
            aring[c % kRing] = c + kRing < kDCC ? buf_load4(wres, wvoff, wcur + (unsigned)(c + kRing) * 1024u)
                                                : buf_load4(wres, wvoff, wnext + (unsigned)(c + kRing - kDCC) * 1024u);
            float b[NTN][4];
#pragma unroll
            for (int tn = 0; tn < NTN; ++tn)
#pragma unroll
                for (int j = 0; j < 4; ++j) b[tn][j] = bq[tn][j];
            if (c + 1 < kDCC) {
#pragma unroll
                for (int tn = 0; tn < NTN; ++tn) {
                    const lds_float* hb = bb[CUR][c + 1] + tn * BX::TNOFF;
                    bq[tn][0] = hb[O00];
                    bq[tn][1] = hb[O01];
                    bq[tn][2] = hb[O10];
                    bq[tn][3] = hb[O11];
                }
            }
            if (c < kDCC / 2) {  // copy of the next box: two loads per group in the first half of the stage ...
#pragma unroll
                for (int f = 2 * c; f < 2 * c + 2; ++f) fv[f] = buf_load(dres, goff[f], dys + pshift);
            } else {             // ... each value goes to LDS 8 groups after its load
#pragma unroll
                for (int f = 2 * (c - kDCC / 2); f < 2 * (c - kDCC / 2) + 2; ++f) sdst[NXT * kDBUF + 256 * f] = fv[f];
            }
            __builtin_amdgcn_sched_barrier(0);
            const float av[4] = {a_cur.x, a_cur.y, a_cur.z, a_cur.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int tn = 0; tn < NTN; ++tn) acc[tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], b[tn][j], acc[tn], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        wcur = wnext;
        __syncthreads();
    };
    for (int par = par0; par < par_end; ++par) {
        const bool more = par + 1 < par_end;
        // the stage after this parity's last one: the next parity's first (new box origin) or, at the very end, the last
        // stage again (copied into the idle buffer, never read)
        const unsigned wlast = more ? (unsigned)(par + 1) * par_bytes : (unsigned)par * par_bytes + (unsigned)(nstage - 1) * kDCC * 1024u;
        const unsigned dlast = more ? 0u : (unsigned)(nstage - 1) * kDCC * chan_bytes;
        int s = 0;
        for (; s + 1 < nstage; s += 2) {   // stages in pairs: the buffer index is a compile-time constant
            stage(IntTag<0>(), (unsigned)(s + 1) * kDCC * chan_bytes, wcur + kDCC * 1024u);
            const bool last = s + 2 == nstage;
            if (last && more) set_goff(par + 1);
            stage(IntTag<1>(), last ? dlast : (unsigned)(s + 2) * kDCC * chan_bytes, last ? wlast : wcur + kDCC * 1024u);
        }
        if (s < nstage) stage(IntTag<0>(), dlast, wlast);   // odd stage count: only with one parity per workgroup
        write_parity(par);
    }
}

template <int MODE>
__global__ void __launch_bounds__(256) conv_dgrad_halo_kernel(HaloDgradArgs a) {
    conv_dgrad_halo_body<MODE, false>(a);
}
template <int MODE>
__global__ void __launch_bounds__(256) conv_dgrad_halo32_kernel(HaloDgradArgs a) {
    conv_dgrad_halo_body<MODE, true>(a);
}

// ---- depth-skip form of conv_dgrad_halo_kernel<1> (4^3 -> 8^3, 64-row workgroups) -------------------------------------------
// Same workgroup (a pair of samples x 64 input channels x ppw parities), same dy boxes, same copy and weight pipelines, same
// stores; what changes is the MFMA: v_mfma_f32_16x16x4_f32 on 16-column tiles that are ONE depth plane qd (4 x 4 positions) of
// the wave's sample.  A wave (row block wm, sample wn) holds 2 row halves x 4 depth planes = 8 accumulators of 4 registers.
//   k = 4 of an MFMA is (th, tw) = (lane >> 5, (lane >> 4) & 1), td is the outer pair: per channel 2 td x 4 qd x 2 row halves.
//   The B fragment of (qd, td) is the box plane hd = qd + 1 - td at the lane's (qh + 1 - th, qw + 1 - tw): it depends on hd only,
//   so the five planes of a channel are read ONCE (one ds_read_b32 each) and serve both td and both row halves.
//   Plane hd is dy depth qd + pd - td: at output parity pd = 0 plane 0 is depth -1, at pd = 1 plane 4 is depth 4 — padding for
//   every sample, every stage and every wave.  The tile (qd 0, td 1) at pd = 0 and (qd 3, td 0) at pd = 1 is therefore not
//   issued and its plane not read: 14 MFMAs and 4 LDS reads per channel instead of 16 and 5.  pd is constant per parity pass: the
//   stage body is instantiated for both and chosen by a wave-uniform branch outside the stages, which stay one basic block.
//   LDS banks: a lane reads word (qh + 1 - th) * 5 + (qw + 1 - tw) + const of a 5 x 5 plane: 25 consecutive words, distinct
//   banks of the 32 (ds_read_b32: two groups of 32 lanes), equal addresses broadcast.
//   Accumulator of (row half rh, plane qd), register v, lane l: channel ci0 + wm*32 + rh*16 + 4*(l >> 4) + v at position
//   (qd, (l >> 2) & 3, l & 3).
// Semantics: the skipped products are weight x (zero padding of dy beyond the depth range).  For finite weights the result is
// that of the same sum with the zeros added; a non-finite weight on such a tap gives NaN (0 x inf) in conv_dgrad_halo_kernel<1>
// and the sum over the in-range positions here (as in the weight-gradient skip form).  The h / w padding is multiplied as before.
// Weight image: wp[((p*MT + mt)*Cout + co)*64 + lane] = float4{ W[co][mt*32 + rh*16 + (lane&15)][tap(p; td, th, tw)],
// (td, rh) = (0,0), (0,1), (1,0), (1,1) } — the size of the 32x32x2 image (pack mode 1 of pack_dgrad_frag_kernel).
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) conv_dgrad_halo_dskip_kernel(HaloDgradArgs a) {
    constexpr int kDCC = 16, kDNF = 16, kDBUF = kDNF * 256;
    using BX = DBox<1>;
    constexpr int kDB = BX::CH;
    extern __shared__ __attribute__((aligned(16))) float box[];  // [2][kDBUF], a buffer = [kDCC][kDB] + tail
    const uint32_t n = blockIdx.x * 2;  // first sample of the pair
    const int ci0 = blockIdx.y * 64;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1, col = lane & 15, kq = lane >> 4;
    const int qh = col >> 2, qw = col & 3, th = kq >> 1, tw = kq & 1;
    const int lanebase = wn * BX::WNOFF + (qh + 1 - th) * BX::BW + (qw + 1 - tw);   // + hd * PL: plane hd of the wave's sample

    f32x4 acc[2][4];   // (row half, depth plane)
#pragma unroll
    for (int rh = 0; rh < 2; ++rh)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd)
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[rh][qd][v] = 0.f;

    lds_float* const bl = (lds_float*)box;
    // one read address per lane; buffer, channel and plane are immediate offsets (at most 2*kDBUF floats = 32 KB < the 16-bit field)
    const lds_float* bb = bl + lanebase;
    pin_vgpr(bb);
    lds_float* sdst = bl + tid;   // element f of a stage goes to sdst[256 f] (+ buffer)
    pin_vgpr(sdst);

    const int G = a.Cout;  // one k-group per output channel
    const int par0 = blockIdx.z * a.ppw, par_end = par0 + a.ppw;
    const unsigned par_bytes = (unsigned)(a.mtiles * 2) * (unsigned)G * 1024u;   // weight image: [parity][row tile][G][64] float4
    const __amdgpu_buffer_rsrc_t wres = make_rsrc(a.wp + ((long)(blockIdx.y * 2 + wm) * G) * 64);
    const unsigned wvoff = lane * 16;

    // copy bookkeeping: exactly that of conv_dgrad_halo_body<1, false> (offset | edge-class words, see there)
    const int O3 = a.g.OD * a.g.OH * a.g.OW;
    const int obias = (a.g.OH + 1) * a.g.OW + 1;
    const __amdgpu_buffer_rsrc_t dres = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.dy + (long)n * a.g.Cy * O3 - obias), 0, 1 << 26, 0x00020000);
    const unsigned chan_bytes = (unsigned)O3 * 4u;
    unsigned gword[kDNF], goff[kDNF];
#pragma unroll
    for (int f = 0; f < kDNF; ++f) {
        const int e = tid + 256 * f;
        const int ci = e / kDB;
        int rem = e - ci * kDB;
        const int smp = rem / 125;
        rem -= smp * 125;
        const int hd = rem / BX::PL, hh = (rem - hd * BX::PL) / BX::BW, hw = rem % BX::BW;
        const int od = hd - 1, oh = hh - 1, ow = hw - 1;   // parity 0; parity bit p adds p
        const bool never = e >= kDCC * kDB || (int)n + smp >= a.batch;
        const unsigned cls = (od < 0 ? 1u << 26 : 0u) | (od + 1 >= a.g.OD ? 1u << 27 : 0u) | (oh < 0 ? 1u << 28 : 0u) |
                             (oh + 1 >= a.g.OH ? 1u << 29 : 0u) | (ow < 0 ? 1u << 30 : 0u) | (ow + 1 >= a.g.OW ? 1u << 31 : 0u);
        const int off0 = (smp * a.g.Cy + ci) * O3 + (od * a.g.OH + oh) * a.g.OW + ow + obias;   // >= 0
        gword[f] = never ? 0xffffffffu : ((unsigned)off0 * 4u) | cls;
        pin_vgpr(gword[f]);
    }
    unsigned pshift = 0;
    auto set_goff = [&](int par) __attribute__((always_inline)) {
        const int pd = (par >> 2) & 1, ph = (par >> 1) & 1, pw = par & 1;
        const unsigned mask = 0x03ffffffu | (pd ? 1u << 27 : 1u << 26) | (ph ? 1u << 29 : 1u << 28) | (pw ? 1u << 31 : 1u << 30);
#pragma unroll
        for (int f = 0; f < kDNF; ++f) goff[f] = gword[f] & mask;
        pshift = (unsigned)((pd * a.g.OH + ph) * a.g.OW + pw) * 4u;
    };
    const long I3 = (long)a.g.ID * a.g.IH * a.g.IW;
    // stores: buffer resource on the wave's sample, one lane offset per depth plane (position of parity 0 + the lane's row of the
    // 4-row block: 4 * kq channels), the accumulator's row block and the parity shift in the scalar offset
    const int nn = (int)n + wn;
    const __amdgpu_buffer_rsrc_t ores = make_rsrc(a.dx + (long)(nn < a.batch ? nn : 0) * a.g.Cx * I3);
    const __amdgpu_buffer_rsrc_t bres = make_rsrc(a.bias ? a.bias : a.dx);
    unsigned ovoff[4];
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
        ovoff[qd] = (unsigned)(((2 * qd) * a.g.IH + 2 * qh) * a.g.IW + 2 * qw + 4 * kq * (int)I3) * 4u;
        pin_vgpr(ovoff[qd]);
    }
    const unsigned bvoff = kq * 16;
    const int clim = a.Cin - 4 * kq;   // the lane's channel cis + 4 kq exists iff cis < clim (Cin % 8 == 0, a 16-row half may be cut)
    const bool paired = a.ppw >= 2;
    float keep[2][4][4];
#pragma unroll
    for (int rh = 0; rh < 2; ++rh)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd)
#pragma unroll
            for (int v = 0; v < 4; ++v) keep[rh][qd][v] = 0.f;
    auto write_parity = [&](int par) __attribute__((always_inline)) {   // dx[n'][ci][2q + p] = act(acc + bias[ci]); acc = 0
        const int pd = (par >> 2) & 1, ph = (par >> 1) & 1, pw = par & 1;
        const unsigned oshift = (unsigned)((pd * a.g.IH + ph) * a.g.IW) * 4u;   // of the (pd, ph, pw = 0) element
        if (nn < a.batch) {
#pragma unroll
            for (int rh = 0; rh < 2; ++rh)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int cis = ci0 + wm * 32 + rh * 16 + v;   // scalar part of the channel; the lane adds 4 * kq
                    if (cis < clim) {
                        const float bv = a.bias ? buf_load(bres, bvoff, (unsigned)cis * 4u) : 0.f;
                        const int soff = (int)((unsigned)cis * (unsigned)I3 * 4u + oshift);
#pragma unroll
                        for (int qd = 0; qd < 4; ++qd) {
                            const float val = sg_apply_act(acc[rh][qd][v] + bv, a.act, a.slope);
                            if (paired && pw == 0) {
                                keep[rh][qd][v] = val;
                            } else if (paired) {   // (pw 0, pw 1) as one 8-byte piece
                                typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                                u32x2 pr;
                                pr.x = __builtin_bit_cast(unsigned, keep[rh][qd][v]);
                                pr.y = __builtin_bit_cast(unsigned, val);
                                __builtin_amdgcn_raw_buffer_store_b64(pr, ores, (int)ovoff[qd], soff, 0);
                            } else {
                                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, val), ores, (int)ovoff[qd],
                                                                      soff + 4 * pw, 0);
                            }
                        }
                    }
                }
        }
#pragma unroll
        for (int rh = 0; rh < 2; ++rh)
#pragma unroll
            for (int qd = 0; qd < 4; ++qd)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[rh][qd][v] = 0.f;
    };

    set_goff(par0);
    float fv[kDNF];
    constexpr int kRing = 8;   // <= kDCC: the ring never reaches past the next stage
    float4 aring[kRing];
    unsigned wcur = (unsigned)par0 * par_bytes;   // scalar byte offset of (parity, stage) in the weight image
#pragma unroll
    for (int f = 0; f < kDNF; ++f) fv[f] = buf_load(dres, goff[f], pshift);
#pragma unroll
    for (int u = 0; u < kRing; ++u) aring[u] = buf_load4(wres, wvoff, wcur + (unsigned)u * 1024u);
#pragma unroll
    for (int f = 0; f < kDNF; ++f) sdst[256 * f] = fv[f];
    __syncthreads();

    const int nstage = a.Cout / kDCC;
    // One stage, one basic block; PD selects the four live planes H0 .. H0 + 3 and the dead (qd, td) tile at compile time.
    auto stage = [&](auto tag, auto pdtag, unsigned dys, unsigned wnext) __attribute__((always_inline)) {
        constexpr int CUR = decltype(tag)::value, NXT = CUR ^ 1, PD = decltype(pdtag)::value;
        constexpr int H0 = PD ? 0 : 1;
        float bq[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) bq[i] = bb[CUR * kDBUF + (H0 + i) * BX::PL];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < kDCC; ++c) {  // one k-group per channel
            const float4 a_cur = aring[c % kRing];
            aring[c % kRing] = c + kRing < kDCC ? buf_load4(wres, wvoff, wcur + (unsigned)(c + kRing) * 1024u)
                                                : buf_load4(wres, wvoff, wnext + (unsigned)(c + kRing - kDCC) * 1024u);
            float b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) b[i] = bq[i];
            if (c + 1 < kDCC) {
#pragma unroll
                for (int i = 0; i < 4; ++i) bq[i] = bb[CUR * kDBUF + (c + 1) * kDB + (H0 + i) * BX::PL];
            }
            if (c < kDCC / 2) {  // copy of the next box: two loads per group in the first half of the stage ...
#pragma unroll
                for (int f = 2 * c; f < 2 * c + 2; ++f) fv[f] = buf_load(dres, goff[f], dys + pshift);
            } else {             // ... each value goes to LDS 8 groups after its load
#pragma unroll
                for (int f = 2 * (c - kDCC / 2); f < 2 * (c - kDCC / 2) + 2; ++f) sdst[NXT * kDBUF + 256 * f] = fv[f];
            }
            __builtin_amdgcn_sched_barrier(0);
            const float av[2][2] = {{a_cur.x, a_cur.y}, {a_cur.z, a_cur.w}};   // [td][rh]
            // consecutive MFMAs go to different accumulators (40-cycle dependent latency against a 32-cycle issue)
#pragma unroll
            for (int td = 0; td < 2; ++td)
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    constexpr int kDead0 = 0, kDead1 = 4;   // the padding plane at pd = 0 / pd = 1
                    const int hd = qd + 1 - td;
                    if (hd == (PD ? kDead1 : kDead0)) continue;
#pragma unroll
                    for (int rh = 0; rh < 2; ++rh)
                        acc[rh][qd] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[td][rh], b[hd - H0], acc[rh][qd], 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
        wcur = wnext;
        __syncthreads();
    };
    auto run_parity = [&](auto pdtag, int par) __attribute__((always_inline)) {
        const bool more = par + 1 < par_end;
        // the stage after this parity's last one: the next parity's first (new box origin) or, at the very end, the last
        // stage again (copied into the idle buffer, never read)
        const unsigned wlast = more ? (unsigned)(par + 1) * par_bytes : (unsigned)par * par_bytes + (unsigned)(nstage - 1) * kDCC * 1024u;
        const unsigned dlast = more ? 0u : (unsigned)(nstage - 1) * kDCC * chan_bytes;
        int s = 0;
        for (; s + 1 < nstage; s += 2) {   // stages in pairs: the buffer index is a compile-time constant
            stage(IntTag<0>(), pdtag, (unsigned)(s + 1) * kDCC * chan_bytes, wcur + kDCC * 1024u);
            const bool last = s + 2 == nstage;
            if (last && more) set_goff(par + 1);
            stage(IntTag<1>(), pdtag, last ? dlast : (unsigned)(s + 2) * kDCC * chan_bytes, last ? wlast : wcur + kDCC * 1024u);
        }
        if (s < nstage) stage(IntTag<0>(), pdtag, dlast, wlast);   // odd stage count: only with one parity per workgroup
    };
    for (int par = par0; par < par_end; ++par) {
        if ((par >> 2) & 1)   // wave-uniform: pd of this parity pass
            run_parity(IntTag<1>(), par);
        else
            run_parity(IntTag<0>(), par);
        write_parity(par);
    }
}

// ---- depth-walk form of conv_dgrad_halo_kernel<0> (8^3 -> 16^3: dy grids with OD == 8, 64-row workgroups) ---------------------
// The same MFMA (32x32x2), dy boxes (3 x 9 x 9 per channel), copy and weight pipelines, weight image (mode 0) and paired stores as
// conv_dgrad_halo_body<0, false>; what changes is which work a workgroup and a wave own, so that the products with the DEPTH
// padding can be left out evenly.  Plane hd of a box is dy depth qd0 - 1 + hd + pd: depth -1 only for (plane pair 0, pd 0, hd 0)
// and depth 8 only for (plane pair 3, pd 1, hd 2) — the column tile of plane qd 0 with td 1, resp. of plane qd 7 with td 0: 2 of
// the 32 (plane, pd, td) combinations, 1/16 of the MFMAs.  In the present form they sit in one wave (wn = plane) of the tdi 0 / 3
// workgroups, where dropping them only makes that wave wait for its partners.  Here
//   one workgroup = (sample, 8 x 8 h/w tile, depth half hf = blockIdx.x & 1, output parity ph = blockIdx.z) x 64 input channels;
//   it walks the two plane pairs tdi = 2 hf, 2 hf + 1 of its half and for each (pd 0, pw 0), (pd 0, pw 1), (pd 1, pw 0), (pd 1, pw 1):
//   8 passes of Cout / 16 stages, pw 0 / 1 adjacent (8-byte stores), exactly one (plane pair, pd) of them on a depth edge:
//   (0, pd 0) for hf 0 — passes 0, 1 — and (3, pd 1) for hf 1 — passes 6, 7;
//   wave (wm, wn): row half wm, h half wn (qh 0-3 / 4-7) of the tile; its two column tiles tn are the two PLANES of the pair.
// In an edge pass the tile (tn 0, td 1) — low edge — or (tn 1, td 0) — high edge — is all padding for every wave alike: its B
// registers are not read and its MFMAs not issued (6 of 8 per channel remain) in 2 of 8 passes: every workgroup and every wave issues 15/16
// of the present form's MFMAs.  The stage body takes the edge as a compile-time tag (0 none, 1 low, 2 high), chosen per pass by a
// wave-uniform branch outside the stages, which stay one basic block.
// A B fragment depends on the box plane hd = tn + 1 - td only: (tn 0, td 0) and (tn 1, td 1) are the same two LDS words, so a channel
// costs 6 reads (3 ds_read2_b32) instead of 8, and 4 in an edge pass.  LDS read addresses: ONE register per lane with buffer, channel,
// plane and tap as immediate offsets (conv_dgrad_halo_dskip_kernel's scheme) instead of the 32 pinned addresses of
// conv_dgrad_halo_body — with those the kernel needs 276 registers and loses its second wave per SIMD.  The price is one v_add_u32
// per channel where the 8-bit offsets of the merged reads do not reach (against 6 - 8 MFMAs of 16 passes): the only VALU work of a stage.
// Compiler gate: 238 VGPR, no AGPR, scratch 0, no VGPR spill, 2 waves/SIMD; 55.0 KB of code (conv_dgrad_halo_kernel<0>: 65.8 KB), of
// which a workgroup runs four stage bodies (2 buffers x {inner, its edge}), against an instruction cache of 64 KB per two CUs.
// The box of the second plane pair lies 2 OH OW floats behind the first one's: a scalar, next to pshift.  The offset | edge-class
// words hold the offsets of the FIRST pair's box and the depth classes (bits 26, 27) of the workgroup's EDGE box (the first for
// hf 0, the second for hf 1); the inner box has no depth padding (OD == 8), its passes mask both depth bits off.
// Semantics: the k order of every accumulator is the present form's (co ascending, then j) and the dropped products have B = 0: for
// finite inputs the results are bit-equal up to the sign of a zero.  A non-finite weight on a tap that meets only depth padding
// gives NaN (0 x inf) in conv_dgrad_halo_kernel<0> and the sum over the in-range positions here, as in the other depth-skip forms.
// The h / w padding is multiplied as before.
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) conv_dgrad_halo_dwalk_kernel(HaloDgradArgs a) {
    constexpr int NTN = 2;
    constexpr int kDCC = 16, kDNF = 16, kDBUF = kDNF * 256;
    using BX = DBox<0>;
    constexpr int kDB = BX::CH;
    extern __shared__ __attribute__((aligned(16))) float box[];  // [2][kDBUF], a buffer = [kDCC][kDB] + tail
    const int hf = blockIdx.x & 1, ph = blockIdx.z;
    uint32_t twi, thi, n, q1;
    a.dntw.divmod(blockIdx.x >> 1, q1, twi);
    a.dnth.divmod(q1, n, thi);
    const int qd0 = hf * 4, qh0 = thi * 8, qw0 = twi * 8;      // qd0: the first plane pair of the half
    const int qd0e = hf ? a.g.OD - 2 : 0;                      // the plane pair on the depth edge
    const int ci0 = blockIdx.y * 64;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1, r = lane & 31, kpar = lane >> 5;
    // lane -> position inside a 32-position column tile (4 h x 8 w of plane tn); address of tap (td,th): lanebase + tn*PL + (1-td)*PL + (1-th)*BW
    const int lanebase = wn * BX::TNOFF + (r >> 3) * BX::BW + (r & 7) + 1 - kpar;

    f32x16 acc[NTN];
#pragma unroll
    for (int t = 0; t < NTN; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;

    lds_float* const bl = (lds_float*)box;
    // one read address per lane; buffer, channel, plane and tap are immediate offsets (at most 2*kDBUF floats = 32 KB < the 16-bit field)
    const lds_float* bb = bl + lanebase;
    pin_vgpr(bb);
    lds_float* sdst = bl + tid;   // element f of a stage goes to sdst[256 f] (+ buffer)
    pin_vgpr(sdst);

    const int G = a.Cout;  // one k-group per output channel
    const unsigned par_bytes = (unsigned)(a.mtiles * 2) * (unsigned)G * 1024u;   // weight image: [parity][row tile][G][64] float4
    const __amdgpu_buffer_rsrc_t wres = make_rsrc(a.wp + ((long)(blockIdx.y * 2 + wm) * G) * 64);
    const unsigned wvoff = lane * 16;

    // copy bookkeeping: that of conv_dgrad_halo_body<0, false> with the depth classes of the edge box (header comment)
    const int O3 = a.g.OD * a.g.OH * a.g.OW;
    const int obias = (a.g.OH + 1) * a.g.OW + 1;
    const __amdgpu_buffer_rsrc_t dres = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(a.dy + (long)n * a.g.Cy * O3 - obias), 0, 1 << 26, 0x00020000);
    const unsigned chan_bytes = (unsigned)O3 * 4u;
    const unsigned pair_bytes = (unsigned)(2 * a.g.OH * a.g.OW) * 4u;      // box origin of the second plane pair against the first
    unsigned gword[kDNF], goff[kDNF];
#pragma unroll
    for (int f = 0; f < kDNF; ++f) {
        const int e = tid + 256 * f;
        const int ci = e / kDB;
        const int rem = e - ci * kDB;
        const int hd = rem / BX::PL, hh = (rem - hd * BX::PL) / BX::BW, hw = rem % BX::BW;
        const int od = qd0 - 1 + hd, ode = qd0e - 1 + hd, oh = qh0 - 1 + hh, ow = qw0 - 1 + hw;   // parity 0; parity bit p adds p
        const bool never = e >= kDCC * kDB;
        const unsigned cls = (ode < 0 ? 1u << 26 : 0u) | (ode + 1 >= a.g.OD ? 1u << 27 : 0u) | (oh < 0 ? 1u << 28 : 0u) |
                             (oh + 1 >= a.g.OH ? 1u << 29 : 0u) | (ow < 0 ? 1u << 30 : 0u) | (ow + 1 >= a.g.OW ? 1u << 31 : 0u);
        const int off0 = ci * O3 + (od * a.g.OH + oh) * a.g.OW + ow + obias;   // >= 0
        gword[f] = never ? 0xffffffffu : ((unsigned)off0 * 4u) | cls;
        pin_vgpr(gword[f]);
    }
    // pass i = 0 .. 7: plane pair i >> 2, pd = (i >> 1) & 1, pw = i & 1
    unsigned pshift = 0;   // scalar byte offset of the current pass's box against (first pair, parity 0)
    auto set_goff = [&](int i) __attribute__((always_inline)) {
        const int pair = i >> 2, pd = (i >> 1) & 1, pw = i & 1;
        const bool dedge = pair == hf;
        const unsigned mask = 0x03ffffffu | (dedge ? (pd ? 1u << 27 : 1u << 26) : 0u) | (ph ? 1u << 29 : 1u << 28) | (pw ? 1u << 31 : 1u << 30);
#pragma unroll
        for (int f = 0; f < kDNF; ++f) goff[f] = gword[f] & mask;
        pshift = (unsigned)((pd * a.g.OH + ph) * a.g.OW + pw) * 4u + (unsigned)pair * pair_bytes;
    };
    const long I3 = (long)a.g.ID * a.g.IH * a.g.IW;
    // stores: one lane offset per plane of the FIRST pair (position of parity 0 + the kpar row); row block of 4 channels, parity and
    // plane-pair shift in the scalar offset
    const __amdgpu_buffer_rsrc_t ores = make_rsrc(a.dx + (long)n * a.g.Cx * I3);
    const __amdgpu_buffer_rsrc_t bres = make_rsrc(a.bias ? a.bias : a.dx);
    unsigned ovoff[NTN];
#pragma unroll
    for (int tn = 0; tn < NTN; ++tn) {
        const int qd = qd0 + tn, qh = qh0 + wn * 4 + (r >> 3), qw = qw0 + (r & 7);
        ovoff[tn] = (unsigned)(((2 * qd) * a.g.IH + 2 * qh) * a.g.IW + 2 * qw + 4 * kpar * (int)I3) * 4u;
        pin_vgpr(ovoff[tn]);
    }
    const unsigned bvoff = kpar * 16;
    const unsigned opair_bytes = (unsigned)(4 * a.g.IH * a.g.IW) * 4u;
    float keep[NTN][16];
#pragma unroll
    for (int t = 0; t < NTN; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) keep[t][q] = 0.f;
    auto write_pass = [&](int i) __attribute__((always_inline)) {   // dx[n][ci][2q + p] = act(acc + bias[ci]); acc = 0
        const int pair = i >> 2, pd = (i >> 1) & 1, pw = i & 1;
        const unsigned oshift = (unsigned)((pd * a.g.IH + ph) * a.g.IW) * 4u + (unsigned)pair * opair_bytes;   // of the (pd, ph, pw = 0) element
        if (pw == 0) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int cis = ci0 + wm * 32 + (q & 3) + 8 * (q >> 2);
                const float bv = a.bias && cis < a.Cin ? buf_load(bres, bvoff, (unsigned)cis * 4u) : 0.f;
#pragma unroll
                for (int tn = 0; tn < NTN; ++tn) keep[tn][q] = sg_apply_act(acc[tn][q] + bv, a.act, a.slope);
            }
        } else {      // (pw 0, pw 1) as one 8-byte piece
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int cis = ci0 + wm * 32 + (q & 3) + 8 * (q >> 2);   // scalar part of the channel; the lane adds 4*kpar
                if (cis < a.Cin) {   // Cin % 8 == 0: the whole 8-channel block is in or out
                    const float bv = a.bias ? buf_load(bres, bvoff, (unsigned)cis * 4u) : 0.f;
#pragma unroll
                    for (int tn = 0; tn < NTN; ++tn) {
                        u32x2 v;
                        v.x = __builtin_bit_cast(unsigned, keep[tn][q]);
                        v.y = __builtin_bit_cast(unsigned, sg_apply_act(acc[tn][q] + bv, a.act, a.slope));
                        __builtin_amdgcn_raw_buffer_store_b64(v, ores, (int)ovoff[tn], (int)((unsigned)cis * (unsigned)I3 * 4u + oshift), 0);
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NTN; ++t)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[t][q] = 0.f;
    };
    auto pass_weights = [&](int i) __attribute__((always_inline)) {      // byte offset of pass i's parity in the weight image
        return (unsigned)(4 * ((i >> 1) & 1) + 2 * ph + (i & 1)) * par_bytes;
    };

    set_goff(0);
    float fv[kDNF];
    constexpr int kRing = 8;   // <= kDCC: the ring never reaches past the next stage
    float4 aring[kRing];
    unsigned wcur = pass_weights(0);   // scalar byte offset of (parity, stage) in the weight image
#pragma unroll
    for (int f = 0; f < kDNF; ++f) fv[f] = buf_load(dres, goff[f], pshift);
#pragma unroll
    for (int u = 0; u < kRing; ++u) aring[u] = buf_load4(wres, wvoff, wcur + (unsigned)u * 1024u);
#pragma unroll
    for (int f = 0; f < kDNF; ++f) sdst[256 * f] = fv[f];
    __syncthreads();

    constexpr int O00 = BX::PL + BX::BW, O01 = BX::PL, O10 = BX::BW, O11 = 0;  // (td,th) -> box offset
    const int nstage = a.Cout / kDCC;      // even (halo_dgrad_plan)
    // One stage, one basic block.  EDGE: 0 every tile is issued, 1 tile (tn 0, td 1) is depth padding, 2 tile (tn 1, td 0) is.
    auto stage = [&](auto tag, auto edgetag, unsigned dys, unsigned wnext) __attribute__((always_inline)) {
        constexpr int CUR = decltype(tag)::value, NXT = CUR ^ 1, EDGE = decltype(edgetag)::value;
        constexpr int kOff[4] = {O00, O01, O10, O11};
        float bq[NTN][4];
#pragma unroll
        for (int tn = 0; tn < NTN; ++tn)
#pragma unroll
            for (int j = 0; j < 4; ++j)      // j = 2 td + th
                if (!((EDGE == 1 && tn == 0 && j >= 2) || (EDGE == 2 && tn == 1 && j < 2))) bq[tn][j] = bb[CUR * kDBUF + tn * BX::PL + kOff[j]];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < kDCC; ++c) {  // one k-group per channel
            const float4 a_cur = aring[c % kRing];
            aring[c % kRing] = c + kRing < kDCC ? buf_load4(wres, wvoff, wcur + (unsigned)(c + kRing) * 1024u)
                                                : buf_load4(wres, wvoff, wnext + (unsigned)(c + kRing - kDCC) * 1024u);
            float b[NTN][4];
#pragma unroll
            for (int tn = 0; tn < NTN; ++tn)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (!((EDGE == 1 && tn == 0 && j >= 2) || (EDGE == 2 && tn == 1 && j < 2))) b[tn][j] = bq[tn][j];
            if (c + 1 < kDCC) {
#pragma unroll
                for (int tn = 0; tn < NTN; ++tn)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (!((EDGE == 1 && tn == 0 && j >= 2) || (EDGE == 2 && tn == 1 && j < 2)))
                            bq[tn][j] = bb[CUR * kDBUF + (c + 1) * kDB + tn * BX::PL + kOff[j]];
            }
            if (c < kDCC / 2) {  // copy of the next box: two loads per group in the first half of the stage ...
#pragma unroll
                for (int f = 2 * c; f < 2 * c + 2; ++f) fv[f] = buf_load(dres, goff[f], dys + pshift);
            } else {             // ... each value goes to LDS 8 groups after its load
#pragma unroll
                for (int f = 2 * (c - kDCC / 2); f < 2 * (c - kDCC / 2) + 2; ++f) sdst[NXT * kDBUF + 256 * f] = fv[f];
            }
            __builtin_amdgcn_sched_barrier(0);
            const float av[4] = {a_cur.x, a_cur.y, a_cur.z, a_cur.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int tn = 0; tn < NTN; ++tn)
                    if (!((EDGE == 1 && tn == 0 && j >= 2) || (EDGE == 2 && tn == 1 && j < 2)))
                        acc[tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], b[tn][j], acc[tn], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        wcur = wnext;
        __syncthreads();
    };
    auto run_pass = [&](auto edgetag, int i) __attribute__((always_inline)) {
        const bool more = i + 1 < 8;
        // the stage after this pass's last one: the next pass's first (new box origin) or, at the very end, the last stage again
        // (copied into the idle buffer, never read)
        const unsigned wlast = more ? pass_weights(i + 1) : pass_weights(i) + (unsigned)(nstage - 1) * kDCC * 1024u;
        const unsigned dlast = more ? 0u : (unsigned)(nstage - 1) * kDCC * chan_bytes;
        for (int s = 0; s + 1 < nstage; s += 2) {   // stages in pairs: the buffer index is a compile-time constant
            stage(IntTag<0>(), edgetag, (unsigned)(s + 1) * kDCC * chan_bytes, wcur + kDCC * 1024u);
            const bool last = s + 2 == nstage;
            if (last && more) set_goff(i + 1);
            stage(IntTag<1>(), edgetag, last ? dlast : (unsigned)(s + 2) * kDCC * chan_bytes, last ? wlast : wcur + kDCC * 1024u);
        }
    };
    for (int i = 0; i < 8; ++i) {
        const bool edge = hf ? i >= 6 : i < 2;      // wave-uniform
        if (!edge)
            run_pass(IntTag<0>(), i);
        else if (hf == 0)
            run_pass(IntTag<1>(), i);
        else
            run_pass(IntTag<2>(), i);
        write_pass(i);
    }
}

size_t halo_dgrad_workspace_bytes(int Cin, int Cout) { return (size_t)8 * ((Cin + 63) / 64) * 64 * Cout * 8 * sizeof(float); }

bool halo_dgrad_form_decode(int impl, HaloDgradForm* form) {
    form->forced = (impl & 1) != 0;
    form->one_parity = (impl & 2) != 0;
    form->ppw = (impl >> 2) & 15;
    form->rows64_dskip = (impl & 64) != 0;
    form->depth_walk = (impl & 128) != 0;
    return (impl & ~255) == 0;
}

HaloDgradPlan halo_dgrad_plan(int batch, int Cin, int Cout, const ConvGeom& g, size_t workspace_bytes, HaloDgradForm form) {
    HaloDgradPlan p = HaloDgradPlan();
    const bool mode1 = g.OD == 4 && g.OH == 4 && g.OW == 4;
    if (!mode1 && (g.OW % 8 != 0 || g.OH % 8 != 0 || g.OD % 2 != 0)) return p;
    if (Cout % 16 != 0 || Cin < 32 || Cin % 8 != 0) return p;
    if (((long)2 * g.Cy * g.OD * g.OH * g.OW + (long)(g.OH + 1) * g.OW + 1) * 4 >= (1L << 26)) return p;   // offset | class word
    if (workspace_bytes < halo_dgrad_workspace_bytes(Cin, Cout)) return p;
    if ((long)batch * g.Cy * g.OD * g.OH * g.OW >= (1L << 31)) return p;
    if ((long)2 * g.Cy * g.OD * g.OH * g.OW * 4 >= (long)kBufRange || (long)Cout * 1024 >= (long)kBufRange) return p;
    const int ntw = mode1 ? 1 : g.OW / 8, nth = mode1 ? 1 : g.OH / 8, ntd = mode1 ? 1 : g.OD / 2;
    const long tiles = mode1 ? (batch + 1) / 2 : (long)batch * ntd * nth * ntw;
    const int mtiles = (Cin + 63) / 64;
    // (round 4, scripts/small_batch_ab2.py: the gather form of the input gradient is slow at every size — 256 -> 128 channels at
    // 4^3: 110 us at 2 .. 16 samples, 145 at 32, against 75 us for one round of this kernel; 128 -> 64 at 8^3: 59 - 75 us against 43)
    if (!form.forced && tiles * mtiles * 8 < (mode1 ? 16 : 64)) return p;
    if (tiles >= (1L << 31) || mtiles > 65535) return p;
    if ((long)8 * mtiles * 2 * Cout * 1024 >= (long)kBufRange) return p;
    // parities per workgroup: as many as keep >= 512 workgroups (2 per CU); form.one_parity: one parity per workgroup
    int ppw = 8;
    while (ppw > 1 && (tiles * mtiles * (8 / ppw) < 512 || form.one_parity || (Cout / 16) % 2 != 0)) ppw >>= 1;
    if (form.ppw && (Cout / 16) % 2 == 0) ppw = form.ppw;   // tests force 2, 4 or 8 parities
    // 32-row workgroups (four waves, one column tile each): when only 32 rows of the tile exist (Cin <= 32), and when 64-row workgroups
    // would leave CUs without one (small batches: 128 workgroups at 16 samples of a 4^3 grid) — twice as many, half as long
    const bool r32 = !form.rows64_dskip && (Cin <= 32 || tiles * mtiles * (8 / ppw) < 256);
    // Depth-skip form of the 4^3 64-row kernel (conv_dgrad_halo_dskip_kernel, its own weight image: job kind 3).  Forced calls (tests,
    // A/B) get it only where they ask for it, without that conv_dgrad_halo_kernel<1>.  The dispatch takes it for every 64-row 4^3
    // call — measured faster at 64, 128 and 256 samples.  Other grids and the 32-row workgroups have no
    // depth-skip form.
    const bool dskip = mode1 && !r32 && (!form.forced || form.rows64_dskip);
    if (form.rows64_dskip && !dskip) return p;
    // Depth-walk form of the 64-row kernel for dy grids of depth 8 (conv_dgrad_halo_dwalk_kernel: the same weight image, job kind 1).
    // A workgroup is (sample, h/w tile, depth half, output parity ph) and walks its 2 plane pairs x (pd, pw): an even stage count as
    // for several parities per workgroup.  Forced calls get it where they ask for it (impl bit 128, not together with the ppw /
    // one-parity bits), the dispatch where it fills a round of two workgroups per CU (DESIGN.md section 3.1 has the measurements).
    const long walk_tiles = (long)batch * nth * ntw * 2;      // grid x
    const bool walk_shape = !mode1 && g.OD == 8 && Cin > 32 && (Cout / 16) % 2 == 0 && walk_tiles < (1L << 31);
    if (form.depth_walk && (!walk_shape || form.ppw || form.one_parity || form.rows64_dskip)) return p;
    const bool dwalk = walk_shape && (form.forced ? form.depth_walk : walk_tiles * mtiles * 2 >= 512);
    p.served = true;
    p.kernel = dskip ? HaloDgradKernel::dskip4
                     : (mode1 ? (r32 ? HaloDgradKernel::rows32_4 : HaloDgradKernel::rows64_4)
                              : (dwalk ? HaloDgradKernel::rows64_dwalk : (r32 ? HaloDgradKernel::rows32 : HaloDgradKernel::rows64)));
    p.grid = dwalk ? dim3((unsigned)walk_tiles, (unsigned)mtiles, 2)
                   : dim3((unsigned)tiles, r32 ? (unsigned)((Cin + 31) / 32) : (unsigned)mtiles, 8 / ppw);
    p.block = 256;
    // registers admit 3 workgroups per CU; take 3 only when the grid then needs fewer CU-slots in total (a 2048-workgroup
    // grid is 4 full rounds at 2 per CU but 2.67 rounds at 3): otherwise a larger LDS request caps the CU at 2
    p.lds = (size_t)2 * 16 * 256 * sizeof(float);
    {
        const long wgs = dwalk ? walk_tiles * mtiles * 2 : tiles * mtiles * (8 / ppw);
        const long cost2 = ((wgs + 511) / 512) * 2, cost3 = ((wgs + 767) / 768) * 3;
        if (cost2 <= cost3) p.lds = 56 * 1024;
    }
    p.image = ImageJob{dskip ? 3 : 1, mtiles * 2, 0};
    p.workspace_need = halo_dgrad_workspace_bytes(Cin, Cout);
    p.mtiles = mtiles;
    p.ppw = dwalk ? 8 : ppw;      // (the depth walk: 8 passes per workgroup)
    p.ntd = ntd;
    p.nth = nth;
    p.ntw = ntw;
    return p;
}

void halo_dgrad_pack(const HaloDgradPlan& p, const float* w, int Cin, int Cin_total, int Cout, void* workspace, hipStream_t stream) {
    const long total = 8L * p.image.nt * Cout * 64;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pack_dgrad_frag_kernel, dim3(blocks), dim3(256), 0, stream, w, workspace_at<float4>(workspace, p.image.offset), Cout,
                       Cin_total, Cin, p.image.nt, p.image.kind >> 1);
}

static HaloDgradArgs halo_dgrad_args(const HaloDgradPlan& p, const float* dy, const float* bias, float* dx, int batch, int Cin, int Cout,
                                     const ConvGeom& g, int act, float slope, void* workspace) {
    HaloDgradArgs a;
    a.dy = dy;
    a.wp = workspace_at<float4>(workspace, p.image.offset);
    a.bias = bias;
    a.dx = dx;
    a.g = g;
    a.Cin = Cin;
    a.Cout = Cout;
    a.mtiles = p.mtiles;
    a.batch = batch;
    a.ppw = p.ppw;
    a.dntw = FastDiv(p.ntw);
    a.dnth = FastDiv(p.nth);
    a.dntd = FastDiv(p.ntd);
    a.act = act;
    a.slope = slope;
    return a;
}

void halo_dgrad_launch(const HaloDgradPlan& p, const float* dy, const float* bias, float* dx, int batch, int Cin, int Cout,
                       const ConvGeom& g, int act, float slope, void* workspace, hipStream_t stream) {
    const HaloDgradArgs a = halo_dgrad_args(p, dy, bias, dx, batch, Cin, Cout, g, act, slope, workspace);
    switch (p.kernel) {
    case HaloDgradKernel::dskip4:
        hipLaunchKernelGGL(conv_dgrad_halo_dskip_kernel, p.grid, dim3(p.block), p.lds, stream, a);
        break;
    case HaloDgradKernel::rows32_4:
        hipLaunchKernelGGL((conv_dgrad_halo32_kernel<1>), p.grid, dim3(p.block), p.lds, stream, a);
        break;
    case HaloDgradKernel::rows64_4:
        hipLaunchKernelGGL((conv_dgrad_halo_kernel<1>), p.grid, dim3(p.block), p.lds, stream, a);
        break;
    case HaloDgradKernel::rows32:
        hipLaunchKernelGGL((conv_dgrad_halo32_kernel<0>), p.grid, dim3(p.block), p.lds, stream, a);
        break;
    case HaloDgradKernel::rows64:
        hipLaunchKernelGGL((conv_dgrad_halo_kernel<0>), p.grid, dim3(p.block), p.lds, stream, a);
        break;
    case HaloDgradKernel::rows64_dwalk:
        hipLaunchKernelGGL(conv_dgrad_halo_dwalk_kernel, p.grid, dim3(p.block), p.lds, stream, a);
        break;
    }
}


// ================================================================================================================
// wgrad form (nn.Conv3d / nn.ConvTranspose3d weight gradient):
//   dW[co, ci, tap] = sum_{n, o} dy[n, co, o] * x[n, ci, 2o + tap - 1]      GEMM  M = Cout, N = Cin*64, K = positions
// Both operands are activations, so A cannot be packed once per call like a weight — but it can be packed once per
// launch by a streaming pre-pass: dy is rewritten into MFMA A-fragment order (one coalesced float4 per lane per 8
// positions), after which the main kernel has the fwd-halo structure with the roles turned: A fragments stream from
// global, B fragments are read from the x halo box of the TWO input channels this workgroup owns (lane = tap,
// position offset immediate), accumulators live for the whole launch, K (positions) is split over workgroups
// (deterministic workspace + finalize).  One stage = one 1x8x8 position tile = 8 k-groups = 32*TM*TN MFMAs per wave
// against 10 copy loads per thread.
constexpr int kWROWD = 368;                 // 18 rows x 20 floats, padded so that a kd step shifts banks by 16
constexpr int kWHS = kHD * kWROWD;          // floats per channel box
constexpr int kWNF = (2 * kHD * kHH + 7) / 8;  // 18 copy elements per thread per stage (2 channels x 72 rows / 8 half-waves)
// Plane stride of the static-skip form (conv_wgrad_halo_kernel<2, true>, below): its column tiles hold all four kd of both channels, so
// a kd step has to shift banks by 12 and a channel step (4 planes = 1456) by 16 — see the bank table above the kernel.
constexpr int kWROWD_SKIP = 364;

struct HaloWgradArgs {
    const float4* ap;   // packed dy: [mt][slice][8 groups][64 lanes]
    const float* x;
    float* ws;          // [nsplit][Cout][Cin*64] partials (or dw itself when nsplit == 1)
    ConvGeom g;
    int Cin, Cout, nslice, per_split, mt_total;
    long ldw;           // row stride of the output (Cin_total*64 when writing dw directly, Cin*64 for partials)
    FastDiv dntw, dnth, dOD;
};

// ap[((mt*nslice + sl)*8 + gq)*64 + lane] = float4{ dy[n][mt*32 + (lane&31)][od][oh0 + gq][ow0 + 2j + (lane>>5)], j=0..3 }
__global__ void __launch_bounds__(256) pack_wgrad_dy_kernel(const float* __restrict__ dy, float4* __restrict__ ap,
                                                            ConvGeom g, int Cout, int MT, int nslice, FastDiv dntw,
                                                            FastDiv dnth, FastDiv dOD) {
    const long total = (long)MT * nslice * 8 * 64;
    const long O3 = (long)g.OD * g.OH * g.OW;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int lane = (int)(e & 63);
        const int gq = (int)((e >> 6) & 7);
        const long q = e >> 9;
        const uint32_t sl = (uint32_t)(q % nslice);
        const int mt = (int)(q / nslice);
        uint32_t twi, thi, od, n, q1, q2;
        dntw.divmod(sl, q1, twi);
        dnth.divmod(q1, q2, thi);
        dOD.divmod(q2, n, od);
        const int co = mt * 32 + (lane & 31);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (co < Cout) {
            const float* src = dy + ((long)n * Cout + co) * O3 + ((long)od * g.OH + (thi * 8 + gq)) * g.OW + twi * 8 + (lane >> 5);
            v = make_float4(src[0], src[2], src[4], src[6]);
        }
        ap[e] = v;
    }
}

// NCH = input channels per workgroup.  2: the form of rounds 1 - 5 — waves (wm, wn), 128 output rows x (2 channels x 64 taps).
// 4 (round 6, layers with Cout <= 64: the 32 -> 64 stage of the progressive discriminator, where half of the 128 rows were
// padding and the gather GEMM — 0.42 of the matrix peak — was the faster choice): every wave owns ONE of four channels and the
// SAME two row tiles, i.e. 64 output rows x (4 channels x 64 taps): the same 4 x 4 MFMA tiles per k-group and wave, no empty row
// tile.  The four channels' boxes share their per-thread copy offsets (the channel is a scalar offset of the load); Cin % 4 == 0.
//
// SKIP (NCH 2, grids with OH == 8: the 8x8 tile spans the whole H extent, so box row 0 is ih = -1 and box row 17 is ih = 16 in EVERY
// stage of every workgroup): the MFMAs whose B operand is all padding are not issued.  A k-pair of an MFMA is two neighbouring ow at one
// (od, oh = gq), so an MFMA is all padding when its whole 32-column tile has the tap row kh with 2 gq + kh - 1 outside [0, 16).  The
// workgroup's 128 columns are therefore mapped so that a tile is uniform in kh:
//     tile (wn, tn) = tap row kh = 2 wn + tn of BOTH channels,   lane r -> (ci_l = r >> 4, kd = (r >> 2) & 3, kw = r & 3)
// and wave wn = 0 drops tile tn = 0 (kh 0) in k-group gq = 0 (ih = -1), wave wn = 1 drops tile tn = 1 (kh 3) in gq = 7 (ih = 16): 8 of
// the 128 MFMAs of a stage each (1/16), with the four ds_read_b32 that fed them — the same for both column waves, every stage, every
// workgroup and every K split.  The variant is chosen ONCE, by a wave-uniform branch on wn at the top of the kernel into two
// instantiations of the whole body (conv_wgrad_halo_body<2, 0 / 1>: sharing the prologue and epilogue around two copies of the loop
// takes 256 VGPRs + 91 AGPRs and the second wave per SIMD — the allocator then moves the accumulators between register classes
// around the two loops); the stage body itself stays one basic block, and both instantiations execute the same barriers in the same order.  The A
// ring, the copy schedule, the barrier count and the element of `ws` a (co, ci, tap) goes to are those of the generic form.  Code:
// 35.8 KB against 17.7 KB (a wave runs one half of it), 183 VGPRs + 64 AGPRs, two waves per SIMD as the generic form.
//   Exact: a dropped product has B = 0 (the copy's out-of-range loads return 0), fma(a, 0, acc) = acc, and the k order of every
//   accumulator is unchanged, so for finite dy the result is bit-identical to the generic form up to the sign of a zero (acc = -0 would
//   have become +0 by adding a +0 product).  For a non-finite dy the generic form produces 0 * Inf = NaN at the taps that touch the
//   padding; this form does not — it returns what the convolution's definition gives, the sum over the in-range positions.
//   Banks (ds_read_b32: bank = dword address % 32, conflicts inside a 32-lane half only; kpar is constant in a half): a lane reads
//   ci_l * 4 P + kd * P + kh * 20 + (kw & 1) * 10 + (kw >> 1) + uniform, P = the plane stride.  kw gives {0, 10, 1, 11}; with
//   P = kWROWD_SKIP = 364 = 12 mod 32, kd adds {0, 12, 24, 4}: 16 distinct banks {0-5, 10-15, 22-25}, and the channel step 1456 = 16
//   mod 32 maps them onto the other 16 — conflict-free.  (P = kWROWD = 368 = 16 would put kd 0 / 2 and 1 / 3 on the same banks, 4-way
//   with the channel step 1472 = 0.)  The copy's ds_write_b32 pattern is independent of P inside the box: a half-wave stores one row,
//   18 lanes on (w & 1) * 10 + (w >> 1) = 18 distinct banks; its 14 out-of-box lanes store to 7 other rows' pad slots (9 and 19 of a
//   row), which land on busy banks 2- or 3-way for either P (of the 36 store instructions of a stage, worst half: 24 x 2-way and
//   12 x 3-way at P = 368, 20 and 16 at P = 364) — 18 stores per thread against 128 MFMAs of 64 cycles.
// V: the static-skip variant of the calling wave — -1 none (the generic form), 0 / 1: column wave wn = V of the SKIP form.
template <int NCH, int V>
__device__ __forceinline__ void conv_wgrad_halo_body(const HaloWgradArgs& a) {
    constexpr bool SKIP = V >= 0;
    static_assert(!SKIP || NCH == 2, "the static-skip column map is the 2-channel form's");
    constexpr int WROWD = SKIP ? kWROWD_SKIP : kWROWD;  // per-variant plane and channel strides of the box
    constexpr int WHS = kHD * WROWD;
    extern __shared__ __attribute__((aligned(16))) float wbox[];  // [2 buffers][NCH channels][kHD][WROWD]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = NCH == 2 ? wave >> 1 : 0, wn = SKIP ? V : (NCH == 2 ? wave & 1 : wave), r = lane & 31, kpar = lane >> 5;
    const int ci0 = blockIdx.x * NCH;                  // the input channels (64 output columns each) of this workgroup
    const int mt0 = blockIdx.y * (NCH == 2 ? 4 : 2);   // 128 (64) output rows = 4 (2) row tiles of 32
    constexpr int NF = NCH == 2 ? kWNF : 2 * kWNF;     // copy elements per thread per stage
    constexpr int NV = NCH == 2 ? kWNF : kWNF / 2;     // distinct per-thread copy offsets (NCH 4: shared by the channels)
    const int split = blockIdx.z;
    const int s_beg = split * a.per_split, s_end = min(a.nslice, s_beg + a.per_split);

    // lane -> (channel, tap) of its column inside each of the wave's two 32-column tiles: col = wn*64 + tn*32 + r is
    // (ci_l = wn, tap = tn*32 + r); SKIP: tile = tap row kh = 2 wn + tn, lane r = (ci_l, kd, kw)
    auto col_ci = [&](int tn) { return SKIP ? r >> 4 : (wn * 64 + tn * 32 + r) >> 6; };
    auto col_tap = [&](int tn) { return SKIP ? ((r >> 2) & 3) * 16 + (2 * wn + tn) * 4 + (r & 3) : (tn * 32 + r) & 63; };
    int lanebase[2];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        const int tap = col_tap(tn), kd = tap >> 4, kh = (tap >> 2) & 3, kw = tap & 3;
        lanebase[tn] = col_ci(tn) * WHS + kd * WROWD + kh * kROWH + (kw & 1) * kHWH + (kw >> 1) + kpar;
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

    // ---- copy bookkeeping: element f is (channel c = f / 9, row 8*(f%9) + tid/32, column tid%32) of the 2-channel box.
    // The box moves with the slice, so the global address has a per-thread part that never changes (voff: position inside
    // the box and channel) and a per-stage part that is the same for every thread (scalar: sample, channel pair, box
    // origin — folded into the buffer resource's base).  Whether an element is padding depends on the slice only
    // through six edge flags (first / last tile in D, H, W): the element's class bits sit in bits 26..31 of `cls`, the
    // stage's flags in the same bits of a scalar, and (cls & flags) | voff is >= num_records (2^26) exactly for padding —
    // one v_and_or_b32 per element per stage is all the vector work the copy needs; the hardware returns 0 for those.
    // Threads outside the box store to an unread pad slot (column 9 of a half row).
    // SKIP: the H flags (bits 28, 29) are set in every stage, so the class bits ride in the offset word itself — voff | cls, an
    // always-outside element is the bare bit 28 — and the stage's offsets are voff & (flags | 0x03ffffff): the same values with half
    // the registers, which is what keeps this form at two waves per SIMD. ----
    const int I3 = a.g.ID * a.g.IH * a.g.IW;
    const int fl_w = tid & 31, frow = tid >> 5;
    const int lds_w = (fl_w & 1) * kHWH + (fl_w >> 1);
    const int prow = (tid >> 1) % (kHD * kHH);
    const int pad = (prow / kHH) * WROWD + (prow % kHH) * kROWH + (tid & 1) * kHWH + (kHWH - 1);
    lds_float* const wl = (lds_float*)wbox;
    lds_float* sdst[kWNF / 2];   // LDS destination of the row inside (buffer 0, channel 0); identical for both channels
    unsigned voff[NV], cls[NV];
#pragma unroll
    for (int f = 0; f < kWNF / 2; ++f) {
        const int row = 8 * f + frow;
        const int hd = row / kHH, hh = row - hd * kHH;
        const bool inbox = fl_w < kHWF && row < kHD * kHH;
        sdst[f] = wl + (inbox ? hd * WROWD + hh * kROWH + lds_w : pad);
        pin_vgpr(sdst[f]);
#pragma unroll
        for (int c = 0; c < (NCH == 2 ? 2 : 1); ++c) {
            const bool ok = inbox && (ci0 + c) < a.Cin;
            voff[c * (kWNF / 2) + f] = ok ? (unsigned)(c * I3 + (hd * a.g.IH + hh) * a.g.IW + fl_w) * 4u : kBufOutside;
            cls[c * (kWNF / 2) + f] = (hd == 0 ? 1u << 26 : 0u) | (hd == kHD - 1 ? 1u << 27 : 0u) | (hh == 0 ? 1u << 28 : 0u) |
                                      (hh == kHH - 1 ? 1u << 29 : 0u) | (fl_w == 0 ? 1u << 30 : 0u) |
                                      (fl_w == kHWF - 1 ? 1u << 31 : 0u);
            if constexpr (SKIP) {
                voff[c * (kWNF / 2) + f] = ok ? voff[c * (kWNF / 2) + f] | cls[c * (kWNF / 2) + f] : 1u << 28;
            } else {
                pin_vgpr(cls[c * (kWNF / 2) + f]);
            }
            pin_vgpr(voff[c * (kWNF / 2) + f]);
        }
    }
    float fv[NF];
    unsigned eoff[NV];   // per stage: (cls & flags) | voff
    __amdgpu_buffer_rsrc_t xres;
    auto xres_of = [&]() __attribute__((always_inline)) { return xres; };
    // element f of a stage's copy: channel f / (kWNF / 2), row pattern f % (kWNF / 2); NCH 4: the channel rides in the scalar offset
    const unsigned chan_bytes = (unsigned)I3 * 4u;
    auto copy_load = [&](int f) __attribute__((always_inline)) {
        if constexpr (NCH == 2) {
            return buf_load(xres_of(), eoff[f], 0);
        } else {
            return buf_load(xres_of(), eoff[f % (kWNF / 2)], (unsigned)(f / (kWNF / 2)) * chan_bytes);
        }
    };
    const int ntw_ = (int)a.g.OW / 8, nth_ = (int)a.g.OH / 8;
    auto copy_prepare = [&](int sl) {  // slice sl -> resource base at the box origin + the padding offsets (scalar work + 18 VALU)
        uint32_t twi, thi, od, n, q1, q2;
        a.dntw.divmod((uint32_t)sl, q1, twi);
        a.dnth.divmod(q1, q2, thi);
        a.dOD.divmod(q2, n, od);
        const long origin = ((long)n * a.g.Cx + ci0) * I3 + ((2 * (long)od - 1) * a.g.IH + (16 * (long)thi - 1)) * a.g.IW +
                            (16 * (long)twi - 1);   // may point before the tensor: those elements are padding
        xres = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x + origin), 0, 1 << 26, 0x00020000);
        const unsigned flags = (od == 0 ? 1u << 26 : 0u) | ((int)od == a.g.OD - 1 ? 1u << 27 : 0u) | (thi == 0 ? 1u << 28 : 0u) |
                               ((int)thi == nth_ - 1 ? 1u << 29 : 0u) | (twi == 0 ? 1u << 30 : 0u) |
                               ((int)twi == ntw_ - 1 ? 1u << 31 : 0u);
#pragma unroll
        for (int f = 0; f < NV; ++f) eoff[f] = SKIP ? voff[f] & (flags | 0x03ffffffu) : (cls[f] & flags) | voff[f];
    };

    const int nst = s_end - s_beg;
    constexpr int kRing = 8;  // A fragments: ring of 8 k-groups (one stage); group index runs over (slice, gq)
    const int G = nst * 8;
    if (nst > 0) {
        __amdgpu_buffer_rsrc_t ares[2];   // packed dy of this wave's two 32-row tiles
#pragma unroll
        for (int t = 0; t < 2; ++t) ares[t] = make_rsrc(a.ap + ((long)(mt0 + wm * 2 + t) * a.nslice + s_beg) * 8 * 64);
        const unsigned avoff = lane * 16;
        // B-fragment read addresses: (buffer, column tile, k-groups 0-3 / 4-7); the rest are immediates.  SKIP: the wave's two
        // tiles are one tap row (kROWH) apart, so one address serves and all of (buffer, tile, k-group) is immediate.
        const lds_float* bb[2][2][2];
        if constexpr (SKIP) {
            const lds_float* b0 = wl + lanebase[0];
            pin_vgpr(b0);
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                    for (int h = 0; h < 2; ++h) bb[b][tn][h] = b0 + b * (NCH * WHS) + tn * kROWH + h * (8 * kROWH);
        } else {
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        bb[b][tn][h] = wl + b * (NCH * WHS) + lanebase[tn] + h * (8 * kROWH);
                        pin_vgpr(bb[b][tn][h]);
                    }
        }

        copy_prepare(s_beg);
#pragma unroll
        for (int f = 0; f < NF; ++f) fv[f] = copy_load(f);
        float4 aring[kRing][2];
#pragma unroll
        for (int u = 0; u < kRing; ++u)
#pragma unroll
            for (int t = 0; t < 2; ++t) aring[u][t] = buf_load4(ares[t], avoff, (unsigned)(u < G ? u : G - 1) * 1024u);
#pragma unroll
        for (int f = 0; f < NF; ++f) sdst[f % (kWNF / 2)][(f / (kWNF / 2)) * WHS] = fv[f];
        __syncthreads();

        // V 0: tile 0 (kh 0) is padding in k-group 0, V 1: tile 1 (kh 3) in k-group 7.  dead(tn, gq) folds after unrolling: a dead
        // tile's LDS reads and MFMAs are simply not emitted.
        auto stage = [&](auto tag, int st) {
            constexpr int CUR = decltype(tag)::value, NXT = CUR ^ 1;
            auto dead = [](int tn, int gq) { return (V == 0 && tn == 0 && gq == 0) || (V == 1 && tn == 1 && gq == 7); };
            const int snext = st + 1 < nst ? st + 1 : st;   // last stage: re-copy into the idle buffer
            float bq[2][4] = {};
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) {
                if (dead(tn, 0)) continue;
                const lds_float* hb = bb[CUR][tn][0];
                bq[tn][0] = hb[0];
                bq[tn][1] = hb[2];
                bq[tn][2] = hb[4];
                bq[tn][3] = hb[6];
            }
            copy_prepare(s_beg + snext);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int gq = 0; gq < 8; ++gq) {   // k-group gq = output row ph of the 8x8 tile; j = column pair
                float4 a_cur[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) a_cur[t] = aring[gq][t];
                int gi = (st + 1) * 8 + gq;
                gi = gi < G ? gi : G - 1;
#pragma unroll
                for (int t = 0; t < 2; ++t) aring[gq][t] = buf_load4(ares[t], avoff, (unsigned)gi * 1024u);
                float b[2][4];
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                    for (int j = 0; j < 4; ++j) b[tn][j] = bq[tn][j];
                if (gq + 1 < 8) {
#pragma unroll
                    for (int tn = 0; tn < 2; ++tn) {
                        if (dead(tn, gq + 1)) continue;
                        const lds_float* hb = bb[CUR][tn][(gq + 1) >> 2] + 2 * ((gq + 1) & 3) * kROWH;
                        bq[tn][0] = hb[0];
                        bq[tn][1] = hb[2];
                        bq[tn][2] = hb[4];
                        bq[tn][3] = hb[6];
                    }
                }
                // copy of the next box: loads spread over groups 0..3, LDS stores 4 groups later
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    if (f * 4 / NF == gq) fv[f] = copy_load(f);
                    if (f * 4 / NF + 4 == gq) sdst[f % (kWNF / 2)][NXT * (NCH * WHS) + (f / (kWNF / 2)) * WHS] = fv[f];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float a0 = j == 0 ? a_cur[0].x : (j == 1 ? a_cur[0].y : (j == 2 ? a_cur[0].z : a_cur[0].w));
                    const float a1 = j == 0 ? a_cur[1].x : (j == 1 ? a_cur[1].y : (j == 2 ? a_cur[1].z : a_cur[1].w));
                    if (!dead(0, gq)) {
                        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b[0][j], acc[0][0], 0, 0, 0);
                        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b[0][j], acc[1][0], 0, 0, 0);
                    }
                    if (!dead(1, gq)) {
                        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b[1][j], acc[0][1], 0, 0, 0);
                        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b[1][j], acc[1][1], 0, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
        };
        for (int st = 0; st + 1 < nst; st += 2) {
            stage(IntTag<0>(), st);
            stage(IntTag<1>(), st + 1);
        }
        if (nst & 1) stage(IntTag<0>(), nst - 1);
    }

    // epilogue: out[split][co][ci*64 + tap]
    float* out = a.ws + (long)split * a.Cout * a.ldw;
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        const int ci = ci0 + col_ci(tn);
        if (ci >= a.Cin) continue;
        const long cbase = (long)ci * 64 + col_tap(tn);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int co = (mt0 + wm * 2 + t) * 32 + (q & 3) + 8 * (q >> 2) + 4 * kpar;
                if (co < a.Cout) out[(long)co * a.ldw + cbase] = acc[t][tn][q];
            }
        }
    }
}

template <int NCH, bool SKIP = false>
__global__ void __launch_bounds__(256) conv_wgrad_halo_kernel(HaloWgradArgs a) {
    if constexpr (!SKIP) {
        conv_wgrad_halo_body<NCH, -1>(a);
    } else {   // wave-uniform: each column wave runs its own instantiation; the barriers of the two pair up one to one
        if ((__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) & 1) == 0) conv_wgrad_halo_body<NCH, 0>(a);
        else conv_wgrad_halo_body<NCH, 1>(a);
    }
}

// ---- wgrad form on 4^3 output grids (8^3 inputs) -----------------------------------------------------------------
// Same structure as conv_wgrad_halo_kernel with the geometry of conv_fwd_halo4_kernel: a slice is a whole sample (its 64
// output positions = 8 k-groups), the box is the zero-padded 10^3 sample of the workgroup's two input channels (padding
// written once, a stage copies 2 x 512 contiguous floats), positions of a group: od = gq >> 1, oh = 2 (gq & 1) + (j >> 1),
// ow = 2 (j & 1) + kpar.
//
// Static padding skip: od = gq >> 1 of every MFMA is a compile-time constant, so with column tiles that are uniform in kd,
//     tile (wn, tn) = tap plane kd = 2 wn + tn of BOTH channels,   lane r -> (ci_l = r >> 4, kh = (r >> 2) & 3, kw = r & 3),
// tile kd = 0 reads the zero plane id = -1 in k-groups 0, 1 (od 0) and tile kd = 3 reads id = 8 in k-groups 6, 7 (od 3).  Wave wn = 0
// drops tile tn = 0 in groups 0, 1, wave wn = 1 drops tile tn = 1 in groups 6, 7: 16 of the 128 MFMAs of a stage each (1/8), with their
// eight ds_read_b32 — the same in both column waves, every stage, workgroup and K split.  As in conv_wgrad_halo_kernel<2, true> the
// variant is chosen once by a wave-uniform branch into two instantiations of the body (conv_wgrad_halo4_body<0 / 1>; 26.0 KB of code
// against 13.1 KB, 164 VGPRs + 64 AGPRs), and the same exactness statement holds: the dropped products
// have B = 0 (the box's zero planes 0 and 9, which are now never read), the k order of every accumulator is unchanged, so the result
// is bit-identical for finite dy up to the sign of a zero; a non-finite dy no longer yields the 0 * Inf = NaN of the padded product.
//   The box has its own strides (conv_fwd_halo4_kernel keeps k4*): half 6, row 12, plane 120, channel 1200.  Banks (dword address
//   % 32 inside a 32-lane half): a lane reads ci_l * 1200 + kh * 12 + (kw & 1) * 6 + (kw >> 1) + uniform.  kw gives {0, 6, 1, 7}, kh adds
//   {0, 12, 24, 4}: 16 distinct banks {0, 1, 4-7, 10-13, 18, 19, 24, 25, 30, 31}, and the channel step 1200 = 16 mod 32 maps them onto
//   the other 16 — conflict-free (half 5 / row 10 has no channel step that does; the former tap-major tiles were 2-way on it).  The
//   copy's ds_write_b32 (a half-wave = 4 rows of 8 consecutive iw) is 2-way with these strides as it was with k4*.  LDS 19 200 B
//   (was 16 640): not what limits the workgroups per CU.
constexpr int kW4HALF = 6, kW4ROW = 12, kW4PLANE = 120, kW4CH = 10 * kW4PLANE;
// ap[((mt*nslice + sl)*8 + gq)*64 + lane] = float4{ dy[sl][mt*32 + (lane&31)][pos(gq, j, lane>>5)], j = 0..3 }
__global__ void __launch_bounds__(256) pack_wgrad_dy4_kernel(const float* __restrict__ dy, float4* __restrict__ ap, int Cout,
                                                             int MT, int nslice) {
    const long total = (long)MT * nslice * 8 * 64;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const int lane = (int)(e & 63);
        const int gq = (int)((e >> 6) & 7);
        const long q = e >> 9;
        const long sl = q % nslice;
        const int mt = (int)(q / nslice);
        const int co = mt * 32 + (lane & 31);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (co < Cout) {
            // j -> position offset (j >> 1) * 4 + 2 (j & 1): j = 0,1,2,3 -> +0, +2, +4, +6
            const float* src = dy + (sl * Cout + co) * 64 + (gq >> 1) * 16 + (gq & 1) * 8 + (lane >> 5);
            v = make_float4(src[0], src[2], src[4], src[6]);
        }
        ap[e] = v;
    }
}

template <int V>   // V = the column wave wn of the caller
__device__ __forceinline__ void conv_wgrad_halo4_body(const HaloWgradArgs& a) {
    constexpr int kBUF = 2 * kW4CH;  // two channels per buffer
    extern __shared__ __attribute__((aligned(16))) float wbox[];  // [2 buffers][2 channels][kW4CH]
    lds_float* const wl = (lds_float*)wbox;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = V, r = lane & 31, kpar = lane >> 5;
    const int ci0 = blockIdx.x * 2, mt0 = blockIdx.y * 4, split = blockIdx.z;
    const int s_beg = split * a.per_split, s_end = min(a.nslice, s_beg + a.per_split);
    const int nst = s_end - s_beg;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

    for (int e = tid; e < 2 * kBUF; e += 256) wl[e] = 0.f;   // the padding, once

    if (nst > 0) {
        // tile (wn, tn) = tap plane kd = 2 wn + tn of both channels, lane r = (ci_l, kh, kw); one address per (buffer, tn, od)
        const lds_float* bb[2][2][4];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int kd = 2 * wn + tn, kh = (r >> 2) & 3, kw = r & 3;
            const int lb = (r >> 4) * kW4CH + kd * kW4PLANE + kh * kW4ROW + (kw & 1) * kW4HALF + (kw >> 1) + kpar;
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int od = 0; od < 4; ++od) {
                    bb[b][tn][od] = wl + b * kBUF + lb + od * (2 * kW4PLANE);
                    pin_vgpr(bb[b][tn][od]);
                }
        }
        // copy: the two channels are 1024 contiguous floats of the sample; thread t moves elements t + 256 f
        unsigned voff[4];
        lds_float* sdst[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const int e = tid + 256 * f, c = e >> 9, idx = e & 511;
            const int id = idx >> 6, ih = (idx >> 3) & 7, iw = idx & 7;
            voff[f] = (ci0 + c) < a.Cin ? (unsigned)e * 4u : kBufOutside;
            sdst[f] = wl + c * kW4CH + (id + 1) * kW4PLANE + (ih + 1) * kW4ROW + ((iw + 1) & 1) * kW4HALF + ((iw + 1) >> 1);
            pin_vgpr(voff[f]);
            pin_vgpr(sdst[f]);
        }
        __amdgpu_buffer_rsrc_t ares[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) ares[t] = make_rsrc(a.ap + ((long)(mt0 + wm * 2 + t) * a.nslice + s_beg) * 8 * 64);
        const unsigned avoff = lane * 16;
        const long slice_floats = (long)a.g.Cx * 512;
        const float* xb = a.x + (long)s_beg * slice_floats + (long)ci0 * 512;
        const int G = nst * 8;
        constexpr int kRing = 8;
        float fv[4];
        __syncthreads();   // zero fill complete
        {
            const __amdgpu_buffer_rsrc_t xres = make_rsrc(xb);
#pragma unroll
            for (int f = 0; f < 4; ++f) fv[f] = buf_load(xres, voff[f], 0);
        }
        float4 aring[kRing][2];
#pragma unroll
        for (int u = 0; u < kRing; ++u)
#pragma unroll
            for (int t = 0; t < 2; ++t) aring[u][t] = buf_load4(ares[t], avoff, (unsigned)(u < G ? u : G - 1) * 1024u);
#pragma unroll
        for (int f = 0; f < 4; ++f) *sdst[f] = fv[f];
        __syncthreads();

        // V 0: tile 0 (kd 0) is padding in k-groups 0, 1 (od 0), V 1: tile 1 (kd 3) in k-groups 6, 7 (od 3).  dead(tn, gq) folds
        // after unrolling: a dead tile's LDS reads and MFMAs are simply not emitted.
        auto stage = [&](auto tag, int st) {
            constexpr int CUR = decltype(tag)::value, NXT = CUR ^ 1;
            auto dead = [](int tn, int gq) { return (V == 0 && tn == 0 && gq < 2) || (V == 1 && tn == 1 && gq >= 6); };
            const int snext = st + 1 < nst ? st + 1 : st;   // last stage: re-copy into the idle buffer
            const __amdgpu_buffer_rsrc_t xres = make_rsrc(xb + (long)snext * slice_floats);
            float bq[2][4] = {};
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) {
                if (dead(tn, 0)) continue;
                const lds_float* hb = bb[CUR][tn][0];
                bq[tn][0] = hb[0];
                bq[tn][1] = hb[2];
                bq[tn][2] = hb[2 * kW4ROW];
                bq[tn][3] = hb[2 * kW4ROW + 2];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int gq = 0; gq < 8; ++gq) {
                float4 a_cur[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) a_cur[t] = aring[gq][t];
                int gi = (st + 1) * 8 + gq;
                gi = gi < G ? gi : G - 1;
#pragma unroll
                for (int t = 0; t < 2; ++t) aring[gq][t] = buf_load4(ares[t], avoff, (unsigned)gi * 1024u);
                float b[2][4];
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                    for (int j = 0; j < 4; ++j) b[tn][j] = bq[tn][j];
                if (gq + 1 < 8) {
#pragma unroll
                    for (int tn = 0; tn < 2; ++tn) {
                        if (dead(tn, gq + 1)) continue;
                        const lds_float* hb = bb[CUR][tn][(gq + 1) >> 1] + ((gq + 1) & 1) * (4 * kW4ROW);
                        bq[tn][0] = hb[0];
                        bq[tn][1] = hb[2];
                        bq[tn][2] = hb[2 * kW4ROW];
                        bq[tn][3] = hb[2 * kW4ROW + 2];
                    }
                }
                if (gq < 4) fv[gq] = buf_load(xres, voff[gq], 0);                 // copy of the next sample: loads ...
                else sdst[gq - 4][NXT * kBUF] = fv[gq - 4];                       // ... and stores 4 groups later
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float a0 = j == 0 ? a_cur[0].x : (j == 1 ? a_cur[0].y : (j == 2 ? a_cur[0].z : a_cur[0].w));
                    const float a1 = j == 0 ? a_cur[1].x : (j == 1 ? a_cur[1].y : (j == 2 ? a_cur[1].z : a_cur[1].w));
                    if (!dead(0, gq)) {
                        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b[0][j], acc[0][0], 0, 0, 0);
                        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b[0][j], acc[1][0], 0, 0, 0);
                    }
                    if (!dead(1, gq)) {
                        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b[1][j], acc[0][1], 0, 0, 0);
                        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b[1][j], acc[1][1], 0, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            __syncthreads();
        };
        for (int st = 0; st + 1 < nst; st += 2) {
            stage(IntTag<0>(), st);
            stage(IntTag<1>(), st + 1);
        }
        if (nst & 1) stage(IntTag<0>(), nst - 1);
    }

    // epilogue: out[split][co][ci*64 + tap]
    float* out = a.ws + (long)split * a.Cout * a.ldw;
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        const int ci = ci0 + (r >> 4);
        if (ci >= a.Cin) continue;
        const long cbase = (long)ci * 64 + (2 * wn + tn) * 16 + (r & 15);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int co = (mt0 + wm * 2 + t) * 32 + (q & 3) + 8 * (q >> 2) + 4 * kpar;
                if (co < a.Cout) out[(long)co * a.ldw + cbase] = acc[t][tn][q];
            }
        }
    }
}

__global__ void __launch_bounds__(256) conv_wgrad_halo4_kernel(HaloWgradArgs a) {
    // wave-uniform: each column wave runs its own instantiation; the barriers of the two pair up one to one
    if ((__builtin_amdgcn_readfirstlane(threadIdx.x >> 6) & 1) == 0) conv_wgrad_halo4_body<0>(a);
    else conv_wgrad_halo4_body<1>(a);
}

// sums the split partials [nsplit][Cout][Cin*64] into dw[Cout][Cin_total*64]
__global__ void __launch_bounds__(256) wgrad_halo_finalize_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                                  int Cout, int ncol, long ldw, int nsplit) {
    // 16-byte pieces (ncol = Cin * 64 and ldw are multiples of 4; the partial images and dw rows are 16-byte aligned), up to four
    // partials requested before the first add; partials are summed in ascending split order for every element
    const long total = (long)Cout * ncol, total4 = total >> 2;
    for (long e4 = (long)blockIdx.x * 256 + threadIdx.x; e4 < total4; e4 += (long)gridDim.x * 256) {
        const f32x4* p = reinterpret_cast<const f32x4*>(ws) + e4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        int s = 0;
        for (; s + 3 < nsplit; s += 4) {
            const f32x4 a0 = p[(long)s * total4], a1 = p[(long)(s + 1) * total4], a2 = p[(long)(s + 2) * total4],
                        a3 = p[(long)(s + 3) * total4];
            v += a0;
            v += a1;
            v += a2;
            v += a3;
        }
        for (; s < nsplit; ++s) v += p[(long)s * total4];
        const long e = e4 << 2;
        const long co = e / ncol, c = e - co * ncol;
        *reinterpret_cast<f32x4*>(dw + co * ldw + c) = v;
    }
}

static bool wgrad_mode4(const ConvGeom& g) { return g.OD == 4 && g.OH == 4 && g.OW == 4; }

// rows64: the 64-row form (conv_wgrad_halo_kernel<4>: four input channels per workgroup) — layers with at most 64 output channels
// on 8-divisible grids; mtiles then counts 64-row tiles (mt_total = 2 mtiles row tiles of 32), else 128-row tiles (4 mtiles).
static bool wgrad_rows64(const ConvGeom& g, int Cin, int Cout) {
    return !wgrad_mode4(g) && Cout <= 64 && Cin >= 4 && Cin % 4 == 0;
}
static void wgrad_halo_plan(int batch, const ConvGeom& g, int Cin, int Cout, int& nslice, int& nsplit, int& mtiles) {
    nslice = wgrad_mode4(g) ? batch : batch * g.OD * (g.OH / 8) * (g.OW / 8);   // 4^3 outputs: a slice is a sample
    const bool rows64 = wgrad_rows64(g, Cin, Cout);
    mtiles = rows64 ? (Cout + 63) / 64 : (Cout + 127) / 128;
    const int ntiles = (rows64 ? Cin / 4 : (Cin + 1) / 2) * mtiles;
    nsplit = (512 + ntiles - 1) / ntiles;
    if (nsplit > nslice / 4) nsplit = nslice / 4 > 0 ? nslice / 4 : 1;   // >= 4 stages per workgroup
    if (nsplit < 1) nsplit = 1;
}

// ---- the packed dy image written by the kernel that PRODUCES dy ---------------------------------------------------------------------
// pack_wgrad_dy(4)_kernel re-reads the incoming gradient of a layer right after the activation backward wrote it (67 MB each way at
// the critic's second layer: 18 us, 0.15 ms per WGAN step with the 4^3 form).  When the halo weight-gradient kernel will serve the
// call and the grid is 8^3 or 4^3 with Cout a multiple of 128 (no padded row tiles), the producer writes the image itself:
// sg_act_bwd_rowsum_pack8 (activation backward + bias row sums + image, 8^3) and sg_head_dot_bwd (4^3), then
// sg_conv3d_k4s2p1_wgrad_prepacked skips the packing launch.  HaloWgradPlan::producer_image answers whether; dy_image.nt and nslice
// say with which MT / nslice.
HaloWgradPlan halo_wgrad_plan(int batch, int Cin, int Cout, const ConvGeom& g, size_t workspace_bytes, bool forced) {
    HaloWgradPlan p = HaloWgradPlan();
    const bool mode4 = wgrad_mode4(g);
    if ((!mode4 && (g.OW % 8 != 0 || g.OH % 8 != 0)) || Cin < 2 || Cout < 32) return p;
    int nslice, nsplit, mtiles;
    wgrad_halo_plan(batch, g, Cin, Cout, nslice, nsplit, mtiles);
    const size_t pack_bytes = (size_t)mtiles * 4 * nslice * 8 * 64 * sizeof(float4);      // (rows64: 2 mtiles row tiles are used)
    p.workspace_need = pack_bytes + (size_t)nsplit * Cout * Cin * 64 * sizeof(float) + 256;
    if ((long)batch * g.Cx * g.ID * g.IH * g.IW >= (1L << 31)) return p;
    if ((long)2 * g.ID * g.IH * g.IW * 4 >= (1L << 26)) return p;   // box offset | edge-class word needs offsets below 2^26
    const bool rows64 = wgrad_rows64(g, Cin, Cout);
    if (rows64 && (long)4 * g.ID * g.IH * g.IW * 4 >= (1L << 26)) return p;
    const int ntiles = (rows64 ? Cin / 4 : (Cin + 1) / 2) * mtiles;
    // auto-dispatch where it wins (round-1 A/B): no half-empty row tiles (Cout <= 64: the 64-row form, round 6) and enough workgroups
    if (!forced && ((Cout <= 64 && !rows64) || (long)ntiles * nsplit < 384)) return p;
    if (workspace_bytes < p.workspace_need) return p;
    p.served = true;
    p.nslice = nslice;
    p.per_split = (nslice + nsplit - 1) / nsplit;
    p.nsplit = (nslice + p.per_split - 1) / p.per_split;
    p.mtiles = mtiles;
    p.dy_image = ImageJob{mode4 ? 1 : 0, rows64 ? mtiles * 2 : mtiles * 4, 0};
    p.producer_image = !forced && (mode4 || (g.OD == 8 && g.OH == 8 && g.OW == 8)) && Cout % 128 == 0;
    p.partial_offset = pack_bytes;
    p.block = 256;
    if (mode4) {
        p.kernel = HaloWgradKernel::halo4;
        p.grid = dim3((Cin + 1) / 2, mtiles, p.nsplit);
        p.lds = (size_t)2 * 2 * kW4CH * sizeof(float);
    } else if (rows64) {
        p.kernel = HaloWgradKernel::rows64;
        p.grid = dim3(Cin / 4, mtiles, p.nsplit);
        p.lds = (size_t)2 * 4 * kWHS * sizeof(float);
    } else {
        // OH == 8: the 8x8 tile spans H, which rows of the box are padding is static -> the form that skips them
        p.kernel = g.OH == 8 ? HaloWgradKernel::rows128_skip_h : HaloWgradKernel::rows128;
        p.grid = dim3((Cin + 1) / 2, mtiles, p.nsplit);
        p.lds = g.OH == 8 ? (size_t)2 * 2 * kHD * kWROWD_SKIP * sizeof(float) : (size_t)2 * 2 * kWHS * sizeof(float);
    }
    return p;
}


// dz = dy * act'(y), row sums of dz, and dz in the halo weight-gradient kernel's A-fragment order, for [N][C][8][8][8] tensors: one
// WAVE per (sample, channel) row of 512 voxels, lane = one (od, oh) line of 8: two b128 loads per operand, two b128 stores of dz,
// and the line's even / odd columns as the two float4 of pack_wgrad_dy_kernel's layout (nth = ntw = 1: slice = n * 8 + od, group = oh).
__global__ void __launch_bounds__(256) act_bwd_pack8_kernel(const float* __restrict__ y, const float* __restrict__ dy,
                                                            float* __restrict__ dz, float* __restrict__ rowsum,
                                                            float4* __restrict__ ap, long rows, int C, long nslice, int act, float slope) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const long base = row * 512 + lane * 8;
    const f32x4 y0 = *reinterpret_cast<const f32x4*>(y + base), y1 = *reinterpret_cast<const f32x4*>(y + base + 4);
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(dy + base), g1 = *reinterpret_cast<const f32x4*>(dy + base + 4);
    f32x4 z0, z1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        z0[j] = act == SG_ACT_LEAKY ? (y0[j] > 0.f ? g0[j] : g0[j] * slope) : (y0[j] > 0.f ? g0[j] : 0.f);
        z1[j] = act == SG_ACT_LEAKY ? (y1[j] > 0.f ? g1[j] : g1[j] * slope) : (y1[j] > 0.f ? g1[j] : 0.f);
    }
    *reinterpret_cast<f32x4*>(dz + base) = z0;
    *reinterpret_cast<f32x4*>(dz + base + 4) = z1;
    const float s = sg_wave_sum(((z0[0] + z0[1]) + (z0[2] + z0[3])) + ((z1[0] + z1[1]) + (z1[2] + z1[3])));
    if (lane == 0) rowsum[row] = s;
    const long n = row / C;
    const int co = (int)(row - n * C), mt = co >> 5, r = co & 31, od = lane >> 3, oh = lane & 7;
    const long e = (((long)mt * nslice + n * 8 + od) * 8 + oh) * 64 + r;
    ap[e] = make_float4(z0[0], z0[2], z1[0], z1[2]);          // columns 0, 2, 4, 6 (lane half 0 of the fragment)
    ap[e + 32] = make_float4(z0[1], z0[3], z1[1], z1[3]);     // columns 1, 3, 5, 7
}
int halo_act_bwd_pack8_launch(const float* y, const float* dy, float* dz, float* rowsum, void* ap, long rows, int C, long nslice,
                              int act, float slope, hipStream_t stream) {
    hipLaunchKernelGGL(act_bwd_pack8_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, y, dy, dz, rowsum, (float4*)ap,
                       rows, C, nslice, act, slope);
    return 1;
}

void halo_wgrad_pack(const HaloWgradPlan& p, const float* dy, int Cout, const ConvGeom& g, void* workspace, hipStream_t stream) {
    float4* ap = workspace_at<float4>(workspace, p.dy_image.offset);
    int blocks = (int)((p.partial_offset / sizeof(float4) + 255) / 256);
    if (blocks > 8192) blocks = 8192;
    if (p.dy_image.kind == 1)
        hipLaunchKernelGGL(pack_wgrad_dy4_kernel, dim3(blocks), dim3(256), 0, stream, dy, ap, Cout, p.dy_image.nt, p.nslice);
    else
        hipLaunchKernelGGL(pack_wgrad_dy_kernel, dim3(blocks), dim3(256), 0, stream, dy, ap, g, Cout, p.dy_image.nt, p.nslice,
                           FastDiv(g.OW / 8), FastDiv(g.OH / 8), FastDiv(g.OD));
}

static HaloWgradArgs halo_wgrad_args(const HaloWgradPlan& p, const float* x, float* dw, int Cin, int Cin_total, int Cout,
                                     const ConvGeom& g, void* workspace) {
    const bool mode4 = p.kernel == HaloWgradKernel::halo4, direct = p.nsplit == 1;
    HaloWgradArgs a;
    a.ap = workspace_at<float4>(workspace, p.dy_image.offset);
    a.x = x;
    a.ws = direct ? dw : workspace_at<float>(workspace, p.partial_offset);
    a.g = g;
    a.Cin = Cin;
    a.Cout = Cout;
    a.nslice = p.nslice;
    a.per_split = p.per_split;
    a.mt_total = p.dy_image.nt;
    a.ldw = direct ? (long)Cin_total * 64 : (long)Cin * 64;
    a.dntw = FastDiv(mode4 ? 1 : g.OW / 8);
    a.dnth = FastDiv(mode4 ? 1 : g.OH / 8);
    a.dOD = FastDiv(g.OD);
    return a;
}

void halo_wgrad_launch(const HaloWgradPlan& p, const float* x, float* dw, int Cin, int Cin_total, int Cout, const ConvGeom& g,
                       void* workspace, hipStream_t stream) {
    const HaloWgradArgs a = halo_wgrad_args(p, x, dw, Cin, Cin_total, Cout, g, workspace);
    switch (p.kernel) {
    case HaloWgradKernel::halo4:
        hipLaunchKernelGGL(conv_wgrad_halo4_kernel, p.grid, dim3(p.block), p.lds, stream, a);
        break;
    case HaloWgradKernel::rows64:
        hipLaunchKernelGGL((conv_wgrad_halo_kernel<4, false>), p.grid, dim3(p.block), p.lds, stream, a);
        break;
    case HaloWgradKernel::rows128_skip_h:
        hipLaunchKernelGGL((conv_wgrad_halo_kernel<2, true>), p.grid, dim3(p.block), p.lds, stream, a);
        break;
    case HaloWgradKernel::rows128:
        hipLaunchKernelGGL((conv_wgrad_halo_kernel<2, false>), p.grid, dim3(p.block), p.lds, stream, a);
        break;
    }
    if (p.nsplit > 1) {
        const long total = (long)Cout * Cin * 64;
        int fb = (int)((total / 4 + 255) / 256);
        if (fb > 2048) fb = 2048;
        hipLaunchKernelGGL(wgrad_halo_finalize_kernel, dim3(fb), dim3(256), 0, stream, (const float*)a.ws, dw, Cout, Cin * 64,
                           (long)Cin_total * 64, p.nsplit);
    }
}


}  // namespace sg
