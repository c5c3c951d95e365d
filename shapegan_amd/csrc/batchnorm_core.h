// shapegan_amd/csrc/batchnorm_core.h — the host-side plan of the BatchNorm kernels (K4) and the slice / walk arithmetic they run on,
// shared with the twin (sg_bn_plan_cpu answers from the same functions).
//
// A channel of x [N, C, S] is the flat range e in [0, N * S): sample n = e / S, position s = e % S.  The statistics passes cut it into
// `nsplit` slices, the apply passes into `napply` >= nsplit slices; a slice is a multiple of 4 elements long (the last one ragged), so
// with S % 4 == 0 every slice starts on a float4 group and no group straddles two samples.
#pragma once
#include "core_fn.h"

// slices per channel of the statistics passes: ~4 workgroups per CU overall, each slice at least 4096 elements, at most 64 (the
// partials of a channel are combined by one wave)
SG_CORE_FN int sg_bn_nsplit(int N, int C, long S) {
    const long per = (long)N * S;
    long want = 1024 / (C > 0 ? C : 1);
    if (want < 1) want = 1;
    long maxs = per / 4096;
    if (maxs < 1) maxs = 1;
    long s = want < maxs ? want : maxs;
    if (s > 64) s = 64;
    return (int)s;
}
// slices per channel of the apply passes: enough workgroups to fill the chip (~8 per CU), each at least 4096 elements
SG_CORE_FN int sg_bn_apply_split(int N, int C, long S) {
    const long per = (long)N * S;
    long want = (2048 + C - 1) / (C > 0 ? C : 1);
    long maxs = per / 4096;
    if (maxs < 1) maxs = 1;
    long s = want < maxs ? want : maxs;
    if (s > 1024) s = 1024;
    if (s < 1) s = 1;
    return (int)s;
}
// slice `sp` of `nsplit` of a channel of `total` elements: [*beg, *end)
SG_CORE_FN void sg_bn_slice(long total, int nsplit, int sp, long* beg, long* end) {
    const long chunk = ((total + nsplit - 1) / nsplit + 3) & ~3L;
    *beg = sp * chunk;
    *end = total < *beg + chunk ? total : *beg + chunk;
}
// flat index e of channel c -> offset in x [N, C, S]
SG_CORE_FN long sg_bn_chan_addr(long e, int c, int C, long S) {
    const long n = e / S, s = e - n * S;
    return (n * C + c) * S + s;
}
// the same walk without a 64-bit division per element: a float4 group at flat index e (e % 4 == 0, S % 4 == 0 so a group never
// straddles two samples) and steps of `step` elements
#if defined(__HIPCC__)
#define SG_BN_MEMBER __host__ __device__ __forceinline__
#else
#define SG_BN_MEMBER inline
#endif
struct SgChanWalk {
    long n, s, S;
    int c, C;
    SG_BN_MEMBER SgChanWalk(long e, int c_, int C_, long S_) : S(S_), c(c_), C(C_) {
        n = e / S_;
        s = e - n * S_;
    }
    SG_BN_MEMBER long addr() const { return (n * C + c) * S + s; }
    SG_BN_MEMBER void advance(long step) {
        s += step;
        if (s >= S) {
            if (step <= S) {
                s -= S;
                ++n;
            } else {
                const long k = s / S;
                n += k;
                s -= k * S;
            }
        }
    }
};
// The shift K of channel c's statistics sums (x: one group's [N, C, S]): the channel's first element.
SG_CORE_FN float sg_bn_shift(const float* x, int c, long S) { return x[(long)c * S]; }
// Whether that shift was too far from the mean for the fp32 sums: m = E[x - K] and var = E[(x-K)^2] - m^2 as the sums give them.  The
// cancellation in E[(x-K)^2] - m^2 multiplies the sums' rounding by 1 + m^2 / var; measured against float64 (tests/batchnorm_forms.py)
// invstd is off by about 0.05 (1 + m^2 / var) 2^-24, and a first element 25 std out (a factor of 600) already put dx beyond its bound.
// Beyond 8 std (a factor of 64) the statistics are therefore formed again around K + m (bn_group_stats).  A Gaussian first element
// never is 8 std from the mean, so channels without such an element keep the one-pass sums and their bits.
SG_CORE_FN bool sg_bn_shift_was_far(double m, double var) { return m * m > 64.0 * var; }
