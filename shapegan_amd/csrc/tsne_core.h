// shapegan_amd/csrc/tsne_core.h — the per-element arithmetic of exact t-SNE (K17): a squared distance, one step of the perplexity search,
// the terms of a pair of the gradient, the gradient of a row from its sums and the descent step.
//
// Included by csrc/tsne.hip and the twin (core_fn.h has the conventions).  What each library keeps: the loops, the order in which the
// terms of a row are added (partial sums in float, flushed into double) and the reductions over rows.  The two libraries therefore agree
// bit for bit on the squared distances, on the symmetrisation and on the update, and to rounding on everything that goes through expf,
// log, log1pf, the reciprocal of a pair and a sum over a row.
#pragma once
#include "core_fn.h"
#include "../../include/shapegan_hip.h"      // SG_TSNE_*

// one coordinate of |x_i - x_j|^2: a sum of squared DIFFERENCES in increasing k (the |a|^2 + |b|^2 - 2ab form cancels for near
// neighbours).  (a - b)^2 = (b - a)^2 exactly, so d2(i, j) and d2(j, i) are the same bits.
SG_CORE_FN float sg_tsne_d2_step(float acc, float a, float b) {
    const float d = a - b;
    return __builtin_fmaf(d, d, acc);
}

SG_CORE_FN bool sg_tsne_sizes_ok(long N, long D, double perplexity) {
    return N >= 4 && N <= SG_TSNE_MAX_POINTS && D >= 1 && D <= SG_TSNE_MAX_DIMS && perplexity >= 1.0 && perplexity < (double)(N - 1);
}

// The state of one row's search for beta (scikit-learn's _binary_search_perplexity: start at 1, double or halve while one bound is
// open, bisect afterwards).  An open bound is +-INFINITY.
struct SgTsneSearch {
    float beta, lo, hi;
};
SG_CORE_FN void sg_tsne_search_init(SgTsneSearch* s) {
    s->beta = 1.0f;
    s->lo = -INFINITY;
    s->hi = INFINITY;
}
// entropy (nats) of p_j = exp(-beta d_j) / sum_p from the two float64 row sums: sum_p = sum_j exp(-beta d_j), sum_dp = sum_j d_j exp(..)
SG_CORE_FN double sg_tsne_entropy(float beta, double sum_p, double sum_dp) { return log(sum_p) + (double)beta * sum_dp / sum_p; }
// diff = entropy - log(perplexity) at s->beta.  Returns true when the search is over at this beta; otherwise moves to the next.
SG_CORE_FN bool sg_tsne_search_next(SgTsneSearch* s, double diff, double tol) {
    if (fabs(diff) <= tol) return true;
    if (diff > 0.0) {      // too flat: beta must grow
        s->lo = s->beta;
        s->beta = s->hi == INFINITY ? s->beta * 2.0f : (s->beta + s->hi) * 0.5f;
    } else {
        s->hi = s->beta;
        s->beta = s->lo == -INFINITY ? s->beta * 0.5f : (s->beta + s->lo) * 0.5f;
    }
    return false;
}
SG_CORE_FN float sg_tsne_cond(float beta, float d) { return expf(-beta * d); }      // d = d2(i, j) - min_j d2(i, j) >= 0

// P_ij = (p_j|i + p_i|j) / 2N: the sum commutes, so P is symmetric bit for bit
SG_CORE_FN float sg_tsne_joint(float a, float b, float two_n) { return (a + b) / two_n; }

// 1 / (1 + q) of a pair: the hardware reciprocal (1 ulp) on the GPU, a division on the host
#if defined(__HIP_DEVICE_COMPILE__)
#define SG_TSNE_RCP(x) __builtin_amdgcn_rcpf(x)
#else
#define SG_TSNE_RCP(x) (1.0f / (x))
#endif

// the sums of a row of the gradient, over a short run of columns (the libraries flush them into float64)
struct SgTsneAcc {
    float s, ax, ay, rx, ry, k;
};
SG_CORE_FN void sg_tsne_acc_zero(SgTsneAcc* a) { a->s = a->ax = a->ay = a->rx = a->ry = a->k = 0.f; }
// one pair (i, j): w = 1 / (1 + |y_i - y_j|^2), not counted when j = i or when the column does not exist (live = false)
template <bool KL>
SG_CORE_FN void sg_tsne_pair(SgTsneAcc* a, float yix, float yiy, float yjx, float yjy, float p, bool live) {
    const float dx = yix - yjx, dy = yiy - yjy;
    const float q = __builtin_fmaf(dx, dx, dy * dy);
    const float w = live ? SG_TSNE_RCP(1.0f + q) : 0.0f;
    const float pw = p * w, w2 = w * w;
    a->s += w;
    a->ax = __builtin_fmaf(pw, dx, a->ax);
    a->ay = __builtin_fmaf(pw, dy, a->ay);
    a->rx = __builtin_fmaf(w2, dx, a->rx);
    a->ry = __builtin_fmaf(w2, dy, a->ry);
    if (KL) a->k = __builtin_fmaf(live ? p : 0.0f, log1pf(q), a->k);
}

// grad_i = 4 (exaggeration a_i - r_i / Z), one coordinate
SG_CORE_FN float sg_tsne_grad(double a, double r, double Z, float exaggeration) { return (float)(4.0 * ((double)exaggeration * a - r / Z)); }

// scikit-learn's _gradient_descent step on one element
SG_CORE_FN void sg_tsne_update_one(float* y, float* velocity, float* gains, float grad, float momentum, float lr, float min_gain) {
    const float v = *velocity;
    float g = (v * grad < 0.0f) ? *gains + 0.2f : *gains * 0.8f;
    g = g < min_gain ? min_gain : g;
    const float nv = momentum * v - lr * (g * grad);
    *gains = g;
    *velocity = nv;
    *y = *y + nv;
}
