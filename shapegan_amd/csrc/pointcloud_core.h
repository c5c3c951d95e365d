// shapegan_amd/csrc/pointcloud_core.h — the per-pair arithmetic of point-cloud evaluation (K13) and of the earth mover's distance (K15).
//
// Included by csrc/pointcloud.hip, csrc/emd.hip and the twin (core_fn.h has the conventions).  What each library keeps: the walks
// over the clouds, the minima and their summation in the header's order, the auction's lists, bids and rounds.
#pragma once
#include "core_fn.h"
#include "../../include/shapegan_hip.h"      // SG_EMD_*

// squared distance: the header's d2, two explicit fused steps (bitwise symmetric in its two points)
SG_CORE_FN float sg_pc_d2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}

// the occupancy cell of a coordinate in [-0.5, 0.5] on a grid of rm1 + 1 cells per axis, clamped to the grid (NaN -> 0)
SG_CORE_FN int sg_pc_occupancy_axis(float x, float rm1) {
    const float t = (x + 0.5f) * rm1;
    return (int)fminf(fmaxf(floorf(t + 0.5f), 0.f), rm1);
}

// ---- K15 ----
SG_CORE_FN float sg_emd_dist(float ax, float ay, float az, float bx, float by, float bz) { return sqrtf(sg_pc_d2(ax, ay, az, bx, by, bz)); }

// the integer cost of a distance in units of u, capped
SG_CORE_FN int sg_emd_cost(float d, float u) {
    const float q = d / u;
    return q < (float)SG_EMD_MAX_COST ? (int)floorf(q) : SG_EMD_MAX_COST;      // NaN: the comparison is false
}
// a FINITE distance beyond the integer range: eps is too small for the pair (SG_EMD_STATUS_EPS)
SG_CORE_FN bool sg_emd_too_small(float d, float u) { return d < INFINITY && d / u >= (float)SG_EMD_MAX_COST; }

// the largest f32 that is not above eps / 4; 0 when eps is not a positive finite number or eps / 4 is below the normal range
SG_CORE_FN float sg_emd_unit(double eps) {
    if (!(eps > 0.0) || !(eps < (double)INFINITY) || eps / 4 < 1.17549435e-38) return 0.f;
    float u = (float)(eps / 4);
    if ((double)u > eps / 4) u = nextafterf(u, 0.f);
    return u;
}

// what an entry point refuses: 0 = fine, 1 = the sizes (P points per cloud, S clouds), 2 = eps
SG_CORE_FN int sg_emd_refused(long S, long P, double eps) {
    if (P < 1 || P > SG_EMD_MAX_POINTS || S < 1 || S > 65535) return 1;
    return sg_emd_unit(eps) == 0.f ? 2 : 0;
}
