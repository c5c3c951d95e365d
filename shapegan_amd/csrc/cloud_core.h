// shapegan_amd/csrc/cloud_core.h — the arithmetic of signed distances from oriented point clouds (K19): the order of a neighbour
// list, the normal of a neighbourhood, the vote of a normal.
//
// Included by csrc/cloud.hip and the twin (core_fn.h has the conventions).  What each library keeps: the walk over the cloud and the
// list of the K best pairs; the pair's d2 is sg_pc_d2 of pointcloud_core.h.
#pragma once
#include "core_fn.h"
#include "pointcloud_core.h"

#define SG_CLOUD_JACOBI_SWEEPS 6

// (d, i) comes before (D, I) in the order of a neighbour list; NaN comes before nothing and nothing comes before NaN
SG_CORE_FN bool sg_cloud_before(float d, int i, float D, int I) { return d < D || (d == D && i < I); }

// the vote of one neighbour p with normal n on the query q: negative = the query is behind the sample
SG_CORE_FN float sg_cloud_vote(float qx, float qy, float qz, float px, float py, float pz, float nx, float ny, float nz) {
    const float dx = qx - px, dy = qy - py, dz = qz - pz;
    return __builtin_fmaf(dz, nz, __builtin_fmaf(dy, ny, dx * nx));
}

// sdf of a query from the smallest d2 of its list, the number of valid neighbours and the number of negative votes
SG_CORE_FN float sg_cloud_signed(float d2_first, int valid, int negative) {
    const float d = sqrtf(d2_first);
    return 2 * negative > valid ? -d : d;
}

// one Jacobi rotation of the pair (p, q) of a symmetric 3x3: app, aqq, apq its 2x2 block, (arp, arq) the remaining row, (v?p, v?q) the
// two columns of the eigenvector matrix
SG_CORE_FN void sg_cloud_rotate(float& app, float& aqq, float& apq, float& arp, float& arq, float& v0p, float& v0q, float& v1p,
                                float& v1q, float& v2p, float& v2q) {
    if (apq == 0.f) return;
    const float theta = (aqq - app) / (2.f * apq);
    const float t = copysignf(1.f, theta) / (fabsf(theta) + sqrtf(__builtin_fmaf(theta, theta, 1.f)));
    const float c = 1.f / sqrtf(__builtin_fmaf(t, t, 1.f));
    const float s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.f;
    float x = arp, y = arq;
    arp = __builtin_fmaf(c, x, -(s * y));
    arq = __builtin_fmaf(s, x, c * y);
    x = v0p, y = v0q;
    v0p = __builtin_fmaf(c, x, -(s * y));
    v0q = __builtin_fmaf(s, x, c * y);
    x = v1p, y = v1q;
    v1p = __builtin_fmaf(c, x, -(s * y));
    v1q = __builtin_fmaf(s, x, c * y);
    x = v2p, y = v2q;
    v2p = __builtin_fmaf(c, x, -(s * y));
    v2q = __builtin_fmaf(s, x, c * y);
}

// The normal [3] and the surface variation of point `self` of a cloud (`cloud`: its `size` points, [size][3]) from the K slots of its
// neighbour list; view: (x, y, z, w) or NULL.  Slots outside [0, size) are not read.
SG_CORE_FN void sg_cloud_normal(const float* cloud, long size, long self, const int* slots, int K, const float* view, float* normal,
                                float* variation) {
    const float px = cloud[self * 3], py = cloud[self * 3 + 1], pz = cloud[self * 3 + 2];
    // the centroid of the samples relative to the point; the point itself is the sample (0, 0, 0)
    int n = 1;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int k = 0; k < K; ++k) {
        const long j = slots[k];
        if (j < 0 || j >= size) continue;
        sx += cloud[j * 3] - px;
        sy += cloud[j * 3 + 1] - py;
        sz += cloud[j * 3 + 2] - pz;
        ++n;
    }
    normal[0] = normal[1] = normal[2] = 0.f;
    *variation = -1.f;
    if (n < 3) return;
    const float cx = sx / (float)n, cy = sy / (float)n, cz = sz / (float)n;
    float ex = 0.f - cx, ey = 0.f - cy, ez = 0.f - cz;
    float a00 = ex * ex, a01 = ex * ey, a02 = ex * ez, a11 = ey * ey, a12 = ey * ez, a22 = ez * ez;
    for (int k = 0; k < K; ++k) {
        const long j = slots[k];
        if (j < 0 || j >= size) continue;
        ex = (cloud[j * 3] - px) - cx;
        ey = (cloud[j * 3 + 1] - py) - cy;
        ez = (cloud[j * 3 + 2] - pz) - cz;
        a00 = __builtin_fmaf(ex, ex, a00);
        a01 = __builtin_fmaf(ex, ey, a01);
        a02 = __builtin_fmaf(ex, ez, a02);
        a11 = __builtin_fmaf(ey, ey, a11);
        a12 = __builtin_fmaf(ey, ez, a12);
        a22 = __builtin_fmaf(ez, ez, a22);
    }
    float v00 = 1.f, v01 = 0.f, v02 = 0.f, v10 = 0.f, v11 = 1.f, v12 = 0.f, v20 = 0.f, v21 = 0.f, v22 = 1.f;
    for (int sweep = 0; sweep < SG_CLOUD_JACOBI_SWEEPS; ++sweep) {
        sg_cloud_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (0, 1): the remaining row is 2
        sg_cloud_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0, 2): the remaining row is 1
        sg_cloud_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1, 2): the remaining row is 0
    }
    // the column of the smallest eigenvalue, the lowest on a tie
    float l0 = a00, nx = v00, ny = v10, nz = v20;
    if (a11 < l0) l0 = a11, nx = v01, ny = v11, nz = v21;
    if (a22 < l0) l0 = a22, nx = v02, ny = v12, nz = v22;
    const float l2 = fmaxf(fmaxf(a00, a11), a22);
    const float l1 = fmaxf(fminf(a00, a11), fminf(fmaxf(a00, a11), a22));
    if (!(l1 > 9.5367431640625e-07f * l2)) return;      // 2^-20: a line, a point, NaN
    const float len = sqrtf(__builtin_fmaf(nz, nz, __builtin_fmaf(ny, ny, nx * nx)));
    nx = nx / len, ny = ny / len, nz = nz / len;
    bool flip;
    if (view) {
        const float w = view[3];
        const float fx = view[0] - w * px, fy = view[1] - w * py, fz = view[2] - w * pz;
        flip = __builtin_fmaf(nz, fz, __builtin_fmaf(ny, fy, nx * fx)) < 0.f;
    } else {
        float big = nx;
        if (fabsf(ny) > fabsf(big)) big = ny;
        if (fabsf(nz) > fabsf(big)) big = nz;
        flip = big < 0.f;
    }
    normal[0] = flip ? -nx : nx;
    normal[1] = flip ? -ny : ny;
    normal[2] = flip ? -nz : nz;
    *variation = l0 / ((l0 + l1) + l2);
}
