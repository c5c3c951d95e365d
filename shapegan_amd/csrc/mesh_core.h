// shapegan_amd/csrc/mesh_core.h — the per-cell arithmetic of marching cubes and of surface sampling (K12, include/shapegan_hip.h).
//
// Included by csrc/mesh.hip and by the twin (core_fn.h has the conventions).  What each library keeps: the walk over the cells, the
// counts and prefix sums that place every vertex and triangle, and the summation of the areas (a tree there, sequential in the twin).
#pragma once
#include "core_fn.h"
#include "mc_tables.h"

// The (virtually padded) grid of one call.  The "cells" are its corners, P0 x P1 x P2: corner (a, b, c) owns the edges toward +1 along
// each axis that exist and, when a + 1 < P0, b + 1 < P1 and c + 1 < P2, the cube with that minimum corner.
struct SgMcGrid {
    int R0, R1, R2;
    int P0, P1, P2;   // corner counts of the padded grid
    int pad;
    float pad_value, level;
};

enum { SG_MC_SLOTS = 24 };   // image entries are vertex * 8 | mask with up to 3 vertices per cell

// fills m; false when an argument is out of range or an int32 index (S * cells * SG_MC_SLOTS) would not stay below 2^31
SG_CORE_FN bool sg_mc_grid(SgMcGrid& m, long S, int R0, int R1, int R2, float level, int pad, float pad_value, long& cells) {
    if (S <= 0 || R0 <= 0 || R1 <= 0 || R2 <= 0 || (pad != 0 && pad != 1)) return false;
    m.R0 = R0;
    m.R1 = R1;
    m.R2 = R2;
    m.P0 = R0 + 2 * pad;
    m.P1 = R1 + 2 * pad;
    m.P2 = R2 + 2 * pad;
    m.pad = pad;
    m.pad_value = pad_value;
    m.level = level;
    cells = (long)m.P0 * m.P1 * m.P2;
    const long lim = 2147483647L / SG_MC_SLOTS;
    return cells <= lim && S <= lim / cells;
}

SG_CORE_FN float sg_mc_value(const SgMcGrid& m, const float* g, int a, int b, int c) {
    if (m.pad) {
        a -= 1;
        b -= 1;
        c -= 1;
        if ((unsigned)a >= (unsigned)m.R0 || (unsigned)b >= (unsigned)m.R1 || (unsigned)c >= (unsigned)m.R2) return m.pad_value;
    }
    return g[((long)a * m.R1 + b) * m.R2 + c];
}

// corner n of the cell at (a, b, c): offset ((n >> 2) & 1, (n >> 1) & 1, n & 1); corners outside the grid read as pad_value
// (they belong only to edges and cubes that do not exist, whose results are discarded)
SG_CORE_FN void sg_mc_corners(const SgMcGrid& m, const float* g, int a, int b, int c, float v[8]) {
    SG_CORE_UNROLL for (int n = 0; n < 8; ++n) {
        const int x = a + ((n >> 2) & 1), y = b + ((n >> 1) & 1), z = c + (n & 1);
        v[n] = (x < m.P0 && y < m.P1 && z < m.P2) ? sg_mc_value(m, g, x, y, z) : m.pad_value;
    }
}

struct SgMcCell {
    int mask;   // bit k: the edge along axis k owned by this cell crosses the level
    int nv, nt;
    int cube;   // case index, -1 when the cell has no cube
};

SG_CORE_FN SgMcCell sg_mc_classify(const SgMcGrid& m, const float v[8], int a, int b, int c) {
    SgMcCell r;
    int cs = 0;
    SG_CORE_UNROLL for (int n = 0; n < 8; ++n) cs |= (v[n] < m.level ? 1 : 0) << n;
    const int in0 = cs & 1;
    r.mask = 0;
    if (a + 1 < m.P0 && in0 != ((cs >> 4) & 1)) r.mask |= 1;
    if (b + 1 < m.P1 && in0 != ((cs >> 2) & 1)) r.mask |= 2;
    if (c + 1 < m.P2 && in0 != ((cs >> 1) & 1)) r.mask |= 4;
    r.nv = __builtin_popcount(r.mask);
    const bool has_cube = a + 1 < m.P0 && b + 1 < m.P1 && c + 1 < m.P2;
    r.cube = has_cube ? cs : -1;
    r.nt = has_cube ? (int)sg_mc_tri_count[cs] : 0;
    return r;
}

// gradient of the padded grid at corner (a, b, c) along `axis`: central difference inside, one-sided at the outermost layer
SG_CORE_FN float sg_mc_grad(const SgMcGrid& m, const float* g, int a, int b, int c, int axis, float spacing) {
    const int p = axis == 0 ? a : axis == 1 ? b : c;
    const int P = axis == 0 ? m.P0 : axis == 1 ? m.P1 : m.P2;
    const int lo = p > 0 ? p - 1 : p, hi = p < P - 1 ? p + 1 : p;
    if (hi == lo) return 0.f;
    float vl, vh;
    if (axis == 0) {
        vl = sg_mc_value(m, g, lo, b, c);
        vh = sg_mc_value(m, g, hi, b, c);
    } else if (axis == 1) {
        vl = sg_mc_value(m, g, a, lo, c);
        vh = sg_mc_value(m, g, a, hi, c);
    } else {
        vl = sg_mc_value(m, g, a, b, lo);
        vh = sg_mc_value(m, g, a, b, hi);
    }
    return (vh - vl) / ((float)(hi - lo) * spacing);
}

// The vertex on the edge along `axis` that cell (a, b, c) owns: v = the cell's corners, g0 = the gradient at (a, b, c), sp / org =
// spacing and origin.  The position interpolates the crossing, the normal the two end gradients (zero when that has no length).
SG_CORE_FN void sg_mc_vertex(const SgMcGrid& m, const float* g, const float* sp, const float* org, int a, int b, int c, const float v[8],
                             const float g0[3], int axis, float pos[3], float nrm[3]) {
    const int idx[3] = {a, b, c};
    const float va = v[0], vb = v[axis == 0 ? 4 : axis == 1 ? 2 : 1];
    const float t = (m.level - va) / (vb - va);
    const int a1 = a + (axis == 0), b1 = b + (axis == 1), c1 = c + (axis == 2);
    float n[3];
    SG_CORE_UNROLL for (int k = 0; k < 3; ++k) {
        const float g1 = sg_mc_grad(m, g, a1, b1, c1, k, sp[k]);
        n[k] = g0[k] + t * (g1 - g0[k]);
    }
    const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    SG_CORE_UNROLL for (int k = 0; k < 3; ++k) {
        pos[k] = ((float)idx[k] + (k == axis ? t : 0.f)) * sp[k] + org[k];
        nrm[k] = len > 0.f ? n[k] / len : 0.f;
    }
}

// Edge code e of a triangle corner (mc_tables.h): its axis, and the offset of the cell that owns it (the edge's minimum corner: the two
// other axes, in increasing order, take the offsets u, w).  sg_mc_rank: the place of that edge's vertex among the owner's vertices.
SG_CORE_FN int sg_mc_edge_owner(int e, int& oa, int& ob, int& oc) {
    const int axis = e >> 2, u = (e >> 1) & 1, w = e & 1;
    oa = axis == 0 ? 0 : u;
    ob = axis == 1 ? 0 : (axis == 0 ? u : w);
    oc = axis == 2 ? 0 : w;
    return axis;
}
SG_CORE_FN int sg_mc_rank(int mask, int axis) { return __builtin_popcount((mask & 7) & ((1 << axis) - 1)); }

// ---- surface sampling ----
// the doubled area of the triangle (p0, p1, p2), in double
SG_CORE_FN double sg_mesh_area2(const float* p0, const float* p1, const float* p2) {
    const double ax = (double)p1[0] - (double)p0[0], ay = (double)p1[1] - (double)p0[1], az = (double)p1[2] - (double)p0[2];
    const double bx = (double)p2[0] - (double)p0[0], by = (double)p2[1] - (double)p0[1], bz = (double)p2[2] - (double)p0[2];
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    return sqrt(cx * cx + cy * cy + cz * cz);
}

// the point at barycentric (u1, u2) of the triangle, the draw reflected into it when u1 + u2 > 1
SG_CORE_FN void sg_mesh_point(const float* p0, const float* p1, const float* p2, float u1, float u2, float out[3]) {
    float p = u1, q = u2;
    if (p + q > 1.f) {
        p = 1.f - p;
        q = 1.f - q;
    }
    SG_CORE_UNROLL for (int k = 0; k < 3; ++k) out[k] = p0[k] + (p * (p1[k] - p0[k]) + q * (p2[k] - p0[k]));
}
