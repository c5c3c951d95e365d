// shapegan_amd/csrc/brickgrid_core.h — the integer and side-of-level arithmetic of the narrow-band voxel grid (K18,
// include/shapegan_hip.h).
//
// Included by csrc/brickgrid.hip and by the twin (core_fn.h has the conventions).  What each library keeps: the walk over bricks and
// points, the scan that orders a list, and the reduction of a brick's points to its two region masks.
#pragma once
#include "core_fn.h"

// The lattice of one call: S shapes of R^3 points (flat index x R^2 + y R + z) cut into (R / B)^3 bricks of B^3 points.  Brick
// (bx, by, bz) of shape s has the global id s * nb + (bx * nbx + by) * nbx + bz; point (lx, ly, lz) of a brick has the local index
// lx B^2 + ly B + lz.
struct SgBrickGeom {
    long S, nb;      // shapes, bricks per shape
    int R, B, nbx;   // lattice points per axis, brick edge, bricks per axis
    int shift;       // log2(B)
};

// fills g; false when an argument is out of range or a global brick id would not stay below 2^31
SG_CORE_FN bool sg_brick_geom(SgBrickGeom& g, long S, int R, int B) {
    if (S <= 0 || R <= 0 || R > 2048 || (B != 4 && B != 8 && B != 16) || R % B != 0) return false;
    g.S = S;
    g.R = R;
    g.B = B;
    g.nbx = R / B;
    g.shift = B == 4 ? 2 : B == 8 ? 3 : 4;
    g.nb = (long)g.nbx * g.nbx * g.nbx;
    return S <= 2147483647L / g.nb;
}

// a value is inside when it is below the level: K12's test
SG_CORE_FN bool sg_brick_inside(float v, float level) { return v < level; }

SG_CORE_FN void sg_brick_decode(const SgBrickGeom& g, long brick, long& s, int& bx, int& by, int& bz) {
    s = brick / g.nb;
    const int b = (int)(brick - s * g.nb);
    bx = b / (g.nbx * g.nbx);
    by = (b / g.nbx) % g.nbx;
    bz = b % g.nbx;
}

// lattice index (within one shape) of local point (lx, ly, lz) of brick (bx, by, bz)
SG_CORE_FN long sg_brick_lattice(const SgBrickGeom& g, int bx, int by, int bz, int lx, int ly, int lz) {
    return ((long)(bx * g.B + lx) * g.R + (by * g.B + ly)) * g.R + (bz * g.B + lz);
}

// corner n of a brick: local offset ((n >> 2) & 1, (n >> 1) & 1, n & 1) * (B - 1); n = 0 is the lowest-index corner
SG_CORE_FN void sg_brick_corner_local(const SgBrickGeom& g, int n, int& lx, int& ly, int& lz) {
    lx = ((n >> 2) & 1) * (g.B - 1);
    ly = ((n >> 1) & 1) * (g.B - 1);
    lz = (n & 1) * (g.B - 1);
}

// the value corner n of a brick counts with: the network's (corner_values [S nb][8]), or 1 where the mask (NULL: none) leaves it out
SG_CORE_FN float sg_brick_corner_value(const SgBrickGeom& g, const float* corner_values, const unsigned char* mask, long s, int bx, int by,
                                       int bz, int n) {
    int lx, ly, lz;
    sg_brick_corner_local(g, n, lx, ly, lz);
    if (mask && !mask[sg_brick_lattice(g, bx, by, bz, lx, ly, lz)]) return 1.f;
    return corner_values[(s * g.nb + ((long)(bx * g.nbx + by) * g.nbx + bz)) * 8 + n];
}

// Seed rules (a)-(d) for one brick; *fill receives the brick's fill (its corner 0).
SG_CORE_FN bool sg_brick_seed_test(const SgBrickGeom& g, const float* corner_values, const unsigned char* mask, long s, int bx, int by,
                                   int bz, float level, float band, int pad, float* fill) {
    const float v0 = sg_brick_corner_value(g, corner_values, mask, s, bx, by, bz, 0);
    const bool f = sg_brick_inside(v0, level);
    *fill = v0;
    bool mixed = false, near = false, any_in = false;
    for (int n = 0; n < 8; ++n) {
        const float v = sg_brick_corner_value(g, corner_values, mask, s, bx, by, bz, n);
        const bool in = sg_brick_inside(v, level);
        mixed = mixed || in != f;                      // (a)
        near = near || fabsf(v - level) <= band;       // (b)
        any_in = any_in || in;
    }
    const int e = g.nbx - 1;
    const bool border = bx == 0 || by == 0 || bz == 0 || bx == e || by == e || bz == e;
    if (mixed || near || (pad && border && any_in)) return true;   // (c): the virtual shell of 1 makes a crossing
    for (int d = 0; d < 27; ++d) {                     // (d): a neighbour's fill on the other side
        const int nx = bx + d / 9 - 1, ny = by + (d / 3) % 3 - 1, nz = bz + d % 3 - 1;
        if (d == 13 || nx < 0 || ny < 0 || nz < 0 || nx > e || ny > e || nz > e) continue;
        if (sg_brick_inside(sg_brick_corner_value(g, corner_values, mask, s, nx, ny, nz, 0), level) != f) return true;
    }
    return false;
}

// Continuation.  Direction d = (dx + 1) * 9 + (dy + 1) * 3 + (dz + 1) names one of the 26 neighbours of a brick (d = 13: itself).
// Bit d of the region mask of local point (lx, ly, lz): the point lies within Chebyshev distance 2 of some point of neighbour d.
SG_CORE_FN unsigned sg_brick_region_mask(int B, int lx, int ly, int lz) {
    const unsigned ax = 2u | (lx < 2 ? 1u : 0u) | (lx >= B - 2 ? 4u : 0u);
    const unsigned ay = 2u | (ly < 2 ? 1u : 0u) | (ly >= B - 2 ? 4u : 0u);
    const unsigned az = 2u | (lz < 2 ? 1u : 0u) | (lz >= B - 2 ? 4u : 0u);
    unsigned m = 0;
    for (int d = 0; d < 27; ++d)
        if (((ax >> (d / 9)) & 1u) && ((ay >> ((d / 3) % 3)) & 1u) && ((az >> (d % 3)) & 1u)) m |= 1u << d;
    return m & ~(1u << 13);
}

// `brick` is newly active; in_mask / out_mask: the union of the region masks of its inside / outside points.  Neighbour d, when it
// exists and is inactive, is flagged if the brick has a point near it on the other side of the level than the neighbour's fill.
SG_CORE_FN void sg_brick_grow_apply(const SgBrickGeom& g, const int* state, const float* fill, int* flag, long brick, int d, unsigned in_mask,
                                    unsigned out_mask, float level) {
    long s;
    int bx, by, bz;
    sg_brick_decode(g, brick, s, bx, by, bz);
    const int nx = bx + d / 9 - 1, ny = by + (d / 3) % 3 - 1, nz = bz + d % 3 - 1, e = g.nbx - 1;
    if (d == 13 || nx < 0 || ny < 0 || nz < 0 || nx > e || ny > e || nz > e) return;
    const long n = s * g.nb + ((long)(nx * g.nbx + ny) * g.nbx + nz);
    if (state[n] != 0) return;
    const unsigned other = sg_brick_inside(fill[n], level) ? out_mask : in_mask;
    if ((other >> d) & 1u) flag[n] = 1;
}
