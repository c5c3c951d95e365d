// shapegan_amd/csrc/topology_core.h — the per-element statements of mesh topology (K12b): which triangles count, the half-edge keys,
// the per-triangle area and volume terms, the tile of the ordered sums.
//
// Included by csrc/topology.hip and the twin (core_fn.h has the conventions).  What each library keeps: the union-find, the scans, the
// walks over the sorted runs and the summation in the header's order.
#pragma once
#include "core_fn.h"

#define SG_TOPO_TILE 256                         // terms per tile of the ordered area / volume sums
#define SG_TOPO_NO_COMPONENT 2147483647          // triangle key of a skipped triangle: sorts behind every component
#define SG_TOPO_NO_EDGE 9223372036854775807LL    // half-edge key of a side that is no edge: sorts behind every edge

// the shape that owns element i of a packed array: the s with offsets[s] <= i < offsets[s + 1] (empty shapes own nothing), clamped
SG_CORE_FN long sg_topo_shape_of(const int64_t* offsets, long S, long i) {
    long lo = 0, hi = S - 1;
    while (lo < hi) {
        const long mid = lo + (hi - lo) / 2;
        if (offsets[mid + 1] <= i)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// a triangle counts when its three indices lie in [0, n) of its shape and inside the vertex array; a, b, c: its GLOBAL vertex indices
SG_CORE_FN bool sg_topo_triangle(const int64_t* face, long vbase, long n, long V, long& a, long& b, long& c) {
    const long i = face[0], j = face[1], k = face[2];
    if (i < 0 || j < 0 || k < 0 || i >= n || j >= n || k >= n || vbase < 0 || vbase + n > V) return false;
    a = vbase + i;
    b = vbase + j;
    c = vbase + k;
    return true;
}

// the key of the side a -> b (global indices below 2^31): (min << 32) | (max << 1) | (1 when the side runs from max to min)
SG_CORE_FN int64_t sg_topo_edge_key(long a, long b) {
    if (a == b) return SG_TOPO_NO_EDGE;
    const long lo = a < b ? a : b, hi = a < b ? b : a;
    return (int64_t)((uint64_t)lo << 32 | (uint64_t)hi << 1 | (uint64_t)(a > b));
}
SG_CORE_FN long sg_topo_edge_low(int64_t key) { return (long)((uint64_t)key >> 32); }
SG_CORE_FN bool sg_topo_same_edge(int64_t x, int64_t y) { return (x >> 1) == (y >> 1); }

// area = |(p1 - p0) x (p2 - p0)| / 2 and volume = p0 . (p1 x p2) / 6 of one triangle, in double from the f32 corners, every fused
// step explicit (the including file switches contraction off)
SG_CORE_FN void sg_topo_terms(const float* p0, const float* p1, const float* p2, double& area, double& volume) {
    const double x0 = p0[0], y0 = p0[1], z0 = p0[2], x1 = p1[0], y1 = p1[1], z1 = p1[2], x2 = p2[0], y2 = p2[1], z2 = p2[2];
    const double ax = x1 - x0, ay = y1 - y0, az = z1 - z0, bx = x2 - x0, by = y2 - y0, bz = z2 - z0;
    const double cx = __builtin_fma(ay, bz, -(az * by)), cy = __builtin_fma(az, bx, -(ax * bz)), cz = __builtin_fma(ax, by, -(ay * bx));
    area = 0.5 * sqrt(__builtin_fma(cz, cz, __builtin_fma(cy, cy, cx * cx)));
    const double nx = __builtin_fma(y1, z2, -(z1 * y2)), ny = __builtin_fma(z1, x2, -(x1 * z2)), nz = __builtin_fma(x1, y2, -(y1 * x2));
    volume = __builtin_fma(z0, nz, __builtin_fma(y0, ny, x0 * nx)) / 6.0;
}
