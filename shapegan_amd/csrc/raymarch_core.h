// shapegan_amd/csrc/raymarch_core.h — the per-ray and per-pixel arithmetic of the sphere tracer (include/shapegan_hip.h: sg_raymarch_*).
//
// Included by csrc/raymarch.hip and by the twin (core_fn.h has the conventions).  What each library keeps: the SDFNet evaluation, the
// active lists and their compaction, the counts and offsets of hits and ground rays.
#pragma once
#include "core_fn.h"

// ---- camera rays (raymarching.py:65-102) ----
// camera = position, right, up, forward (3 doubles each) and the focal length; cc = |position|^2 - radius^2; p = on entry the position
// in float32.  Writes the direction d of pixel pix of a W x W image and moves p to the ray's entry into the bounding sphere; a ray that
// misses the sphere keeps p and returns false (it is never marched, raymarching.py:91-97).
SG_CORE_FN bool sg_rm_camera_ray(const double* camera, double cc, int W, long pix, float d[3], float p[3]) {
    // np.linspace(-1, 1, W): i * (2 / (W - 1)) - 1, the last one exactly 1; meshgrid: x along a row, y down the rows
    const long row = pix / W, col = pix - row * W;
    const double step = W > 1 ? 2.0 / (double)(W - 1) : 0.0;
    const double sx = col == W - 1 && W > 1 ? 1.0 : (double)col * step + -1.0;
    const double sy = row == W - 1 && W > 1 ? 1.0 : (double)row * step + -1.0;
    SG_CORE_UNROLL for (int c = 0; c < 3; ++c) d[c] = (float)(sx * camera[3 + c] + sy * camera[6 + c] + camera[12] * camera[9 + c]);
    const float n = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    SG_CORE_UNROLL for (int c = 0; c < 3; ++c) d[c] = d[c] / n;
    const float b = (p[0] * d[0] + p[1] * d[1] + p[2] * d[2]) * 2.f;
    const double disc = (double)(b * b) - 4.0 * cc;
    if (!(disc >= 0.0)) return false;
    const double t = (-(double)b - sqrt(disc)) / 2.0;
    SG_CORE_UNROLL for (int c = 0; c < 3; ++c) p[c] = (float)((double)p[c] + (double)d[c] * t);
    return true;
}

// ---- one march step of one ray (raymarching.py:106-117, :47-55) ----
// p += d * s; the ray has hit if 0 < s < threshold; otherwise it leaves by p.y > radius (shadow rays) or by |p| > radius, or survives
SG_CORE_FN void sg_rm_move(float* p, const float* d, float s) {
    const float x = p[0] + d[0] * s, y = p[1] + d[1] * s, z = p[2] + d[2] * s;
    p[0] = x;
    p[1] = y;
    p[2] = z;
}
SG_CORE_FN bool sg_rm_hit(float s, float threshold) { return s > 0.f && s < threshold; }
SG_CORE_FN bool sg_rm_left(const float* p, float radius, int shadow) {
    return shadow ? p[1] > radius : sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]) > radius;
}

// ---- ground plane (raymarching.py:159-163) ----
// the ground point q of a non-hit pixel looking down: its ray (p, d) meets y = ground within |xz| < 3
SG_CORE_FN bool sg_rm_ground_point(unsigned char status, const float* p, const float* d, float ground, float q[3]) {
    if (!(d[1] < 0.f) || status) return false;
    const float t = (p[1] - ground) / d[1];
    SG_CORE_UNROLL for (int c = 0; c < 3; ++c) q[c] = p[c] - d[c] * t;
    return sqrtf(q[0] * q[0] + q[2] * q[2]) < 3.f;
}

// ---- shadow ray towards the light from q (raymarching.py:37-42): direction in float64, cast; start q + 0.1 d ----
SG_CORE_FN void sg_rm_shadow_ray(const double* light, const float* q, float* sdir, float* spos) {
    double d[3];
    SG_CORE_UNROLL for (int c = 0; c < 3; ++c) d[c] = light[c] - (double)q[c];
    const double n = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    SG_CORE_UNROLL for (int c = 0; c < 3; ++c) {
        const float df = (float)(d[c] / n);
        sdir[c] = df;
        spos[c] = q[c] + df * 0.1f;
    }
}

// ---- shading (raymarching.py:130-175): float64 like the reference's numpy, uint8 by truncation ----
// k = the pixel's slot (hit index, -2 - ground index, or -1), d = its ray direction, grad = d sdf / d p of the hits (normalised here),
// shadow = the shadow rays' status (hits, then ground rays from nhits)
SG_CORE_FN void sg_rm_shade(int k, const float* d, const float* hit_pos, const float* grad, const unsigned char* shadow, long nhits,
                            const double* light, const double* color, unsigned char* rgb) {
    double px[3] = {1.0, 1.0, 1.0};
    if (k >= 0) {
        const float* g = grad + (long)k * 3;
        const float gn = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
        const float nf[3] = {g[0] / gn, g[1] / gn, g[2] / gn};
        const double seen = (double)(1.f - (float)shadow[k]);
        double ld[3];
        SG_CORE_UNROLL for (int c = 0; c < 3; ++c) ld[c] = light[c] - (double)hit_pos[(long)k * 3 + c];
        const double ln = sqrt(ld[0] * ld[0] + ld[1] * ld[1] + ld[2] * ld[2]);
        SG_CORE_UNROLL for (int c = 0; c < 3; ++c) ld[c] = ld[c] / ln;
        const double dn = ld[0] * nf[0] + ld[1] * nf[1] + ld[2] * nf[2];
        const double diffuse = fmin(fmax(dn, 0.0), 1.0) * seen;
        double rf[3];
        SG_CORE_UNROLL for (int c = 0; c < 3; ++c) rf[c] = ld[c] - dn * (double)nf[c] * 2.0;
        const double rn = sqrt(rf[0] * rf[0] + rf[1] * rf[1] + rf[2] * rf[2]);
        double spec = (rf[0] / rn) * d[0] + (rf[1] / rn) * d[1] + (rf[2] / rn) * d[2];
        spec = fmin(fmax(spec, 0.0), 1.0);
        spec = pow(spec, 20.0) * seen;
        float rim = -(nf[0] * d[0] + nf[1] * d[1] + nf[2] * d[2]);
        rim = 1.f - fminf(fmaxf(rim, 0.f), 1.f);
        rim = rim * rim * rim * rim * 0.3f;
        SG_CORE_UNROLL for (int c = 0; c < 3; ++c) px[c] = fmin(fmax(color[c] * (diffuse * 0.5 + 0.5) + (spec * 0.3 + (double)rim), 0.0), 1.0);
    } else if (k <= -2) {
        const double dk = (double)(0.35f * (float)shadow[nhits + (-2 - k)]);
        SG_CORE_UNROLL for (int c = 0; c < 3; ++c) px[c] -= dk;
    }
    SG_CORE_UNROLL for (int c = 0; c < 3; ++c) rgb[c] = (unsigned char)(px[c] * 255.0);
}
