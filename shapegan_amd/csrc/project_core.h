// shapegan_amd/csrc/project_core.h — the step that moves a point toward a level set of an SDFNet, given the network's value and
// gradient at the point (K7d: csrc/sdfnet_project.hip and sg_sdfnet_project_cpu of the twin; header: sg_sdfnet_project).
//
// One statement of the rule for both libraries (core_fn.h has the conventions: contraction off in the including file, every fused
// step an explicit __builtin_fmaf, IEEE division and square root).  float32, in this order:
//   d   = out - level
//   n2  = fma(gx, gx, fma(gy, gy, gz gz))
//   t   = d / n2          rule 0: Newton's step for f(x) = level along the gradient
//       = d / sqrt(n2)    rule 1: the reference's step, which takes |grad f| = 1 for granted (model/sdf_net.py:146)
//   s   = t g,  len = |t| sqrt(n2);  max_step > 0 and len > max_step: s *= max_step / len
//   !(n2 > 0) or a component of s not finite: s = 0      (a flat spot, or an overflow: the point stays where it is)
//   x  -= s
#pragma once
#include "core_fn.h"

#define SG_PROJECT_RULE_NEWTON 0
#define SG_PROJECT_RULE_UNIT 1

SG_CORE_FN void sg_project_step(float* x, float out, const float* g, float level, int rule, float max_step) {
    const float d = out - level;
    const float n2 = __builtin_fmaf(g[0], g[0], __builtin_fmaf(g[1], g[1], g[2] * g[2]));
    const float nrm = sqrtf(n2);
    const float t = rule == SG_PROJECT_RULE_NEWTON ? d / n2 : d / nrm;
    float s0 = t * g[0], s1 = t * g[1], s2 = t * g[2];
    const float len = fabsf(t) * nrm;
    if (max_step > 0.f && len > max_step) {
        const float c = max_step / len;
        s0 *= c;
        s1 *= c;
        s2 *= c;
    }
    const bool finite = fabsf(s0) <= 3.402823466e38f && fabsf(s1) <= 3.402823466e38f && fabsf(s2) <= 3.402823466e38f;      // (false for NaN)
    if (!(n2 > 0.f) || !finite) s0 = s1 = s2 = 0.f;
    x[0] -= s0;
    x[1] -= s1;
    x[2] -= s2;
}
