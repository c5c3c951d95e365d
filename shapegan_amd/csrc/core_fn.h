// shapegan_amd/csrc/core_fn.h — what every *_core.h shares: the function qualifier and the order-preserving integer image of a float.
//
// A *_core.h is plain C++ without HIP types, included by its .hip file and by the twin (csrc_cpu/shapegan_cpu.cpp), so the formulas
// it states exist ONCE and the two libraries agree bit for bit.  The including file switches contraction off before the include;
// every fused step is an explicit __builtin_fmaf; division and square root are IEEE (hipcc's default, and g++'s).  Nothing in a core
// header touches memory other than through the pointers it is given.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SG_CORE_FN __host__ __device__ __forceinline__
#define SG_CORE_UNROLL _Pragma("unroll")
#else
#define SG_CORE_FN static inline
#define SG_CORE_UNROLL
#endif

// the order-preserving integer image of a float (signed compare: min of keys = key of min) and back
SG_CORE_FN int sg_float_key(float f) {
    const int b = __builtin_bit_cast(int, f);
    return b >= 0 ? b : b ^ 0x7fffffff;
}
SG_CORE_FN float sg_key_float(int k) { return __builtin_bit_cast(float, k >= 0 ? k : k ^ 0x7fffffff); }
