// Just enough of the HIP device environment for the host compiler to take csrc/ew_math.cuh and csrc/ew_apply.cuh as
// plain C++: empty qualifiers, declarations for the names the (never instantiated) wave / block sums mention, and host
// stand-ins for the two fp32 hardware built-ins of hb_sigmoid<float>.  The stand-ins round like libm, not like the
// instructions, so SIGMOID and SOFTPLUS_GRAD in fp32 are not comparable bit for bit with a device run; everything else
// in the op table is the same C++ on both sides.
#pragma once
#include <cmath>
#define __device__
#define __forceinline__ inline __attribute__((always_inline))
struct hb_host_dim3 {
  unsigned x, y, z;
};
static hb_host_dim3 threadIdx = {0, 0, 0}, blockDim = {1, 1, 1};
static inline void __syncthreads() {}
template <typename T>
static inline T __shfl_xor(T v, int, int) { return v; }
static inline float hb_host_fast_expf(float x) { return exp2f(0x1.715476p+0f * x); }
#define __expf(x) hb_host_fast_expf(x)   // (glibc declares a __expf of its own)
#define __builtin_amdgcn_rcpf(x) (1.0f / (x))
