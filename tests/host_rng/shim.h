// Just enough of the HIP device environment for the host compiler to take csrc/rng_core.cuh and csrc/rng_seed.cuh as
// plain C++: empty qualifiers, and host stand-ins for the three fp32 hardware built-ins of HbRng::normal2(float&, float&)
// and for the device library's sincospi.  The stand-ins round like libm, not like the instructions, so the fp32 normals
// of a host run are not comparable bit for bit with a device run; the stand-ins RECORD their argument, which is how the
// driver reads the u1 and u2 that normal2 forms (those are plain C++: the same bits on both sides).
#pragma once
#include <cmath>
#include <cstdint>
#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))

static float g_log_arg = -1.f, g_cos_arg = -1.f, g_sin_arg = -1.f;
// v_log_f32: log2
static inline float hb_host_log2(float x) {
  g_log_arg = x;
  return (float)std::log2((double)x);
}
// v_cos_f32 / v_sin_f32: argument in revolutions
static inline float hb_host_cos_rev(float x) {
  g_cos_arg = x;
  return (float)std::cos(6.283185307179586476925 * (double)x);
}
static inline float hb_host_sin_rev(float x) {
  g_sin_arg = x;
  return (float)std::sin(6.283185307179586476925 * (double)x);
}
#define __builtin_amdgcn_logf(x) hb_host_log2(x)
#define __builtin_amdgcn_cosf(x) hb_host_cos_rev(x)
#define __builtin_amdgcn_sinf(x) hb_host_sin_rev(x)

// sin(pi y), cos(pi y): the angle reduced exactly around the nearest multiple of pi/2 first, so the results are good to an
// ulp next to their zeros too
static inline void sincospi(double y, double* sn, double* cs) {
  const double k = std::nearbyint(2.0 * y);
  const double r = y - 0.5 * k;
  const double s = std::sin(3.141592653589793238463 * r), c = std::cos(3.141592653589793238463 * r);
  switch ((long)k & 3) {
    case 0: *sn = s, *cs = c; break;
    case 1: *sn = c, *cs = -s; break;
    case 2: *sn = -s, *cs = -c; break;
    default: *sn = -c, *cs = s; break;
  }
}
