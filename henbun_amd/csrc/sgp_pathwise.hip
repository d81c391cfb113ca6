// Pathwise posterior function draws of the sparse GP (hb_sgp_pathwise_*, include/henbun_hip.h; not in the reference;
// Wilson et al. 2020, "Efficiently sampling functions from Gaussian process posteriors").
//
// A draw is a coefficient row coef_s = [ w_s / sqrt(L) | v_s ] of length 2L + M; evaluating S draws at n points is one
// contraction
//     out[S, n] = scale * coef[S, 2L + M] . B(x)[2L + M, n],
//     B[2l, j] = cos(p_lj),  B[2l + 1, j] = sin(p_lj),  p_lj = sum_k omega_lk x_jk / ell_k          (prior path)
//     B[2L + m, j] = exp(-1/2 sum_k ((z_mk - x_jk) / ell_k)^2)                                      (update)
// whose right operand is never written to memory: ONE kernel, a workgroup per strip of PW_CN columns (a wave per 32 of
// them), walks the basis rows in K-steps of PW_KT.  Per step each wave synthesises the PW_KT x 32 basis tile of its own
// columns into LDS -- one sincos per (frequency, column) fills the two adjacent rows 2l, 2l + 1; the RBF rows take the
// difference-then-scale exp2 form of sgp_strip.cuh -- the workgroup stages the matching coef tile, and the product runs
// on the 16 x 16 x 4 MFMA of the dtype with the draws on the rows (S padded to 16 inside the kernel).  A basis value is
// synthesised once and applied to every draw of the workgroup (up to PW_SMAX; more draws tile the grid's y).
//
// A draw is a FUNCTION: the K order is the same for every column and every call (the trig rows in steps of PW_KT, the
// tail of the last step zero-filled, then the RBF rows likewise), an MFMA accumulates each output element as a k-ordered
// fma chain of its own, ragged strips read a copy of the last column and mask the store.  So the value at a point does
// not depend on the other points of the call: two calls, or X evaluated in pieces, return the same bits.
//
// Phases reach the hundreds (x hundreds of lengthscales out, |omega| up to 4), where a float phase has lost 1e-5 of a
// radian before any sine is taken.  Both dtypes form the phase in REVOLUTIONS in double, p / 2 pi = sum_k omega_lk
// (x_jk / (2 pi ell_k)), drop the whole revolutions exactly, reduce to a quadrant and evaluate the two Taylor polynomials
// on [-pi/4, pi/4] in double (6 + 6 terms for float, 9 + 10 for double: truncation below 1e-10 / 1e-18); the float kernel
// rounds the finished value once.  DESIGN.md 3, "Pathwise function draws".
#include "sgp_pathwise.cuh"
#include "../../include/henbun_hip.h"

// D, NST: see PwColumn and pw_value_tiles (csrc/sgp_pathwise.cuh), which hold the synthesis and the K-loop
template <typename T, int D, int NST>
__global__ void __launch_bounds__(PW_THREADS) sgp_pathwise_kernel(PwArgs<T> a) {
  typedef PwMma<T> MM;
  const int n = a.n, S = a.S;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l16 = lane & 15;
  const int s0 = blockIdx.y * PW_SMAX;
  const int col0 = blockIdx.x * PW_CN + 32 * w;
  typename MM::Acc acc[NST][2];
  pw_value_tiles<T, D, NST>(a, s0, acc);

  // masked store: register r of lane l is draw s0 + 16 st + row(l, r), column col0 + 16 ct + l % 16
#pragma unroll
  for (int st = 0; st < NST; ++st)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int s = s0 + 16 * st + MM::row(lane, r), j = col0 + 16 * ct + l16;
        if (s < S && j < n) a.out[(long)s * n + j] = a.scale * acc[st][ct][r];
      }
}

template <typename T, int D>
static void pathwise_launch_d(const PwArgs<T>& a, int nst, dim3 grid, hipStream_t st) {
  if (nst == 1)
    hipLaunchKernelGGL((sgp_pathwise_kernel<T, D, 1>), grid, dim3(PW_THREADS), 0, st, a);
  else if (nst == 2)
    hipLaunchKernelGGL((sgp_pathwise_kernel<T, D, 2>), grid, dim3(PW_THREADS), 0, st, a);
  else if (nst == 3)
    hipLaunchKernelGGL((sgp_pathwise_kernel<T, D, 3>), grid, dim3(PW_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL((sgp_pathwise_kernel<T, D, 4>), grid, dim3(PW_THREADS), 0, st, a);
}

template <typename T>
static int sgp_pathwise(int kind, const T* x, const T* omega, const T* z, const T* ell, long dl, const T* coef, double scale,
                        T* out, long n, long L, long M, long d, long S, hipStream_t st) {
  HB_REQUIRE(kind == HB_KERN_RBF, "hb_sgp_pathwise: the random-feature prior path is that of the UnitRBF kernel only (kind=%d)",
             kind);
  HB_REQUIRE(n >= 0 && L >= 1 && M >= 0 && d >= 1 && S >= 1, "hb_sgp_pathwise: bad extents (n=%ld L=%ld M=%ld d=%ld S=%ld)", n, L, M,
             d, S);
  HB_REQUIRE(dl == 1 || dl == d, "hb_sgp_pathwise: lengthscales must have 1 or d entries");
  HB_REQUIRE(x && omega && ell && coef && out && (z || M == 0), "hb_sgp_pathwise: NULL pointer");
  HB_REQUIRE(n < 2147483647L && L < (1L << 29) && M < (1L << 29) && S * (2 * L + M) < 2147483647L && S * n < 2147483647L &&
                 d < 2147483647L && hb_cdiv(S, PW_SMAX) <= 65535,
             "hb_sgp_pathwise: too large (n, S (2L + M) and S n must be below 2^31)");
  if (n == 0) return 0;
  PwArgs<T> a;
  a.x = x; a.omega = omega; a.z = z; a.ell = ell; a.dl = dl; a.coef = coef; a.scale = (T)scale; a.out = out;
  a.n = (int)n; a.L = (int)L; a.M = (int)M; a.d = (int)d; a.S = (int)S;
  const dim3 grid((unsigned)hb_cdiv(n, PW_CN), (unsigned)hb_cdiv(S, PW_SMAX), 1);
  // every workgroup of the grid carries the same number of row tiles: those of min(S, PW_SMAX) draws
  const int nst = hb_cdiv(S < PW_SMAX ? S : PW_SMAX, 16);
  if (d == 1)
    pathwise_launch_d<T, 1>(a, nst, grid, st);
  else if (d == 2)
    pathwise_launch_d<T, 2>(a, nst, grid, st);
  else if (d == 3)
    pathwise_launch_d<T, 3>(a, nst, grid, st);
  else if (d == 4)
    pathwise_launch_d<T, 4>(a, nst, grid, st);
  else
    pathwise_launch_d<T, 0>(a, nst, grid, st);
  HB_LAUNCH_CHECK();
  return 0;
}

extern "C" int hb_sgp_pathwise_f32(int kind, const float* x, const float* omega, const float* z, const float* ell, long dl,
                                   const float* coef, double scale, float* out, long n, long L, long M, long d, long S,
                                   void* stream) {
  return sgp_pathwise<float>(kind, x, omega, z, ell, dl, coef, scale, out, n, L, M, d, S, (hipStream_t)stream);
}
extern "C" int hb_sgp_pathwise_f64(int kind, const double* x, const double* omega, const double* z, const double* ell, long dl,
                                   const double* coef, double scale, double* out, long n, long L, long M, long d, long S,
                                   void* stream) {
  return sgp_pathwise<double>(kind, x, omega, z, ell, dl, coef, scale, out, n, L, M, d, S, (hipStream_t)stream);
}
