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
#include "common.cuh"
#include "mfma16.cuh"
#include "sgp_strip.cuh"
#include "../../include/henbun_hip.h"

#define PW_THREADS 256   // 4 waves, 32 columns each
#define PW_CN 128        // columns per workgroup
#define PW_KT 32         // basis rows per K-step
#define PW_SMAX 64       // draws per workgroup (4 row tiles of 16)
#define PW_BLD 48        // row stride of a wave's basis tile: rows k, k + 1 of an operand read land on disjoint banks
#define PW_CLD (PW_KT + 2)  // row stride of the coef tile: rows s, s + 1 two banks apart (four for double)

// (sin, cos)(2 pi rev) in double.  rev - rint(rev) is exact; t = 4 frac in [-2, 2], q = rint(t) the quadrant,
// r = (t - q) pi / 2 in [-pi/4, pi/4]; NS / NC Taylor terms of sin r / cos r.
template <int NS, int NC>
__device__ __forceinline__ void pw_sincos_rev(double rev, double& s, double& c) {
  constexpr double IF[20] = {1.0, 1.0, 1.0 / 2, 1.0 / 6, 1.0 / 24, 1.0 / 120, 1.0 / 720, 1.0 / 5040, 1.0 / 40320, 1.0 / 362880,
                             1.0 / 3628800, 1.0 / 39916800, 1.0 / 479001600, 1.0 / 6227020800.0, 1.0 / 87178291200.0,
                             1.0 / 1307674368000.0, 1.0 / 20922789888000.0, 1.0 / 355687428096000.0,
                             1.0 / 6402373705728000.0, 1.0 / 121645100408832000.0};
  static_assert(2 * NS - 1 < 20 && 2 * NC - 2 < 20, "table of inverse factorials");
  const double t = 4.0 * (rev - rint(rev)), q = rint(t);
  const double r = (t - q) * 1.57079632679489661923, r2 = r * r;
  double ps = (NS & 1) ? IF[2 * NS - 1] : -IF[2 * NS - 1];
#pragma unroll
  for (int i = NS - 2; i >= 0; --i) ps = fma(ps, r2, (i & 1) ? -IF[2 * i + 1] : IF[2 * i + 1]);
  double pc = (NC & 1) ? IF[2 * NC - 2] : -IF[2 * NC - 2];
#pragma unroll
  for (int i = NC - 2; i >= 0; --i) pc = fma(pc, r2, (i & 1) ? -IF[2 * i] : IF[2 * i]);
  ps *= r;
  const int qi = (int)q & 3;   // 0: (s, c)  1: (c, -s)  2: (-s, -c)  3: (-c, s)
  const double ss = (qi & 1) ? pc : ps, cc = (qi & 1) ? ps : pc;
  s = (qi & 2) ? -ss : ss;
  c = ((qi + 1) & 2) ? -cc : cc;
}
template <typename T> __device__ __forceinline__ void pw_sincos(double rev, T& s, T& c);
template <> __device__ __forceinline__ void pw_sincos<float>(double rev, float& s, float& c) {
  double sd, cd;
  pw_sincos_rev<6, 6>(rev, sd, cd);
  s = (float)sd, c = (float)cd;
}
template <> __device__ __forceinline__ void pw_sincos<double>(double rev, double& s, double& c) { pw_sincos_rev<9, 10>(rev, s, c); }

template <typename T>
struct PwArgs {
  const T* x;      // [n, d]
  const T* omega;  // [L, d]
  const T* z;      // [M, d] (unused for M == 0)
  const T* ell;    // [dl]
  long dl;
  const T* coef;   // [S, 2L + M]
  T scale;
  T* out;          // [S, n]
  int n, L, M, d, S;
};

// D: the input dimension when it is at most 4 (the column's coordinates then live in registers), 0: any d, the
// coordinates re-read from memory at every use.  NST: row tiles of 16 draws per workgroup.
template <typename T, int D, int NST>
__global__ void __launch_bounds__(PW_THREADS) sgp_pathwise_kernel(PwArgs<T> a) {
  typedef PwMma<T> MM;
  constexpr int SP = 16 * NST, DR = D ? D : 1;
  __shared__ __attribute__((aligned(16))) T Bs[PW_THREADS / 64][PW_KT][PW_BLD];
  __shared__ __attribute__((aligned(16))) T Cs[SP][PW_CLD];
  const int n = a.n, L = a.L, M = a.M, S = a.S, d = D ? D : a.d;
  const int Kc = 2 * L + M;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 31, h = lane >> 5;        // synthesis: column of the wave's tile, row parity
  const int l16 = lane & 15, g = lane >> 4;      // MFMA operands
  const int s0 = blockIdx.y * PW_SMAX;
  const int col0 = blockIdx.x * PW_CN + 32 * w;
  const long jc = (long)(col0 + c < n ? col0 + c : n - 1) * d;   // columns past n: a copy of the last one (never written out)
  const T* __restrict__ xj = a.x + jc;

  // the column: x / (2 pi ell) in double for the phases, raw x and exp2-scale / ell for the RBF rows
  double xr[DR];
  T xs[DR], sc[DR];
#pragma unroll
  for (int k = 0; k < DR; ++k) {
    if (D) {
      const T e = a.ell[a.dl == 1 ? 0 : k];
      xs[k] = xj[k];
      xr[k] = (double)xs[k] * (0.15915494309189533577 / (double)e);
      sc[k] = T(SGP_EXP2_SCALE) / e;
    }
  }
  auto phase = [&](const T* __restrict__ om) {   // p / 2 pi of the frequency at om[0 .. d-1]
    double rev = 0.0;
    if (D) {
#pragma unroll
      for (int k = 0; k < DR; ++k) rev = fma((double)om[k], xr[k], rev);
    } else {
      for (int k = 0; k < d; ++k) rev = fma((double)om[k], (double)xj[k] * (0.15915494309189533577 / (double)a.ell[a.dl == 1 ? 0 : k]), rev);
    }
    return rev;
  };
  auto rbf = [&](const T* __restrict__ zm) {     // K(z_m, x): the difference first, scaled afterwards (sgp_strip.cuh)
    T r2 = T(0);
    if (D) {
#pragma unroll
      for (int k = 0; k < DR; ++k) {
        const T tt = (zm[k] - xs[k]) * sc[k];
        r2 += tt * tt;
      }
    } else {
      for (int k = 0; k < d; ++k) {
        const T tt = (zm[k] - xj[k]) * (T(SGP_EXP2_SCALE) / a.ell[a.dl == 1 ? 0 : k]);
        r2 += tt * tt;
      }
    }
    return hb_exp2_neg<T>(r2);
  };

  // coef tile of a K-step through registers: element e = tid + PW_THREADS i is (draw e / PW_KT, row e % PW_KT); rows
  // past the section's end and draws past S are zeros
  constexpr int CIT = SP * PW_KT / PW_THREADS;
  T creg[CIT];
  auto coef_request = [&](int kb, int kend) {    // rows kb .. of coef, valid below kend
#pragma unroll
    for (int i = 0; i < CIT; ++i) {
      const int e = tid + PW_THREADS * i, s = s0 + e / PW_KT, k = kb + e % PW_KT;
      const bool ok = s < S && k < kend;
      creg[i] = ok ? a.coef[(long)s * Kc + k] : T(0);
    }
  };
  auto coef_store = [&]() {
#pragma unroll
    for (int i = 0; i < CIT; ++i) {
      const int e = tid + PW_THREADS * i;
      Cs[e / PW_KT][e % PW_KT] = creg[i];
    }
  };

  typename MM::Acc acc[NST][2];
#pragma unroll
  for (int st = 0; st < NST; ++st)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[st][ct][r] = T(0);

  // K-steps: nT over the trig rows (PW_KT / 2 frequencies each), then nR over the RBF rows
  const int nT = (2 * L + PW_KT - 1) / PW_KT, nR = (M + PW_KT - 1) / PW_KT;
  auto step_rows = [&](int t, int& kb, int& kend) {
    if (t < nT)
      kb = t * PW_KT, kend = 2 * L;
    else
      kb = 2 * L + (t - nT) * PW_KT, kend = Kc;
  };
  int kb, kend;
  step_rows(0, kb, kend);
  coef_request(kb, kend);
#pragma nounroll
  for (int t = 0; t < nT + nR; ++t) {
    __syncthreads();   // the MFMAs of the step before have read both tiles
    coef_store();
    if (t < nT) {
      // frequencies 16 t + h + 2 i: one sincos fills rows 2 (h + 2 i) and 2 (h + 2 i) + 1 of the tile
#pragma unroll
      for (int i = 0; i < PW_KT / 4; ++i) {
        const int f = h + 2 * i, l = t * (PW_KT / 2) + f;
        T sn, cs;
        pw_sincos<T>(phase(a.omega + (long)(l < L ? l : L - 1) * d), sn, cs);
        Bs[w][2 * f][c] = l < L ? cs : T(0);
        Bs[w][2 * f + 1][c] = l < L ? sn : T(0);
      }
    } else {
#pragma unroll
      for (int i = 0; i < PW_KT / 2; ++i) {
        const int r = h + 2 * i, m = (t - nT) * PW_KT + r;
        const T v = rbf(a.z + (long)(m < M ? m : M - 1) * d);
        Bs[w][r][c] = m < M ? v : T(0);
      }
    }
    if (t + 1 < nT + nR) {   // the next step's coef tile is in flight during the MFMAs
      step_rows(t + 1, kb, kend);
      coef_request(kb, kend);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < PW_KT / 4; ++kk) {
      const T b0 = Bs[w][4 * kk + g][l16], b1 = Bs[w][4 * kk + g][16 + l16];
#pragma unroll
      for (int st = 0; st < NST; ++st) {
        const T av = Cs[16 * st + l16][4 * kk + g];
        acc[st][0] = MM::mma(av, b0, acc[st][0]);
        acc[st][1] = MM::mma(av, b1, acc[st][1]);
      }
    }
  }

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
