// What the kernels over pathwise function draws share (csrc/sgp_pathwise.hip: values; csrc/sgp_pathwise_grad.hip: input
// gradients and the per-draw extremum; csrc/sgp_pathwise_acq.hip: the acquisition reduced over the draws): the tile
// constants, the double-revolution sincos, the synthesis of a column's basis
// values, the staging of the coef tile and the K-loop of the value contraction.  One definition of each -- but for the
// K-loop, which the gradient kernel repeats with its own operands (see pw_value_tiles) -- so that every kernel forms the
// same basis values and the same k-ordered fma chains: their outputs agree to the bit.  At the end, the host-side checks
// and argument packing the entries have in common.
#ifndef HB_SGP_PATHWISE_CUH
#define HB_SGP_PATHWISE_CUH

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

// The arg-max rule of hb_sgp_pathwise_argmax and hb_sgp_acq (comparisons strict, ties to the lowest column, a NaN or an
// empty slot j < 0 never taken): (k2, j2) takes over from (k1, j1): it holds a value, and the other holds none, a smaller key, or the same at a later column
template <typename T>
__device__ __forceinline__ bool pw_takes(T k2, long j2, T k1, long j1) {
  return j2 >= 0 && (j1 < 0 || k2 > k1 || (k2 == k1 && j2 < j1));
}

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

// The column a lane synthesises.  D: the input dimension when it is at most 4 (the coordinates then live in registers),
// 0: any d, the coordinates re-read from memory at every use.
template <typename T, int D>
struct PwColumn {
  static constexpr int DR = D ? D : 1;
  const T* __restrict__ xj;
  const T* __restrict__ ell;
  long dl;
  int d;
  // x / (2 pi ell) in double for the phases, raw x and exp2-scale / ell for the RBF rows
  double xr[DR];
  T xs[DR], sc[DR];

  __device__ __forceinline__ void load(const PwArgs<T>& a, int j) {   // j < n
    d = D ? D : a.d;
    xj = a.x + (long)j * d;
    ell = a.ell;
    dl = a.dl;
#pragma unroll
    for (int k = 0; k < DR; ++k) {
      if (D) {
        const T e = ell[dl == 1 ? 0 : k];
        xs[k] = xj[k];
        xr[k] = (double)xs[k] * (0.15915494309189533577 / (double)e);
        sc[k] = T(SGP_EXP2_SCALE) / e;
      }
    }
  }
  __device__ __forceinline__ double phase(const T* __restrict__ om) const {   // p / 2 pi of the frequency at om[0 .. d-1]
    double rev = 0.0;
    if (D) {
#pragma unroll
      for (int k = 0; k < DR; ++k) rev = fma((double)om[k], xr[k], rev);
    } else {
      for (int k = 0; k < d; ++k) rev = fma((double)om[k], (double)xj[k] * (0.15915494309189533577 / (double)ell[dl == 1 ? 0 : k]), rev);
    }
    return rev;
  }
  __device__ __forceinline__ T rbf(const T* __restrict__ zm) const {   // K(z_m, x): the difference first, scaled afterwards (sgp_strip.cuh)
    T r2 = T(0);
    if (D) {
#pragma unroll
      for (int k = 0; k < DR; ++k) {
        const T tt = (zm[k] - xs[k]) * sc[k];
        r2 += tt * tt;
      }
    } else {
      for (int k = 0; k < d; ++k) {
        const T tt = (zm[k] - xj[k]) * (T(SGP_EXP2_SCALE) / ell[dl == 1 ? 0 : k]);
        r2 += tt * tt;
      }
    }
    return hb_exp2_neg<T>(r2);
  }
  // K-step t of the basis into column c of the wave's tile Bw [PW_KT][PW_BLD]; h: the row parity this lane fills.
  // t < nT: frequencies 16 t + h + 2 i, one sincos fills rows 2 (h + 2 i) and 2 (h + 2 i) + 1; else the RBF rows
  __device__ __forceinline__ void fill(const PwArgs<T>& a, int t, int nT, T (*__restrict__ Bw)[PW_BLD], int c, int h) const {
    const int L = a.L, M = a.M;
    if (t < nT) {
#pragma unroll
      for (int i = 0; i < PW_KT / 4; ++i) {
        const int f = h + 2 * i, l = t * (PW_KT / 2) + f;
        T sn, cs;
        pw_sincos<T>(phase(a.omega + (long)(l < L ? l : L - 1) * d), sn, cs);
        Bw[2 * f][c] = l < L ? cs : T(0);
        Bw[2 * f + 1][c] = l < L ? sn : T(0);
      }
    } else {
#pragma unroll
      for (int i = 0; i < PW_KT / 2; ++i) {
        const int r = h + 2 * i, m = (t - nT) * PW_KT + r;
        const T v = rbf(a.z + (long)(m < M ? m : M - 1) * d);
        Bw[r][c] = m < M ? v : T(0);
      }
    }
  }
};

// coef tile of a K-step through registers: element e = tid + PW_THREADS i is (draw e / PW_KT, row e % PW_KT); rows past
// the section's end and draws past S are zeros.  SP: draws per workgroup.
template <typename T, int SP>
struct PwCoefTile {
  static constexpr int CIT = SP * PW_KT / PW_THREADS;
  T creg[CIT];
  __device__ __forceinline__ void request(const PwArgs<T>& a, int s0, int kb, int kend, int tid) {   // rows kb .. of coef, valid below kend
    const int Kc = 2 * a.L + a.M;
#pragma unroll
    for (int i = 0; i < CIT; ++i) {
      const int e = tid + PW_THREADS * i, s = s0 + e / PW_KT, k = kb + e % PW_KT;
      const bool ok = s < a.S && k < kend;
      creg[i] = ok ? a.coef[(long)s * Kc + k] : T(0);
    }
  }
  __device__ __forceinline__ void store(T (*__restrict__ Cs)[PW_CLD], int tid) const {
#pragma unroll
    for (int i = 0; i < CIT; ++i) {
      const int e = tid + PW_THREADS * i;
      Cs[e / PW_KT][e % PW_KT] = creg[i];
    }
  }
};

// rows [kb, kend) of K-step t: nT steps over the trig rows (PW_KT / 2 frequencies each), then the RBF rows
__device__ __forceinline__ void pw_step_rows(int t, int nT, int L, int Kc, int& kb, int& kend) {
  if (t < nT)
    kb = t * PW_KT, kend = 2 * L;
  else
    kb = 2 * L + (t - nT) * PW_KT, kend = Kc;
}

// acc[st][ct] = coef[s0 + 16 st .., :] . B(x)[:, col0 + 16 ct ..] for the wave's 32 columns, col0 = 128 blockIdx.x + 32 w:
// register r of lane l is draw s0 + 16 st + row(l, r), column col0 + 16 ct + l % 16.  NST: row tiles of 16 draws.
// SECOND COPY: sgp_pathwise_grad_kernel (csrc/sgp_pathwise_grad.hip) repeats this prologue and K-loop with its derivative
// operands woven into the MFMA loop (its accumulator sets and factor table do not fit a per-step hook without moving
// the loop's registers into a functor).  Its `out` must stay these bits: a change to the lane decomposition, the order of
// store / fill / request, the barriers or the order of the MFMAs here is made there too
// (tests/test_pathwise_grad_gpu.py::test_grad_kernel_against_the_restatement compares the two bit for bit).
template <typename T, int D, int NST>
__device__ __forceinline__ void pw_value_tiles(const PwArgs<T>& a, int s0, typename PwMma<T>::Acc (&acc)[NST][2]) {
  typedef PwMma<T> MM;
  constexpr int SP = 16 * NST;
  __shared__ __attribute__((aligned(16))) T Bs[PW_THREADS / 64][PW_KT][PW_BLD];
  __shared__ __attribute__((aligned(16))) T Cs[SP][PW_CLD];
  const int n = a.n, L = a.L, M = a.M;
  const int Kc = 2 * L + M;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 31, h = lane >> 5;        // synthesis: column of the wave's tile, row parity
  const int l16 = lane & 15, g = lane >> 4;      // MFMA operands
  const int col0 = blockIdx.x * PW_CN + 32 * w;
  PwColumn<T, D> col;
  col.load(a, col0 + c < n ? col0 + c : n - 1);   // columns past n: a copy of the last one (never written out)
  PwCoefTile<T, SP> ct;

#pragma unroll
  for (int st = 0; st < NST; ++st)
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[st][cc][r] = T(0);

  const int nT = (2 * L + PW_KT - 1) / PW_KT, nR = (M + PW_KT - 1) / PW_KT;
  int kb, kend;
  pw_step_rows(0, nT, L, Kc, kb, kend);
  ct.request(a, s0, kb, kend, tid);
#pragma nounroll
  for (int t = 0; t < nT + nR; ++t) {
    __syncthreads();   // the MFMAs of the step before have read both tiles
    ct.store(Cs, tid);
    col.fill(a, t, nT, Bs[w], c, h);
    if (t + 1 < nT + nR) {   // the next step's coef tile is in flight during the MFMAs
      pw_step_rows(t + 1, nT, L, Kc, kb, kend);
      ct.request(a, s0, kb, kend, tid);
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
}

// ------------------------------------------------------------------------------------------------ host
// the checks hb_sgp_pathwise makes, under the caller's name; the entry's own output pointers are checked by the caller
template <typename T>
static int pathwise_check(const char* who, int kind, const T* x, const T* omega, const T* z, const T* ell, long dl, const T* coef,
                          bool outputs, long n, long nmin, long L, long M, long d, long S, long smax) {
  HB_REQUIRE(kind == HB_KERN_RBF, "%s: the random-feature prior path is that of the UnitRBF kernel only (kind=%d)", who, kind);
  HB_REQUIRE(n >= nmin && L >= 1 && M >= 0 && d >= 1 && S >= 1, "%s: bad extents (n=%ld L=%ld M=%ld d=%ld S=%ld)", who, n, L, M, d, S);
  HB_REQUIRE(dl == 1 || dl == d, "%s: lengthscales must have 1 or d entries", who);
  HB_REQUIRE(x && omega && ell && coef && outputs && (z || M == 0), "%s: NULL pointer", who);
  HB_REQUIRE(n < 2147483647L && L < (1L << 29) && M < (1L << 29) && S * (2 * L + M) < 2147483647L && S * n < 2147483647L &&
                 d < 2147483647L && hb_cdiv(S, smax) <= 65535,
             "%s: too large (n, S (2L + M) and S n must be below 2^31)", who);
  return 0;
}

template <typename T>
static PwArgs<T> pathwise_args(const T* x, const T* omega, const T* z, const T* ell, long dl, const T* coef, double scale, T* out,
                               long n, long L, long M, long d, long S) {
  PwArgs<T> a;
  a.x = x; a.omega = omega; a.z = z; a.ell = ell; a.dl = dl; a.coef = coef; a.scale = (T)scale; a.out = out;
  a.n = (int)n; a.L = (int)L; a.M = (int)M; a.d = (int)d; a.S = (int)S;
  return a;
}

#endif  // HB_SGP_PATHWISE_CUH
