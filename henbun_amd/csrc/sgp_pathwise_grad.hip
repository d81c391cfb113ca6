// Maximising pathwise function draws (include/henbun_hip.h; not in the reference): the input gradient of every draw
// (hb_sgp_pathwise_grad_*) and the per-draw extremum over a set of candidates (hb_sgp_pathwise_argmax_*).  Both are
// sgp_pathwise_kernel (csrc/sgp_pathwise.hip) with more done to the basis tile it synthesises: the synthesis, the coef
// staging and the K order are the shared code of csrc/sgp_pathwise.cuh, so the values they form are its bits.
//
// GRADIENT.  With p_lj = sum_k omega_lk x_jk / ell_k,
//     d out[s, j] / d x_jk = scale ( sum_l (omega_lk / ell_k) [ -coef[s, 2l] sin p_lj + coef[s, 2l+1] cos p_lj ]
//                                    + sum_m coef[s, 2L+m] K(z_m, x_j) (z_mk - x_jk) / ell_k^2 )
// is the value contraction with another right operand: trig row 2l <- -B[2l+1] omega_lk / ell_k, row 2l+1 <- B[2l]
// omega_lk / ell_k, RBF row <- B (z_mk - x_jk) / ell_k^2.  The operand of dimension k is formed in registers from the
// value tile as the MFMA loop reads it (a lane reads row r and, in a trig step, its partner r ^ 1) and a small LDS table
// of per-row factors (the signed omega_lk / ell_k, or z_mk): no sincos or exp2 beyond those of the value, no second
// tile.  (1 + DG) accumulator sets: fewer draws per workgroup than the value kernel's 64 -- 32 (two row tiles), 16 for
// double at d >= 3, where two row tiles of 1 + d double accumulator sets leave the register file -- and d <= 4 keeps all
// its dimensions in one workgroup; larger d takes the dimensions in groups of 4 on blockIdx.z, the basis synthesised
// again per group (the memory path of PwColumn), the values stored by group 0.
//
// ARG-MAX.  The value kernel's accumulators are not stored: scale acc, rounded to T -- the number hb_sgp_pathwise would
// have written -- is compared within a lane's registers, across the 16 lanes of a row, across the four waves through
// LDS, and the workgroup leaves (key, column) per draw in the workspace; a second launch, a workgroup per draw, folds
// the strips.  key = the value (largest) or its negation (smallest); comparisons are strict, equal keys go to the lower
// column, a NaN is never taken: the result is the first occurrence of the extremum, whatever the order of the fold.
#include "sgp_pathwise.cuh"
#include "../../include/henbun_hip.h"

#define PWG_SMAX 32      // draws per workgroup of the gradient kernel (2 row tiles of 16) ...
// ... but one row tile for double at d >= 3: (1 + d) sets of 2 x 2 double accumulator tiles spill
template <typename T> static inline long pwg_smax(long d) { return sizeof(T) == 8 && d >= 3 ? 16 : PWG_SMAX; }
#define PWG_DG 4         // dimensions per workgroup

template <typename T>
struct PwGradArgs {
  PwArgs<T> v;     // v.out may be NULL
  T* grad;         // [S, n, d]
};

// D: as for sgp_pathwise_kernel; DG = D dimensions (all of them) for D in 1 .. 4, PWG_DG per blockIdx.z for D == 0.
// SECOND COPY of pw_value_tiles (csrc/sgp_pathwise.cuh): the prologue, the store / fill / request order, the two barriers
// and the value MFMAs below repeat it line for line, with the factor table and the derivative operands added.  The
// synthesis (PwColumn), the coef staging (PwCoefTile) and pw_step_rows are the shared definitions; the loop is not, so a
// change to either copy is made in both -- `out` here is promised to be hb_sgp_pathwise's bits.
template <typename T, int D, int NST>
__global__ void __launch_bounds__(PW_THREADS) sgp_pathwise_grad_kernel(PwGradArgs<T> ga) {
  typedef PwMma<T> MM;
  constexpr int SP = 16 * NST, DG = D ? D : PWG_DG;
  __shared__ __attribute__((aligned(16))) T Bs[PW_THREADS / 64][PW_KT][PW_BLD];
  __shared__ __attribute__((aligned(16))) T Cs[SP][PW_CLD];
  __shared__ T Fs[DG][PW_KT];   // per (dimension, row) factor: signed omega_lk / ell_k (trig step), z_mk (RBF step)
  const PwArgs<T>& a = ga.v;
  const int n = a.n, L = a.L, M = a.M, S = a.S, d = D ? D : a.d;
  const int Kc = 2 * L + M;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 31, h = lane >> 5;        // synthesis: column of the wave's tile, row parity
  const int l16 = lane & 15, g = lane >> 4;      // MFMA operands
  const int s0 = blockIdx.y * SP;                // (the host launches NST = its draws per workgroup / 16)
  const int col0 = blockIdx.x * PW_CN + 32 * w;
  const int k0 = D ? 0 : blockIdx.z * PWG_DG;    // first dimension of this workgroup
  PwColumn<T, D> col;
  col.load(a, col0 + c < n ? col0 + c : n - 1);   // columns past n: a copy of the last one (never written out)
  PwCoefTile<T, SP> ct;

  // the two columns this lane holds in the MFMA's B operand: their coordinates and 1 / ell^2 for the RBF factor
  T xm[2][DG], ie2[DG];
#pragma unroll
  for (int k = 0; k < DG; ++k) {
    const bool ok = k0 + k < d;
    const T e = a.ell[a.dl == 1 || !ok ? 0 : k0 + k];
    ie2[k] = ok ? T(1) / (e * e) : T(0);
#pragma unroll
    for (int cc = 0; cc < 2; ++cc) {
      const int j = col0 + 16 * cc + l16;
      xm[cc][k] = ok ? a.x[(long)(j < n ? j : n - 1) * d + k0 + k] : T(0);
    }
  }
  // this thread's entry of the factor table: dimension k0 + fk, row fr
  const int fk = tid / PW_KT, fr = tid % PW_KT;
  const bool fok = fk < DG && k0 + fk < d;
  const T fie = fok ? T(1) / a.ell[a.dl == 1 ? 0 : k0 + fk] : T(0);

  typename MM::Acc acc[NST][2], accd[DG][NST][2];
#pragma unroll
  for (int st = 0; st < NST; ++st)
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[st][cc][r] = T(0);
#pragma unroll
        for (int k = 0; k < DG; ++k) accd[k][st][cc][r] = T(0);
      }

  const int nT = (2 * L + PW_KT - 1) / PW_KT, nR = (M + PW_KT - 1) / PW_KT;
  int kb, kend;
  pw_step_rows(0, nT, L, Kc, kb, kend);
  ct.request(a, s0, kb, kend, tid);
#pragma nounroll
  for (int t = 0; t < nT + nR; ++t) {
    const bool trig = t < nT;
    __syncthreads();   // the MFMAs of the step before have read the tiles and the table
    ct.store(Cs, tid);
    col.fill(a, t, nT, Bs[w], c, h);
    if (fk < DG) {
      T f = T(0);
      if (fok) {
        if (trig) {
          const int l = t * (PW_KT / 2) + fr / 2;
          if (l < L) {
            const T q = a.omega[(long)l * d + k0 + fk] * fie;
            f = (fr & 1) ? q : -q;
          }
        } else {
          const int m = (t - nT) * PW_KT + fr;
          f = a.z[(long)(m < M ? m : M - 1) * d + k0 + fk];   // rows past M: the basis value is 0
        }
      }
      Fs[fk][fr] = f;
    }
    if (t + 1 < nT + nR) {   // the next step's coef tile is in flight during the MFMAs
      pw_step_rows(t + 1, nT, L, Kc, kb, kend);
      ct.request(a, s0, kb, kend, tid);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < PW_KT / 4; ++kk) {
      const int r = 4 * kk + g;
      const T b0 = Bs[w][r][l16], b1 = Bs[w][r][16 + l16];
      T e0[DG], e1[DG];
      if (trig) {
        const T p0 = Bs[w][r ^ 1][l16], p1 = Bs[w][r ^ 1][16 + l16];
#pragma unroll
        for (int k = 0; k < DG; ++k) {
          const T f = Fs[k][r];
          e0[k] = p0 * f, e1[k] = p1 * f;
        }
      } else {
#pragma unroll
        for (int k = 0; k < DG; ++k) {
          const T f = Fs[k][r];
          e0[k] = b0 * ((f - xm[0][k]) * ie2[k]), e1[k] = b1 * ((f - xm[1][k]) * ie2[k]);
        }
      }
#pragma unroll
      for (int st = 0; st < NST; ++st) {
        const T av = Cs[16 * st + l16][4 * kk + g];
        acc[st][0] = MM::mma(av, b0, acc[st][0]);
        acc[st][1] = MM::mma(av, b1, acc[st][1]);
#pragma unroll
        for (int k = 0; k < DG; ++k) {
          accd[k][st][0] = MM::mma(av, e0[k], accd[k][st][0]);
          accd[k][st][1] = MM::mma(av, e1[k], accd[k][st][1]);
        }
      }
    }
  }

  // masked stores: register r of lane l is draw s0 + 16 st + row(l, r), column col0 + 16 cc + l % 16
#pragma unroll
  for (int st = 0; st < NST; ++st)
#pragma unroll
    for (int cc = 0; cc < 2; ++cc)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int s = s0 + 16 * st + MM::row(lane, r), j = col0 + 16 * cc + l16;
        if (s < S && j < n) {
          const long e = (long)s * n + j;
          if (a.out && k0 == 0) a.out[e] = a.scale * acc[st][cc][r];
#pragma unroll
          for (int k = 0; k < DG; ++k)
            if (k0 + k < d) ga.grad[e * d + k0 + k] = a.scale * accd[k][st][cc][r];
        }
      }
}

// ------------------------------------------------------------------------------------------------ arg-max
template <typename T>
struct PwArgmaxArgs {
  PwArgs<T> v;     // v.out unused
  int largest;
  T* ws;           // keys [S, strips], then columns within the strip [S, strips] (-1: no comparable value)
};

template <typename T, int D, int NST>
__global__ void __launch_bounds__(PW_THREADS) sgp_pathwise_argmax_kernel(PwArgmaxArgs<T> aa) {
  typedef PwMma<T> MM;
  constexpr int SP = 16 * NST;
  __shared__ T Rk[PW_THREADS / 64][SP];
  __shared__ int Rj[PW_THREADS / 64][SP];
  const PwArgs<T>& a = aa.v;
  const int n = a.n, S = a.S;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), l16 = lane & 15;
  const int s0 = blockIdx.y * PW_SMAX;
  const int cw = 32 * w;                         // the wave's first column within the strip
  const int col0 = blockIdx.x * PW_CN + cw;
  typename MM::Acc acc[NST][2];
  pw_value_tiles<T, D, NST>(a, s0, acc);

#pragma unroll
  for (int st = 0; st < NST; ++st)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      T bk = -INFINITY;
      int bj = -1;
      // the lane's two columns, the lower first; then the 16 lanes of the row
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        const T v = a.scale * acc[st][cc][r];   // the value hb_sgp_pathwise stores
        const T key = aa.largest ? v : -v;
        const int jl = cw + 16 * cc + l16;
        if (col0 + 16 * cc + l16 < n && key == key && (bj < 0 || key > bk)) bk = key, bj = jl;
      }
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) {
        const T ok = __shfl_xor(bk, m);
        const int oj = __shfl_xor(bj, m);
        if (pw_takes<T>(ok, oj, bk, bj)) bk = ok, bj = oj;
      }
      if (l16 == 0) {
        const int sl = 16 * st + MM::row(lane, r);
        Rk[w][sl] = bk, Rj[w][sl] = bj;
      }
    }
  __syncthreads();
  if (tid < SP && s0 + tid < S) {
    T bk = Rk[0][tid];
    int bj = Rj[0][tid];
#pragma unroll
    for (int ww = 1; ww < PW_THREADS / 64; ++ww)
      if (pw_takes<T>(Rk[ww][tid], Rj[ww][tid], bk, bj)) bk = Rk[ww][tid], bj = Rj[ww][tid];
    const long ns = gridDim.x, e = (long)(s0 + tid) * ns + blockIdx.x;
    aa.ws[e] = bk;
    aa.ws[(long)S * ns + e] = (T)bj;
  }
}

// one workgroup per draw: thread i takes strips i, i + 256, ... in order, then a tree over the threads
template <typename T>
__global__ void __launch_bounds__(PW_THREADS) sgp_pathwise_argmax_fold_kernel(const T* __restrict__ ws, int ns, int S, int largest,
                                                                              T* __restrict__ best, long* __restrict__ idx) {
  __shared__ T Rk[PW_THREADS];
  __shared__ long Rj[PW_THREADS];
  const int s = blockIdx.x, tid = threadIdx.x;
  const T* __restrict__ keys = ws + (long)s * ns;
  const T* __restrict__ cols = ws + (long)S * ns + (long)s * ns;
  T bk = -INFINITY;
  long bj = -1;
  for (int b = tid; b < ns; b += PW_THREADS) {
    const T k = keys[b];
    const int cj = (int)cols[b];
    const long j = cj < 0 ? -1 : (long)b * PW_CN + cj;
    if (pw_takes<T>(k, j, bk, bj)) bk = k, bj = j;
  }
  Rk[tid] = bk, Rj[tid] = bj;
  __syncthreads();
  for (int m = PW_THREADS / 2; m > 0; m >>= 1) {
    if (tid < m && pw_takes<T>(Rk[tid + m], Rj[tid + m], Rk[tid], Rj[tid])) Rk[tid] = Rk[tid + m], Rj[tid] = Rj[tid + m];
    __syncthreads();
  }
  if (tid == 0) {
    best[s] = largest ? Rk[0] : -Rk[0];   // no comparable value: -inf (largest), +inf (smallest), idx -1
    idx[s] = Rj[0];
  }
}

// ------------------------------------------------------------------------------------------------ host
template <typename T, int D>
static void pathwise_grad_launch_d(const PwGradArgs<T>& a, int nst, dim3 grid, hipStream_t st) {
  if constexpr (sizeof(T) == 8 && (D == 0 || D >= 3)) {   // pwg_smax: one row tile
    hipLaunchKernelGGL((sgp_pathwise_grad_kernel<T, D, 1>), grid, dim3(PW_THREADS), 0, st, a);
  } else {
    if (nst == 1)
      hipLaunchKernelGGL((sgp_pathwise_grad_kernel<T, D, 1>), grid, dim3(PW_THREADS), 0, st, a);
    else
      hipLaunchKernelGGL((sgp_pathwise_grad_kernel<T, D, 2>), grid, dim3(PW_THREADS), 0, st, a);
  }
}

template <typename T>
static int sgp_pathwise_grad(int kind, const T* x, const T* omega, const T* z, const T* ell, long dl, const T* coef, double scale,
                             T* out, T* grad, long n, long L, long M, long d, long S, hipStream_t st) {
  const char* who = "hb_sgp_pathwise_grad";
  if (int rc = pathwise_check<T>(who, kind, x, omega, z, ell, dl, coef, grad != nullptr, n, 0, L, M, d, S, pwg_smax<T>(d))) return rc;
  HB_REQUIRE(d < 65536 * (long)PWG_DG && S * n < 2147483647L / d, "%s: too large (S n d must be below 2^31)", who);
  if (n == 0) return 0;
  PwGradArgs<T> a;
  a.v = pathwise_args<T>(x, omega, z, ell, dl, coef, scale, out, n, L, M, d, S);
  a.grad = grad;
  const dim3 grid((unsigned)hb_cdiv(n, PW_CN), (unsigned)hb_cdiv(S, pwg_smax<T>(d)), d <= 4 ? 1u : (unsigned)hb_cdiv(d, PWG_DG));
  // every workgroup of the grid carries the same number of row tiles: those of min(S, pwg_smax) draws
  const int nst = hb_cdiv(S < pwg_smax<T>(d) ? S : pwg_smax<T>(d), 16);
  if (d == 1)
    pathwise_grad_launch_d<T, 1>(a, nst, grid, st);
  else if (d == 2)
    pathwise_grad_launch_d<T, 2>(a, nst, grid, st);
  else if (d == 3)
    pathwise_grad_launch_d<T, 3>(a, nst, grid, st);
  else if (d == 4)
    pathwise_grad_launch_d<T, 4>(a, nst, grid, st);
  else
    pathwise_grad_launch_d<T, 0>(a, nst, grid, st);
  HB_LAUNCH_CHECK();
  return 0;
}

template <typename T, int D>
static void pathwise_argmax_launch_d(const PwArgmaxArgs<T>& a, int nst, dim3 grid, hipStream_t st) {
  if (nst == 1)
    hipLaunchKernelGGL((sgp_pathwise_argmax_kernel<T, D, 1>), grid, dim3(PW_THREADS), 0, st, a);
  else if (nst == 2)
    hipLaunchKernelGGL((sgp_pathwise_argmax_kernel<T, D, 2>), grid, dim3(PW_THREADS), 0, st, a);
  else if (nst == 3)
    hipLaunchKernelGGL((sgp_pathwise_argmax_kernel<T, D, 3>), grid, dim3(PW_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL((sgp_pathwise_argmax_kernel<T, D, 4>), grid, dim3(PW_THREADS), 0, st, a);
}

extern "C" long hb_sgp_pathwise_argmax_ws_elems(long n, long S) {
  if (n < 1 || S < 1) return 0;
  return 2 * S * ((n + PW_CN - 1) / PW_CN);
}

template <typename T>
static int sgp_pathwise_argmax(int kind, const T* x, const T* omega, const T* z, const T* ell, long dl, const T* coef, double scale,
                               int largest, T* best, long* idx, long n, long L, long M, long d, long S, T* ws, hipStream_t st) {
  const char* who = "hb_sgp_pathwise_argmax";
  if (int rc = pathwise_check<T>(who, kind, x, omega, z, ell, dl, coef, best && idx, n, 1, L, M, d, S, PW_SMAX)) return rc;
  HB_REQUIRE(ws || hb_sgp_pathwise_argmax_ws_elems(n, S) == 0, "%s: the workspace is NULL (hb_sgp_pathwise_argmax_ws_elems)", who);
  PwArgmaxArgs<T> a;
  a.v = pathwise_args<T>(x, omega, z, ell, dl, coef, scale, (T*)nullptr, n, L, M, d, S);
  a.largest = largest != 0;
  a.ws = ws;
  const int ns = hb_cdiv(n, PW_CN);
  const dim3 grid((unsigned)ns, (unsigned)hb_cdiv(S, PW_SMAX), 1);
  const int nst = hb_cdiv(S < PW_SMAX ? S : PW_SMAX, 16);
  if (d == 1)
    pathwise_argmax_launch_d<T, 1>(a, nst, grid, st);
  else if (d == 2)
    pathwise_argmax_launch_d<T, 2>(a, nst, grid, st);
  else if (d == 3)
    pathwise_argmax_launch_d<T, 3>(a, nst, grid, st);
  else if (d == 4)
    pathwise_argmax_launch_d<T, 4>(a, nst, grid, st);
  else
    pathwise_argmax_launch_d<T, 0>(a, nst, grid, st);
  HB_LAUNCH_CHECK();
  hipLaunchKernelGGL((sgp_pathwise_argmax_fold_kernel<T>), dim3((unsigned)S), dim3(PW_THREADS), 0, st, (const T*)ws, ns, (int)S,
                     a.largest, best, idx);
  HB_LAUNCH_CHECK();
  return 0;
}

extern "C" int hb_sgp_pathwise_grad_f32(int kind, const float* x, const float* omega, const float* z, const float* ell, long dl,
                                        const float* coef, double scale, float* out, float* grad, long n, long L, long M, long d,
                                        long S, void* stream) {
  return sgp_pathwise_grad<float>(kind, x, omega, z, ell, dl, coef, scale, out, grad, n, L, M, d, S, (hipStream_t)stream);
}
extern "C" int hb_sgp_pathwise_grad_f64(int kind, const double* x, const double* omega, const double* z, const double* ell, long dl,
                                        const double* coef, double scale, double* out, double* grad, long n, long L, long M, long d,
                                        long S, void* stream) {
  return sgp_pathwise_grad<double>(kind, x, omega, z, ell, dl, coef, scale, out, grad, n, L, M, d, S, (hipStream_t)stream);
}
extern "C" int hb_sgp_pathwise_argmax_f32(int kind, const float* x, const float* omega, const float* z, const float* ell, long dl,
                                          const float* coef, double scale, int largest, float* best, long* idx, long n, long L,
                                          long M, long d, long S, float* ws, void* stream) {
  return sgp_pathwise_argmax<float>(kind, x, omega, z, ell, dl, coef, scale, largest, best, idx, n, L, M, d, S, ws,
                                    (hipStream_t)stream);
}
extern "C" int hb_sgp_pathwise_argmax_f64(int kind, const double* x, const double* omega, const double* z, const double* ell, long dl,
                                          const double* coef, double scale, int largest, double* best, long* idx, long n, long L,
                                          long M, long d, long S, double* ws, void* stream) {
  return sgp_pathwise_argmax<double>(kind, x, omega, z, ell, dl, coef, scale, largest, best, idx, n, L, M, d, S, ws,
                                     (hipStream_t)stream);
}
