// Batch acquisition from pathwise function draws (hb_sgp_pathwise_acq_*, include/henbun_hip.h; not in the reference;
// Wilson et al. 2020, section 5): the Monte-Carlo expected improvement / probability of improvement of S coherent
// function draws over per-draw incumbents,
//     value[j] = (1 / S) sum_s u(sigma (v_sj - incumbent[s])),   u = max(., 0) (EI)  or  1[. > 0] (PI),
// v_sj the number hb_sgp_pathwise stores, and the arg-max of value over the columns.  It is sgp_pathwise_kernel
// (csrc/sgp_pathwise.hip) with another epilogue: where that kernel stores its accumulators and sgp_pathwise_argmax_kernel
// (csrc/sgp_pathwise_grad.hip) reduces them over the columns, this one reduces them over the DRAWS.  [S, n] is never
// written.
//
// The grid is the pathwise grid, strips of PW_CN columns x tiles of PW_SMAX draws.  After the K-loop a lane holds, for
// each of its two columns, four draws per row tile: it adds their terms in double (registers in order), then the four
// lane groups (__shfl_xor 16, 32: both operands of each add are swapped between the partners, so every lane ends with
// the same bits), then the row tiles in order.  A wave owns its 32 columns, so the sum of a column never leaves the wave.
//   one tile of draws (S <= PW_SMAX): the workgroup finishes -- divides by S, rounds to T, stores value (if asked for),
//     and leaves ONE (key, column) pair per strip in the workspace for the arg-max;
//   more tiles: the workgroup stores its double partial of each column, ws[tile, j]; sgp_pathwise_acq_sum_kernel adds the
//     tiles of a column in tile order and finishes in the same way.
// sgp_pathwise_acq_fold_kernel then folds the strips' pairs.  The order of every sum is fixed by S alone and a column
// never meets another one before the arg-max: value[j] depends neither on the other columns nor on n.  The arg-max
// compares the ROUNDED values with pw_takes (strict, ties to the lowest column, a NaN never taken), so it is the first
// occurrence of the maximum of `value` whatever the order of the fold.  No atomics.
#include "sgp_pathwise.cuh"
#include "../../include/henbun_hip.h"

template <typename T>
struct PwAcqArgs {
  PwArgs<T> v;          // v.out unused
  const T* incumbent;   // [S]
  int acq, largest;
  int argmax;           // leave the strips' (key, column) pairs in `part`
  T* value;             // [n] or NULL
  double* tiles;        // [tiles of draws, n] partial sums (more than one tile of draws only)
  double* part;         // keys [strips], then columns [strips] (-1: no comparable value)
};

// the term of draw s at a column whose stored value is v: sigma (v - b) in double, then the acquisition's u.  A NaN stays one.
template <typename T>
__device__ __forceinline__ double pwacq_term(T v, T b, int acq, int largest) {
#pragma clang fp contract(off)   // v is a rounded product: the difference is taken of it, not fused into it
  const double t = largest ? (double)v - (double)b : (double)b - (double)v;
  if (t != t) return t;
  if (acq == HB_PWACQ_PI) return t > 0.0 ? 1.0 : 0.0;
  return t > 0.0 ? t : 0.0;
}

// (key, column) of a strip: slot c of Rk / Rj holds the rounded value of the strip's column c and its index in x (-1: past
// n, or a NaN); a tree over the PW_CN slots leaves the pair in the workspace
template <typename T>
__device__ __forceinline__ void pwacq_strip_best(int tid, T* __restrict__ Rk, long* __restrict__ Rj, double* __restrict__ part,
                                                 long strips) {
  __syncthreads();
  for (int m = PW_CN / 2; m > 0; m >>= 1) {
    if (tid < m && pw_takes<T>(Rk[tid + m], Rj[tid + m], Rk[tid], Rj[tid])) Rk[tid] = Rk[tid + m], Rj[tid] = Rj[tid + m];
    __syncthreads();
  }
  if (tid == 0) {
    part[blockIdx.x] = (double)Rk[0];
    part[strips + blockIdx.x] = (double)Rj[0];   // below 2^31: exact
  }
}

template <typename T, int D, int NST>
__global__ void __launch_bounds__(PW_THREADS) sgp_pathwise_acq_kernel(PwAcqArgs<T> aa) {
  typedef PwMma<T> MM;
  __shared__ T Rk[PW_CN];
  __shared__ long Rj[PW_CN];
  const PwArgs<T>& a = aa.v;
  const int n = a.n, S = a.S;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), l16 = lane & 15;
  const int s0 = blockIdx.y * PW_SMAX;
  const int col0 = blockIdx.x * PW_CN + 32 * w;
  typename MM::Acc acc[NST][2];
  pw_value_tiles<T, D, NST>(a, s0, acc);

  double p[2] = {0.0, 0.0};
  {
#pragma clang fp contract(off)   // scale * acc is rounded to T before the incumbent is taken off: hb_sgp_pathwise's bits
#pragma unroll
    for (int st = 0; st < NST; ++st) {
      T b[4];
      bool ok[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int s = s0 + 16 * st + MM::row(lane, r);
        ok[r] = s < S;
        b[r] = aa.incumbent[ok[r] ? s : S - 1];
      }
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        double q = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const T v = a.scale * acc[st][cc][r];   // the value hb_sgp_pathwise stores
          const double u = pwacq_term<T>(v, b[r], aa.acq, aa.largest);
          q += ok[r] ? u : 0.0;
        }
        q += __shfl_xor(q, 16);
        q += __shfl_xor(q, 32);
        p[cc] += q;
      }
    }
  }

  // every lane group holds the same sums: group cc of the first two writes column col0 + 16 cc + l16
  const int g = lane >> 4;
  const int j = col0 + 16 * (g & 1) + l16;
  const double mine = (g & 1) ? p[1] : p[0];
  if (gridDim.y > 1) {
    if (g < 2 && j < n) aa.tiles[(long)blockIdx.y * n + j] = mine;
    return;
  }
  const T val = (T)(mine / (double)S);
  if (g < 2 && j < n && aa.value) aa.value[j] = val;
  if (aa.argmax) {
    if (g < 2) {   // slot: the column within the strip
      const int c = 32 * w + 16 * g + l16;
      Rk[c] = val, Rj[c] = (j < n && val == val) ? (long)j : -1;
    }
    pwacq_strip_best<T>(tid, Rk, Rj, aa.part, gridDim.x);
  }
}

// more than one tile of draws: a workgroup per strip, a thread per column -- the tiles' partials in tile order, then the finish
template <typename T>
__global__ void __launch_bounds__(PW_CN) sgp_pathwise_acq_sum_kernel(const double* __restrict__ tiles, int ntile, int n, int S, int argmax,
                                                                     T* __restrict__ value, double* __restrict__ part) {
  __shared__ T Rk[PW_CN];
  __shared__ long Rj[PW_CN];
  const int tid = threadIdx.x;
  const long j = (long)blockIdx.x * PW_CN + tid;
  T k = T(0);
  long jj = -1;
  if (j < n) {
    double sum = tiles[j];
    for (int t = 1; t < ntile; ++t) sum += tiles[(long)t * n + j];
    k = (T)(sum / (double)S);
    if (value) value[j] = k;
    if (k == k) jj = j;
  }
  if (argmax) {
    Rk[tid] = k, Rj[tid] = jj;
    pwacq_strip_best<T>(tid, Rk, Rj, part, gridDim.x);
  }
}

// one workgroup: thread i takes strips i, i + 256, ... in order, then a tree over the threads (the fixed order of
// sgp_pathwise_argmax_fold_kernel)
template <typename T>
__global__ void __launch_bounds__(PW_THREADS) sgp_pathwise_acq_fold_kernel(const double* __restrict__ part, int ns, T* __restrict__ best,
                                                                           long* __restrict__ idx) {
  __shared__ T Rk[PW_THREADS];
  __shared__ long Rj[PW_THREADS];
  const int tid = threadIdx.x;
  T bk = -INFINITY;
  long bj = -1;
  for (int b = tid; b < ns; b += PW_THREADS) {
    const T k = (T)part[b];
    const long j = (long)part[ns + b];
    if (pw_takes<T>(k, j, bk, bj)) bk = k, bj = j;
  }
  Rk[tid] = bk, Rj[tid] = bj;
  __syncthreads();
  for (int m = PW_THREADS / 2; m > 0; m >>= 1) {
    if (tid < m && pw_takes<T>(Rk[tid + m], Rj[tid + m], Rk[tid], Rj[tid])) Rk[tid] = Rk[tid + m], Rj[tid] = Rj[tid + m];
    __syncthreads();
  }
  if (tid == 0) {
    best[0] = Rj[0] < 0 ? (T)-INFINITY : Rk[0];   // no comparable value: idx -1, best -inf
    idx[0] = Rj[0];
  }
}

// ------------------------------------------------------------------------------------------------ host
template <typename T, int D>
static void pathwise_acq_launch_d(const PwAcqArgs<T>& a, int nst, dim3 grid, hipStream_t st) {
  if (nst == 1)
    hipLaunchKernelGGL((sgp_pathwise_acq_kernel<T, D, 1>), grid, dim3(PW_THREADS), 0, st, a);
  else if (nst == 2)
    hipLaunchKernelGGL((sgp_pathwise_acq_kernel<T, D, 2>), grid, dim3(PW_THREADS), 0, st, a);
  else if (nst == 3)
    hipLaunchKernelGGL((sgp_pathwise_acq_kernel<T, D, 3>), grid, dim3(PW_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL((sgp_pathwise_acq_kernel<T, D, 4>), grid, dim3(PW_THREADS), 0, st, a);
}

// doubles: [tiles of draws, n] partial sums when the draws take more than one tile, then (key, column) per strip
extern "C" long hb_sgp_pathwise_acq_ws_elems(long n, long S) {
  if (n < 1 || S < 1) return 0;
  const long ntile = (S + PW_SMAX - 1) / PW_SMAX;
  return (ntile > 1 ? ntile * n : 0) + 2 * ((n + PW_CN - 1) / PW_CN);
}

template <typename T>
static int sgp_pathwise_acq(int kind, const T* x, const T* omega, const T* z, const T* ell, long dl, const T* coef, double scale, int acq,
                            int largest, const T* incumbent, T* value, T* best, long* idx, long n, long L, long M, long d, long S,
                            double* ws, hipStream_t st) {
  const char* who = "hb_sgp_pathwise_acq";
  const bool argmax = best && idx;
  if (int rc = pathwise_check<T>(who, kind, x, omega, z, ell, dl, coef, incumbent && (value || argmax), n, 1, L, M, d, S, PW_SMAX))
    return rc;
  HB_REQUIRE(acq == HB_PWACQ_EI || acq == HB_PWACQ_PI, "%s: unknown acquisition %d (HB_PWACQ_EI, HB_PWACQ_PI)", who, acq);
  HB_REQUIRE((best != nullptr) == (idx != nullptr), "%s: best and idx are given together or not at all", who);
  HB_REQUIRE(ws || hb_sgp_pathwise_acq_ws_elems(n, S) == 0, "%s: the workspace is NULL (hb_sgp_pathwise_acq_ws_elems)", who);
  const int ns = hb_cdiv(n, PW_CN), ntile = hb_cdiv(S, PW_SMAX);
  PwAcqArgs<T> a;
  a.v = pathwise_args<T>(x, omega, z, ell, dl, coef, scale, (T*)nullptr, n, L, M, d, S);
  a.incumbent = incumbent;
  a.acq = acq;
  a.largest = largest != 0;
  a.argmax = argmax;
  a.value = value;
  a.tiles = ws;
  a.part = ws + (ntile > 1 ? (long)ntile * n : 0);
  const dim3 grid((unsigned)ns, (unsigned)ntile, 1);
  const int nst = hb_cdiv(S < PW_SMAX ? S : PW_SMAX, 16);
  if (d == 1)
    pathwise_acq_launch_d<T, 1>(a, nst, grid, st);
  else if (d == 2)
    pathwise_acq_launch_d<T, 2>(a, nst, grid, st);
  else if (d == 3)
    pathwise_acq_launch_d<T, 3>(a, nst, grid, st);
  else if (d == 4)
    pathwise_acq_launch_d<T, 4>(a, nst, grid, st);
  else
    pathwise_acq_launch_d<T, 0>(a, nst, grid, st);
  HB_LAUNCH_CHECK();
  if (ntile > 1) {
    hipLaunchKernelGGL((sgp_pathwise_acq_sum_kernel<T>), dim3((unsigned)ns), dim3(PW_CN), 0, st, (const double*)a.tiles, ntile, (int)n,
                       (int)S, a.argmax, value, a.part);
    HB_LAUNCH_CHECK();
  }
  if (argmax) {
    hipLaunchKernelGGL((sgp_pathwise_acq_fold_kernel<T>), dim3(1), dim3(PW_THREADS), 0, st, (const double*)a.part, ns, best, idx);
    HB_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int hb_sgp_pathwise_acq_f32(int kind, const float* x, const float* omega, const float* z, const float* ell, long dl,
                                       const float* coef, double scale, int acq, int largest, const float* incumbent, float* value,
                                       float* best, long* idx, long n, long L, long M, long d, long S, double* ws, void* stream) {
  return sgp_pathwise_acq<float>(kind, x, omega, z, ell, dl, coef, scale, acq, largest, incumbent, value, best, idx, n, L, M, d, S, ws,
                                 (hipStream_t)stream);
}
extern "C" int hb_sgp_pathwise_acq_f64(int kind, const double* x, const double* omega, const double* z, const double* ell, long dl,
                                       const double* coef, double scale, int acq, int largest, const double* incumbent, double* value,
                                       double* best, long* idx, long n, long L, long M, long d, long S, double* ws, void* stream) {
  return sgp_pathwise_acq<double>(kind, x, omega, z, ell, dl, coef, scale, acq, largest, incumbent, value, best, idx, n, L, M, d, S, ws,
                                  (hipStream_t)stream);
}
