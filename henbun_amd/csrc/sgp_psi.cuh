// What csrc/sgp_psi.hip (psi statistics, prediction) and csrc/sgp_psi_grad.hip (their gradients) share: the tile and
// split constants, the value functions psi_point_terms / psi_half / psi1_value / psi2_value, the lower-triangle tile index
// and the host-side split rules.  Not in the reference.
#pragma once
#include <type_traits>
#include "host_calls.cuh"   // hb_round64, HB_REQUIRE
#include "sgp_strip.cuh"    // SGP_DREG

#define PSI_BT 64            // tile of pairs (rows = columns)
#define PSI_PB 64            // points staged per step (at most)
#define PSI_THREADS 256
#define PSI_TILE (PSI_BT * PSI_BT)
#define PSI_TARGET_WG 4096   // tiles x splits aimed at: units a quarter of a round long, so that the last round is short
                             // (1024 measured 62 % of the bare-exp rate at M = 512 where this measures more: DESIGN.md 3)
#define PSI_LDS_BYTES 49152  // staging budget: PSI_PB points while they fit, fewer for large d
#define PSI_DMAX 1535        // one point's terms (4 d + 2 doubles) must fit the staging budget
#define PSI_PMAX 4           // columns of Y one pass of psi1_stats_kernel carries
#define PSI_PAIRS_WG 4096    // pairs per workgroup of psi_predict_kernel (16 per thread)
#define PSI_GMAX 64          // workgroups per point of psi_predict_kernel (at most)
#define PSI_PCHUNK 32768L    // points per launch of psi_predict_kernel (at most)

// ---- the shared value functions -------------------------------------------------------------------------------------------
// The terms of one point, 4 d + 2 doubles: [mu (d)][a (d)][g (d)][a1 (d)][lp2][lp1] with
//   a = 1 / (l^2 + 2 s), g = -(1 / l^2 - a) / 4 = -s a / (2 l^2), lp2 = -1/2 sum log1p(2 s / l^2)      (psi2)
//   a1 = 1 / (l^2 + s), lp1 = -1/2 sum log1p(s / l^2)                                                   (psi1)
template <typename T>
__device__ __forceinline__ void psi_point_terms(const T* __restrict__ xm, const T* __restrict__ xv, const T* __restrict__ ell,
                                                long dl, int d, double* __restrict__ out) {
  double lp2 = 0.0, lp1 = 0.0;
  for (int k = 0; k < d; ++k) {
    const double l = (double)ell[dl == 1 ? 0 : k], s = (double)xv[k];
    const double l2 = l * l, il2 = 1.0 / l2;
    const double a = 1.0 / __builtin_fma(2.0, s, l2);
    out[k] = (double)xm[k];
    out[d + k] = a;
    out[2 * d + k] = -0.5 * (s * il2) * a;
    out[3 * d + k] = 1.0 / (l2 + s);
    lp2 += log1p(2.0 * (s * il2));
    lp1 += log1p(s * il2);
  }
  out[4 * d] = -0.5 * lp2;
  out[4 * d + 1] = -0.5 * lp1;
}
// -1/2 sum_k a_k (mu_k - z_k)^2; D > 0: the dimension at compile time
template <int D, typename Z>
__device__ __forceinline__ double psi_half(const double* __restrict__ mu, const double* __restrict__ a, const Z* __restrict__ z,
                                           int d) {
  double q = 0.0;
  const int n = D ? D : d;
#pragma unroll
  for (int k = 0; k < n; ++k) {
    const double t = mu[k] - (double)z[k];
    q = __builtin_fma(a[k] * t, t, q);
  }
  return -0.5 * q;
}
__device__ __forceinline__ double psi1_value(double lp1, double h) { return exp(lp1 + h); }
// hm, hq: psi_half of the two inducing points with the psi2 terms; symmetric in (m, m') bit for bit
template <int D, typename Z>
__device__ __forceinline__ double psi2_value(double lp2, double hm, double hq, const Z* __restrict__ zm,
                                             const Z* __restrict__ zq, const double* __restrict__ g, int d) {
  double e = lp2 + (hm + hq);
  const int n = D ? D : d;
#pragma unroll
  for (int k = 0; k < n; ++k) {
    const double dz = (double)zm[k] - (double)zq[k];
    e = __builtin_fma(dz * dz, g[k], e);
  }
  return exp(e);   // an exponent below the range underflows to 0
}

__device__ __forceinline__ void psi_tile_of(long t, long* ti, long* tj) {
  long i = (long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (i * (i + 1) / 2 > t) --i;
  while ((i + 1) * (i + 2) / 2 <= t) ++i;
  *ti = i;
  *tj = t - i * (i + 1) / 2;
}

template <typename T>
struct PsiArgs {
  const T* Xm;    // [N, d]
  const T* Xv;    // [N, d]
  const T* Y;     // [N, P]
  const T* z;     // [M, d]
  const T* ell;   // [dl]
  long dl, N, M, d, P;
  long ks;        // points per split (a multiple of PSI_PB)
  long T_;        // lower-triangle tiles
  int pb;         // points staged per step
  double* part;   // [splits][T_][64 x 64]
  double* cpart;  // [splits][P][M]
};

// the terms of points n0 .. n0 + np - 1 -> LDS (one thread per point), between two barriers
template <typename T>
__device__ __forceinline__ void psi_stage(const PsiArgs<T>& a, long n0, int np, double* psm) {
  const int d = (int)a.d;
  __syncthreads();   // the readers of the step before are done
  if ((int)threadIdx.x < np)
    psi_point_terms(a.Xm + (n0 + threadIdx.x) * a.d, a.Xv + (n0 + threadIdx.x) * a.d, a.ell, a.dl, d, psm + threadIdx.x * (4 * d + 2));
  __syncthreads();
}

// ---- host: tiles, splits, staging -----------------------------------------------------------------------------------------
static inline long psi_tiles(long M) {
  const long nt = (M + PSI_BT - 1) / PSI_BT;
  return nt * (nt + 1) / 2;
}
static inline long psi_max_splits(long M) {
  const long s = PSI_TARGET_WG / psi_tiles(M);
  return s > 1 ? s : 1;
}
// splits of N: tiles x splits about PSI_TARGET_WG, a split at least one staging step long -- a function of (N, M) alone
static inline void psi_split(long N, long M, long* ks, long* splits) {
  const long S = psi_max_splits(M);
  long k = (N + S - 1) / S;
  k = (k + PSI_PB - 1) / PSI_PB * PSI_PB;
  *ks = k;
  *splits = (N + k - 1) / k;
}
static inline int psi_stage_points(long d) {
  const long pb = PSI_LDS_BYTES / ((4 * d + 2) * 8);
  return (int)(pb > PSI_PB ? PSI_PB : pb);
}
#define PSI_DOUBLES_AS(dtype_bytes, doubles) ((doubles) * (8 / (dtype_bytes)))

#define PSI_DISPATCH_D(d, CALL) \
  switch ((d) <= SGP_DREG ? (int)(d) : 0) { \
    case 1: CALL(1); break; \
    case 2: CALL(2); break; \
    case 3: CALL(3); break; \
    case 4: CALL(4); break; \
    default: CALL(0); break; \
  }
