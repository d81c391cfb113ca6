// Kernel expectations of the unit RBF kernel under Gaussian inputs x ~ N(mu, diag(s)), s_k >= 0 (the psi statistics of
// Titsias & Lawrence 2010): hb_sgp_psi_stats_* and hb_sgp_psi_predict_* (include/henbun_hip.h).  Not in the reference.
//
//   psi1(m)     = E k(x, z_m)             = prod_k (1 + s_k / l_k^2)^-1/2   exp(-1/2 sum_k (mu_k - z_mk)^2 / (l_k^2 + s_k))
//   psi2(m, m') = E k(x, z_m) k(x, z_m')  = prod_k (1 + 2 s_k / l_k^2)^-1/2 exp(e),   with a_k = 1 / (l_k^2 + 2 s_k):
//   e = -1/2 sum_k a_k [(mu_k - z_mk)^2 + (mu_k - z_m'k)^2] - 1/4 sum_k (z_mk - z_m'k)^2 (1 / l_k^2 - a_k)
// Every term of e is <= 0 (no cancellation); 1 / l^2 - a is formed as 2 s a / l^2, exact at s = 0, where psi1 = k(mu, z_m)
// and psi2 = k(mu, z_m) k(mu, z_m').  The prefactors enter as logs (log1p), inside the one exponential.
//
// ALL ARITHMETIC IS DOUBLE whatever the storage type T: Phi = W Psi2 W^T amplifies an error of Psi2 by |W|^2 ~ 1 / jitter
// ("Uncertain inputs"); the _f32 and _f64 entries differ in the type they load.
//
// Psi2 = sum_n psi2_n is NOT a rank update once s differs from point to point: it is one exponential per (point, pair of
// inducing points), N M (M + 1) / 2 of them, on the VALU.
//   psi2_stats_kernel   grid = (64 x 64 lower-triangle tiles of Psi2) x (splits of N); 256 threads in 16 x 16, each with a
//                       4 x 4 register block of pairs (rows ty + 16 i, columns tx + 16 j) and its 8 inducing points in
//                       registers (d <= SGP_DREG; a loop over global z beyond).  The points of a step (at most 64) are
//                       staged in LDS as their terms mu, a, g = -(1 / l^2 - a) / 4, and the log prefactor; every thread
//                       reads the same words (broadcast).  Per point a thread forms its 8 half exponents -1/2 sum a
//                       (mu - z)^2 once and one exponential per pair.  On the diagonal tiles the 6 register blocks that lie
//                       wholly above the diagonal are skipped (the point loop is compiled in two forms, chosen per
//                       workgroup).  Double accumulators; the tile goes to the workspace as a partial.
//   psi1_stats_kernel   C[p, m] = sum_n psi1_n(m) Y_np: N M exponentials, 64 inducing points x 4 point lanes per workgroup,
//                       the same splits of N, partials to the workspace.
//   psi_fold_kernel     Psi2 (lower triangle, and its mirror image from the SAME register: bitwise symmetric) and C take the
//                       sum of the splits' partials in split order; the last block sums yy.  A launch boundary is the only
//                       synchronisation: no atomics, no flags, two calls return the same bits.
// The number of splits is a function of (N, M) alone and the workspace one of (M, P) alone.
//
//   psi_predict_kernel  e1[j] = sum_m beta_m psi1_j(m), e2[j] = sum_{m, m'} Q_mm' psi2_j(m, m'): the pairs of the lower
//                       triangle of Q (off-diagonal terms doubled) of ONE point are spread over G workgroups, G a function
//                       of M alone, so a point's bits do not depend on the other points of the call; thread sums in pair
//                       order, block_sum, partials folded in workgroup order by psi_predict_fold_kernel.
// Both families evaluate psi1 and psi2 through psi_point_terms / psi_half / psi1_value / psi2_value (sgp_psi.cuh).
#include "sgp_psi.cuh"   // constants, value functions, PsiArgs / psi_stage, split rules

template <typename T, int D>
__global__ void __launch_bounds__(PSI_THREADS) psi2_stats_kernel(PsiArgs<T> a) {
  extern __shared__ double psm[];
  const int d = (int)a.d, stride = 4 * d + 2;
  const long sp = (long)blockIdx.x / a.T_, t = (long)blockIdx.x % a.T_;
  long ti, tj;
  psi_tile_of(t, &ti, &tj);
  const bool diag = ti == tj;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const long kbeg = sp * a.ks, kend = kbeg + a.ks < a.N ? kbeg + a.ks : a.N;

  // the thread's 4 + 4 inducing points; rows beyond M are clamped (computed, never read by the fold)
  long gi[4], gj[4];
  double zr[4][D ? D : 1], zc[4][D ? D : 1];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    gi[i] = ti * PSI_BT + ty + 16 * i;
    gj[i] = tj * PSI_BT + tx + 16 * i;
    if (gi[i] >= a.M) gi[i] = a.M - 1;
    if (gj[i] >= a.M) gj[i] = a.M - 1;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      zr[i][k] = (double)a.z[gi[i] * D + k];
      zc[i][k] = (double)a.z[gj[i] * D + k];
    }
  }
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;

  // the staged points of a step against the register block.  DIAG: the 6 register blocks that lie wholly above the diagonal
  // are left out AT COMPILE TIME, so that either form is one straight run of independent exponentials
  auto points = [&](auto DIAG, int np) {
    for (int p = 0; p < np; ++p) {
      const double* pt = psm + p * stride;
      const double lp2 = pt[4 * d];
      double hr[4], hc[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (D) {
          hr[i] = psi_half<D>(pt, pt + d, zr[i], d);
          hc[i] = psi_half<D>(pt, pt + d, zc[i], d);
        } else {
          hr[i] = psi_half<0>(pt, pt + d, a.z + gi[i] * a.d, d);
          hc[i] = psi_half<0>(pt, pt + d, a.z + gj[i] * a.d, d);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (decltype(DIAG)::value && j > i) continue;
          if (D)
            acc[i][j] += psi2_value<D>(lp2, hr[i], hc[j], zr[i], zc[j], pt + 2 * d, d);
          else
            acc[i][j] += psi2_value<0>(lp2, hr[i], hc[j], a.z + gi[i] * a.d, a.z + gj[j] * a.d, pt + 2 * d, d);
        }
    }
  };
  for (long n0 = kbeg; n0 < kend; n0 += a.pb) {
    const int np = (int)(kend - n0 < a.pb ? kend - n0 : a.pb);
    psi_stage(a, n0, np, psm);
    if (diag)
      points(std::true_type(), np);
    else
      points(std::false_type(), np);
  }
  double* out = a.part + (sp * a.T_ + t) * PSI_TILE;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) out[(ty + 16 * i) * PSI_BT + tx + 16 * j] = acc[i][j];
}

// C partials: workgroup = 64 inducing points x 4 point lanes (lane nl takes the staged points nl, nl + 4, ..), the lanes
// added in lane order through LDS
template <typename T, int D>
__global__ void __launch_bounds__(PSI_THREADS) psi1_stats_kernel(PsiArgs<T> a) {
  extern __shared__ double psm[];
  __shared__ double red[3][PSI_PMAX][64];
  const int d = (int)a.d, stride = 4 * d + 2;
  const long nmb = (a.M + 63) / 64;
  const long sp = (long)blockIdx.x / nmb, mb = (long)blockIdx.x % nmb;
  const int tid = threadIdx.x, ml = tid & 63, nl = tid >> 6;
  const long m = mb * 64 + ml, mc = m < a.M ? m : a.M - 1;
  const long kbeg = sp * a.ks, kend = kbeg + a.ks < a.N ? kbeg + a.ks : a.N;
  double zr[D ? D : 1];
#pragma unroll
  for (int k = 0; k < D; ++k) zr[k] = (double)a.z[mc * D + k];

  for (long p0 = 0; p0 < a.P; p0 += PSI_PMAX) {   // P > PSI_PMAX: further passes (psi1 is formed again)
    const int pw = (int)(a.P - p0 < PSI_PMAX ? a.P - p0 : PSI_PMAX);
    double acc[PSI_PMAX] = {0.0, 0.0, 0.0, 0.0};
    for (long n0 = kbeg; n0 < kend; n0 += a.pb) {
      const int np = (int)(kend - n0 < a.pb ? kend - n0 : a.pb);
      psi_stage(a, n0, np, psm);
      for (int p = nl; p < np; p += 4) {
        const double* pt = psm + p * stride;
        const double h = D ? psi_half<D>(pt, pt + 3 * d, zr, d) : psi_half<0>(pt, pt + 3 * d, a.z + mc * a.d, d);
        const double v = psi1_value(pt[4 * d + 1], h);
        const T* y = a.Y + (n0 + p) * a.P + p0;
#pragma unroll
        for (int c = 0; c < PSI_PMAX; ++c)
          if (c < pw) acc[c] = __builtin_fma(v, (double)y[c], acc[c]);
      }
    }
    __syncthreads();   // red of the pass before has been read
    if (nl > 0) {
#pragma unroll
      for (int c = 0; c < PSI_PMAX; ++c) red[nl - 1][c][ml] = acc[c];
    }
    __syncthreads();
    if (nl == 0 && m < a.M) {
#pragma unroll
      for (int c = 0; c < PSI_PMAX; ++c)
        if (c < pw) a.cpart[(sp * a.P + p0 + c) * a.M + m] = ((acc[c] + red[0][c][ml]) + red[1][c][ml]) + red[2][c][ml];
    }
  }
}

// blocks [0, 16 T_): one element of one tile per thread, the sum of the splits in split order, written to (i, j) and (j, i);
// the blocks after them: one entry of C per thread; the last block: yy
template <typename T>
__global__ void __launch_bounds__(256) psi_fold_kernel(const double* __restrict__ part, const double* __restrict__ cpart, long T_,
                                                       long splits, long M, long P, double* __restrict__ Psi2,
                                                       double* __restrict__ C, const T* __restrict__ Y, long N,
                                                       double* __restrict__ yy) {
  __shared__ double red[16];
  const long blk = blockIdx.x;
  if (blk == (long)gridDim.x - 1) {
    for (long p = 0; p < P; ++p) {
      double s = 0.0;
      for (long j = threadIdx.x; j < N; j += blockDim.x) {
        const double y = (double)Y[j * P + p];
        s = __builtin_fma(y, y, s);
      }
      s = block_sum(s, red);
      if (threadIdx.x == 0) yy[p] = s;
    }
  } else if (blk < 16 * T_) {
    const long t = blk / 16, e = (blk % 16) * 256 + threadIdx.x;
    long ti, tj;
    psi_tile_of(t, &ti, &tj);
    const long gi = ti * PSI_BT + e / PSI_BT, gj = tj * PSI_BT + e % PSI_BT;
    if (gi >= M || gj > gi) return;
    double s = 0.0;
    for (long k = 0; k < splits; ++k) s += part[(k * T_ + t) * PSI_TILE + e];
    Psi2[gi * M + gj] = s;
    Psi2[gj * M + gi] = s;
  } else {
    const long q = (blk - 16 * T_) * 256 + threadIdx.x;
    if (q >= P * M) return;
    double s = 0.0;
    for (long k = 0; k < splits; ++k) s += cpart[k * P * M + q];
    C[q] = s;
  }
}

// ---- prediction -----------------------------------------------------------------------------------------------------------
template <typename T, int D>
__global__ void __launch_bounds__(PSI_THREADS) psi_predict_kernel(const T* __restrict__ Xm, const T* __restrict__ Xv,
                                                                  const T* __restrict__ z, const T* __restrict__ ell, long dl,
                                                                  const double* __restrict__ beta, const double* __restrict__ Q,
                                                                  double* __restrict__ part, long M, long dd, long G) {
  extern __shared__ double psm[];
  __shared__ double red[16];
  const int d = (int)dd, tid = threadIdx.x;
  const long j = (long)blockIdx.x / G, g = (long)blockIdx.x % G;
  if (tid == 0) psi_point_terms(Xm + j * dd, Xv + j * dd, ell, dl, d, psm);
  __syncthreads();
  const double* mu = psm;
  const double lp2 = psm[4 * d], lp1 = psm[4 * d + 1];
  const long L = M * (M + 1) / 2, per = (L + G - 1) / G;
  const long pend = (g + 1) * per < L ? (g + 1) * per : L;
  double s2 = 0.0, s1 = 0.0;
  long m = 0, q = 0;
  if (g * per + tid < pend) psi_tile_of(g * per + tid, &m, &q);   // pair p of the lower triangle, row by row: (m, q), q <= m
  for (long p = g * per + tid; p < pend; p += PSI_THREADS, q += PSI_THREADS) {
    while (q > m) q -= ++m;   // the next pair of this thread: PSI_THREADS places on, wrapped over the rows
    const T* zm = z + m * dd;
    const T* zq = z + q * dd;
    const double hm = psi_half<D>(mu, mu + d, zm, d), hq = psi_half<D>(mu, mu + d, zq, d);
    const double v = psi2_value<D>(lp2, hm, hq, zm, zq, mu + 2 * d, d);
    const double w = Q[m * M + q];
    s2 = __builtin_fma(m == q ? w : 2.0 * w, v, s2);
  }
  if (g == 0)
    for (long m = tid; m < M; m += PSI_THREADS)
      s1 = __builtin_fma(beta[m], psi1_value(lp1, psi_half<D>(mu, mu + 3 * d, z + m * dd, d)), s1);
  s2 = block_sum(s2, red);
  s1 = block_sum(s1, red);
  if (tid == 0) {
    part[2 * blockIdx.x] = s1;
    part[2 * blockIdx.x + 1] = s2;
  }
}
__global__ void __launch_bounds__(256) psi_predict_fold_kernel(const double* __restrict__ part, long n, long G,
                                                               double* __restrict__ e1, double* __restrict__ e2) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  double s = 0.0;
  for (long g = 0; g < G; ++g) s += part[2 * (j * G + g) + 1];
  e1[j] = part[2 * j * G];
  e2[j] = s;
}

// ---- host -----------------------------------------------------------------------------------------------------------------
static inline long psi_predict_groups(long M) {
  const long g = (M * (M + 1) / 2 + PSI_PAIRS_WG - 1) / PSI_PAIRS_WG;
  return g > PSI_GMAX ? PSI_GMAX : g;
}

extern "C" long hb_sgp_psi_stats_ws_elems(long N, long M, long d, long P, int dtype_bytes) {
  (void)d;
  if (N <= 0 || M <= 0 || P <= 0 || (dtype_bytes != 4 && dtype_bytes != 8)) return 0;
  const long S = psi_max_splits(M);
  return PSI_DOUBLES_AS(dtype_bytes, hb_round64(S * psi_tiles(M) * PSI_TILE) + hb_round64(S * P * M));
}
extern "C" long hb_sgp_psi_predict_ws_elems(long n, long M, long d, int dtype_bytes) {
  (void)d;
  if (n <= 0 || M <= 0 || (dtype_bytes != 4 && dtype_bytes != 8)) return 0;
  return PSI_DOUBLES_AS(dtype_bytes, hb_round64(2 * (n < PSI_PCHUNK ? n : PSI_PCHUNK) * psi_predict_groups(M)));
}


template <typename T>
static int sgp_psi_stats(int kind, const T* Xmean, const T* Xvar, const T* Y, const T* z, const T* ell, long dl, double* Psi2,
                         double* C, double* yy, long N, long M, long d, long P, T* ws, hipStream_t st) {
  const char* who = "hb_sgp_psi_stats";
  HB_REQUIRE(kind == HB_KERN_RBF, "%s: only the UnitRBF kernel has these closed forms (kind=%d)", who, kind);
  HB_REQUIRE(N >= 1 && M >= 1 && d >= 1 && P >= 1 && d <= PSI_DMAX, "%s: bad extents (N=%ld M=%ld d=%ld P=%ld; d <= %d)", who, N,
             M, d, P, PSI_DMAX);
  HB_REQUIRE(dl == 1 || dl == d, "%s: lengthscales must have 1 or d entries", who);
  HB_REQUIRE(Xmean && Xvar && Y && z && ell, "%s: NULL input pointer", who);
  HB_REQUIRE(Psi2 && C && yy, "%s: NULL output pointer", who);
  HB_REQUIRE(ws && (uintptr_t)ws % 16 == 0, "%s: needs a 16-byte aligned workspace of %ld elements", who,
             hb_sgp_psi_stats_ws_elems(N, M, d, P, (int)sizeof(T)));
  HB_REQUIRE(M * M < 2147483647L, "%s: matrix too large (M=%ld)", who, M);
  PsiArgs<T> a;
  a.Xm = Xmean; a.Xv = Xvar; a.Y = Y; a.z = z; a.ell = ell; a.dl = dl; a.N = N; a.M = M; a.d = d; a.P = P;
  long splits;
  psi_split(N, M, &a.ks, &splits);   // splits <= psi_max_splits(M): the workspace holds them
  a.T_ = psi_tiles(M);
  a.pb = psi_stage_points(d);
  a.part = (double*)ws;
  a.cpart = a.part + hb_round64(psi_max_splits(M) * a.T_ * PSI_TILE);
  const size_t lds = (size_t)a.pb * (4 * d + 2) * 8;
  const long nmb = (M + 63) / 64;
#define PSI_LAUNCH_STATS(D)                                                                                               \
  do {                                                                                                                    \
    hipLaunchKernelGGL((psi2_stats_kernel<T, D>), dim3((unsigned)(a.T_ * splits)), dim3(PSI_THREADS), lds, st, a);         \
    hipLaunchKernelGGL((psi1_stats_kernel<T, D>), dim3((unsigned)(nmb * splits)), dim3(PSI_THREADS), lds, st, a);          \
  } while (0)
  PSI_DISPATCH_D(d, PSI_LAUNCH_STATS);
#undef PSI_LAUNCH_STATS
  HB_LAUNCH_CHECK();
  const long fb = 16 * a.T_ + (P * M + 255) / 256 + 1;
  hipLaunchKernelGGL((psi_fold_kernel<T>), dim3((unsigned)fb), dim3(256), 0, st, a.part, a.cpart, a.T_, splits, M, P, Psi2, C, Y,
                     N, yy);
  HB_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int sgp_psi_predict(int kind, const T* Xmean, const T* Xvar, const T* z, const T* ell, long dl, const double* beta,
                           const double* Q, double* e1, double* e2, long n, long M, long d, T* ws, hipStream_t st) {
  const char* who = "hb_sgp_psi_predict";
  HB_REQUIRE(kind == HB_KERN_RBF, "%s: only the UnitRBF kernel has these closed forms (kind=%d)", who, kind);
  HB_REQUIRE(n >= 0 && M >= 1 && d >= 1 && d <= PSI_DMAX, "%s: bad extents (n=%ld M=%ld d=%ld; d <= %d)", who, n, M, d, PSI_DMAX);
  HB_REQUIRE(dl == 1 || dl == d, "%s: lengthscales must have 1 or d entries", who);
  if (n == 0) return 0;
  HB_REQUIRE(Xmean && Xvar && z && ell && beta && Q, "%s: NULL input pointer", who);
  HB_REQUIRE(e1 && e2, "%s: NULL output pointer", who);
  HB_REQUIRE(ws && (uintptr_t)ws % 16 == 0, "%s: needs a 16-byte aligned workspace of %ld elements", who,
             hb_sgp_psi_predict_ws_elems(n, M, d, (int)sizeof(T)));
  HB_REQUIRE(M * M < 2147483647L, "%s: matrix too large (M=%ld)", who, M);
  const long G = psi_predict_groups(M);
  const size_t lds = (size_t)(4 * d + 2) * 8;
  double* part = (double*)ws;
  for (long c0 = 0; c0 < n; c0 += PSI_PCHUNK) {
    const long nc = n - c0 < PSI_PCHUNK ? n - c0 : PSI_PCHUNK;
#define PSI_LAUNCH_PREDICT(D)                                                                                                   \
  hipLaunchKernelGGL((psi_predict_kernel<T, D>), dim3((unsigned)(nc * G)), dim3(PSI_THREADS), lds, st, Xmean + c0 * d, Xvar + c0 * d, \
                     z, ell, dl, beta, Q, part, M, d, G)
    PSI_DISPATCH_D(d, PSI_LAUNCH_PREDICT);
#undef PSI_LAUNCH_PREDICT
    HB_LAUNCH_CHECK();
    hipLaunchKernelGGL(psi_predict_fold_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, st, part, nc, G, e1 + c0, e2 + c0);
    HB_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int hb_sgp_psi_stats_f32(int kind, const float* Xmean, const float* Xvar, const float* Y, const float* z,
                                    const float* ell, long dl, double* Psi2, double* C, double* yy, long N, long M, long d, long P,
                                    float* ws, void* stream) {
  return sgp_psi_stats<float>(kind, Xmean, Xvar, Y, z, ell, dl, Psi2, C, yy, N, M, d, P, ws, (hipStream_t)stream);
}
extern "C" int hb_sgp_psi_stats_f64(int kind, const double* Xmean, const double* Xvar, const double* Y, const double* z,
                                    const double* ell, long dl, double* Psi2, double* C, double* yy, long N, long M, long d, long P,
                                    double* ws, void* stream) {
  return sgp_psi_stats<double>(kind, Xmean, Xvar, Y, z, ell, dl, Psi2, C, yy, N, M, d, P, ws, (hipStream_t)stream);
}
extern "C" int hb_sgp_psi_predict_f32(int kind, const float* Xmean, const float* Xvar, const float* z, const float* ell, long dl,
                                      const double* beta, const double* Q, double* e1, double* e2, long n, long M, long d,
                                      float* ws, void* stream) {
  return sgp_psi_predict<float>(kind, Xmean, Xvar, z, ell, dl, beta, Q, e1, e2, n, M, d, ws, (hipStream_t)stream);
}
extern "C" int hb_sgp_psi_predict_f64(int kind, const double* Xmean, const double* Xvar, const double* z, const double* ell,
                                      long dl, const double* beta, const double* Q, double* e1, double* e2, long n, long M, long d,
                                      double* ws, void* stream) {
  return sgp_psi_predict<double>(kind, Xmean, Xvar, z, ell, dl, beta, Q, e1, e2, n, M, d, ws, (hipStream_t)stream);
}
