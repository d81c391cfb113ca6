// Gradients of the psi statistics of the unit RBF kernel (csrc/sgp_psi.hip) with respect to the input means and variances,
// the inducing points and the lengthscales: hb_sgp_psi_grad_* (include/henbun_hip.h).  Not in the reference.
//
// For a bound F that depends on the per-point statistics as
//   F = 1/2 sum_n sum_{m, m'} Q_mm' psi2_n(m, m') + sum_n sum_m rho_nm psi1_n(m),   rho_nm = sum_p R_mp Y_np,
// with u_k = l_k^2, a_k = 1 / (u_k + 2 s_k), a1_k = 1 / (u_k + s_k), t_k = mu_k - (z_mk + z_m'k) / 2, dz_k = z_mk - z_m'k,
// tau_k = mu_k - z_mk:
//   dlog psi2 / dmu_k = -2 a_k t_k                 dlog psi1 / dmu_k = -a1_k tau_k
//   dlog psi2 / ds_k  = -a_k + 2 a_k^2 t_k^2       dlog psi1 / ds_k  = -1/2 a1_k + 1/2 a1_k^2 tau_k^2
//   dlog psi2 / dz_mk = a_k t_k - dz_k / (2 u_k)   dlog psi1 / dz_mk = a1_k tau_k
//   dlog psi2 / du_k  = s_k a_k / u_k + dz_k^2 / (4 u_k^2) + a_k^2 t_k^2       dlog psi1 / du_k = 1/2 s_k a1_k / u_k + 1/2 a1_k^2 tau_k^2
// and d / dl_k = 2 l_k d / du_k.  s a / u is formed as -2 g with the g of psi_point_terms, exact at s = 0; no log s anywhere.
// ALL ARITHMETIC IS DOUBLE whatever the storage type T (Q carries |W|^2 ~ 1 / jitter); _f32 and _f64 differ in what they load.
//
// The outputs sum over different axes, so there are two passes, each one exponential per (point, pair of the lower triangle):
//   psi_grad_point_kernel  mubar, sbar.  One THREAD owns one point (a wave of 64 points per workgroup): its terms live in
//                          registers (d <= SGP_DREG) and it walks rows [r_g, r_g+1) of the lower triangle of Q, z and Q read
//                          at wave-uniform addresses (one scalar-cache word for all lanes).  Per pair it adds w = c Q psi2
//                          (c = 1/2 on the diagonal) to S0, w t to S1_k, w t^2 to S2_k; per row the psi1 sums U0, U1_k, U2_k
//                          with rho formed on the fly.  The G row splits (G and r_g functions of M alone, balanced by pair
//                          count) are a second grid dimension; psi_grad_point_fold_kernel adds them in split order.  No
//                          cross-thread sum: a point's bits do not depend on the other points of the call.  d > SGP_DREG: the
//                          terms of the chunk go to the workspace transposed ([term][point], coalesced) and a third grid
//                          dimension takes PSIG_DB dimensions each (the exponentials are formed again per block of dims).
//   psi_grad_pair_kernel   the psi2 part of zbar, ellbar: grid, staging and 4 x 4 register block of psi2_stats_kernel.  A
//                          thread keeps its 16 weights c Q (0 above the diagonal and beyond M), the 16 sums C0 = sum_n w, and
//                          sum_n w a t for its 4 rows and 4 columns (the mirror image of a pair has the same a t and the
//                          opposite dz); the dz terms do not depend on the point and are added from C0 after the loop.  Rows
//                          are summed over the 16 threads that share them through LDS in lane order, columns likewise.
//   psi1_grad_kernel       the psi1 part: 64 inducing points x 4 point lanes, as psi1_stats_kernel.
//   psi_grad_fold_kernel   zbar[m] = its row partials (tiles of its tile row), column partials (tiles of its tile column)
//                          and psi1 partials in split and tile order; the last block ellbar.
// Launch boundaries are the only synchronisation: no atomics, no flags; two calls return the same bits.  The workspace is a
// function of (M, d) alone: N is walked in chunks of at most PSIG_CHUNK points by the point pass and in splits by the other.
#include "sgp_psi.cuh"

#define PSIG_PT 64                    // points per workgroup of the point pass: one per lane of one wave
#define PSIG_GMAX 16                  // row splits of the triangle (at most)
#define PSIG_PAIRS 512                // pairs per row split aimed at
#define PSIG_CHUNK 32768L             // points per launch of the point pass (at most)
#define PSIG_PART_DOUBLES (1L << 22)  // budget of the point pass's partials and terms: fewer points per launch beyond it
#define PSIG_DB 8                     // dimensions per block, loop form of the point pass
#define PSIG_ZB 4                     // dimensions per block, loop form of the pair passes

// ---- point-major pass: mubar, sbar ----------------------------------------------------------------------------------------
__host__ __device__ static inline long psig_groups(long M) {
  const long g = (M * (M + 1) / 2 + PSIG_PAIRS - 1) / PSIG_PAIRS;
  return g > PSIG_GMAX ? PSIG_GMAX : g;
}
// first row of split g: rows [psig_row(g), psig_row(g + 1)) hold about 1 / G of the pairs -- a function of (g, G, M) alone
__device__ __forceinline__ long psig_row(long g, long G, long M) {
  if (g <= 0) return 0;
  if (g >= G) return M;
  long r = (long)((double)M * sqrt((double)g / (double)G));
  return r < 0 ? 0 : (r > M ? M : r);
}

template <typename T>
struct PsiGradPointArgs {
  const T* Xm;       // [nc, d]: the chunk
  const T* Xv;
  const T* Y;        // [nc, P]
  const T* z;        // [M, d]
  const T* ell;
  const double* Q;   // [M, M]
  const double* R;   // [M, P]
  long dl, nc, M, d, P, G;
  long cs;           // chunk stride of part and terms (points, a multiple of 64, >= nc)
  double* part;      // [G][2][d][cs]
  double* terms;     // [4 d + 2][cs] (loop form only)
};

template <typename T, int D>
__global__ void __launch_bounds__(PSIG_PT) psi_grad_point_kernel(PsiGradPointArgs<T> a) {
  const long n = (long)blockIdx.x * PSIG_PT + threadIdx.x;
  const long nn = n < a.nc ? n : a.nc - 1;   // lanes beyond the chunk repeat its last point and write nothing
  const long g = blockIdx.y;
  double pt[4 * D + 2];
  psi_point_terms(a.Xm + nn * D, a.Xv + nn * D, a.ell, a.dl, D, pt);
  const double lp2 = pt[4 * D], lp1 = pt[4 * D + 1];
  double S0 = 0.0, U0 = 0.0, S1[D], S2[D], U1[D], U2[D];
#pragma unroll
  for (int k = 0; k < D; ++k) S1[k] = S2[k] = U1[k] = U2[k] = 0.0;
  const long r0 = psig_row(g, a.G, a.M), r1 = psig_row(g + 1, a.G, a.M);
  const T* y = a.Y + nn * a.P;
  for (long m = r0; m < r1; ++m) {
    double zm[D];
#pragma unroll
    for (int k = 0; k < D; ++k) zm[k] = (double)a.z[m * D + k];
    // psi1 of row m
    double rho = 0.0;
    for (long c = 0; c < a.P; ++c) rho = __builtin_fma(a.R[m * a.P + c], (double)y[c], rho);
    const double w1 = rho * psi1_value(lp1, psi_half<D>(pt, pt + 3 * D, zm, D));
    U0 += w1;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double tau = pt[k] - zm[k], wt = w1 * tau;
      U1[k] += wt;
      U2[k] = __builtin_fma(wt, tau, U2[k]);
    }
    // psi2 of the pairs (m, q), q <= m
    const double hm = psi_half<D>(pt, pt + D, zm, D);
    const double* Qm = a.Q + m * a.M;
    for (long q = 0; q <= m; ++q) {
      double zq[D];
#pragma unroll
      for (int k = 0; k < D; ++k) zq[k] = (double)a.z[q * D + k];
      const double hq = psi_half<D>(pt, pt + D, zq, D);
      const double v = psi2_value<D>(lp2, hm, hq, zm, zq, pt + 2 * D, D);
      const double w = (q == m ? 0.5 * Qm[q] : Qm[q]) * v;
      S0 += w;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const double t = pt[k] - 0.5 * (zm[k] + zq[k]), wt = w * t;
        S1[k] += wt;
        S2[k] = __builtin_fma(wt, t, S2[k]);
      }
    }
  }
  if (n >= a.nc) return;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double ak = pt[D + k], a1 = pt[3 * D + k];
    a.part[((g * 2 + 0) * D + k) * a.cs + n] = -2.0 * ak * S1[k] - a1 * U1[k];
    a.part[((g * 2 + 1) * D + k) * a.cs + n] = (-ak * S0 + 2.0 * ak * ak * S2[k]) + (-0.5 * a1 * U0 + 0.5 * a1 * a1 * U2[k]);
  }
}

// loop form: the terms of the chunk, transposed -- the expressions of psi_point_terms
template <typename T>
__global__ void __launch_bounds__(256) psi_grad_terms_kernel(PsiGradPointArgs<T> a) {
  const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.nc) return;
  const long d = a.d;
  double lp2 = 0.0, lp1 = 0.0;
  for (long k = 0; k < d; ++k) {
    const double l = (double)a.ell[a.dl == 1 ? 0 : k], s = (double)a.Xv[n * d + k];
    const double l2 = l * l, il2 = 1.0 / l2;
    const double ak = 1.0 / __builtin_fma(2.0, s, l2);
    a.terms[k * a.cs + n] = (double)a.Xm[n * d + k];
    a.terms[(d + k) * a.cs + n] = ak;
    a.terms[(2 * d + k) * a.cs + n] = -0.5 * (s * il2) * ak;
    a.terms[(3 * d + k) * a.cs + n] = 1.0 / (l2 + s);
    lp2 += log1p(2.0 * (s * il2));
    lp1 += log1p(s * il2);
  }
  a.terms[4 * d * a.cs + n] = -0.5 * lp2;
  a.terms[(4 * d + 1) * a.cs + n] = -0.5 * lp1;
}

// loop form: any d; blockIdx.z takes dimensions [PSIG_DB z, PSIG_DB (z + 1)) and forms every exponent again
template <typename T>
__global__ void __launch_bounds__(PSIG_PT) psi_grad_point_loop_kernel(PsiGradPointArgs<T> a) {
  const long n = (long)blockIdx.x * PSIG_PT + threadIdx.x;
  const long nn = n < a.nc ? n : a.nc - 1;
  const long g = blockIdx.y, d = a.d, k0 = (long)blockIdx.z * PSIG_DB;
  const double* tm = a.terms + nn;   // term j of this point: tm[j * cs]
  const long cs = a.cs;
  const double lp2 = tm[4 * d * cs], lp1 = tm[(4 * d + 1) * cs];
  long kk[PSIG_DB];   // the block's dimensions, clamped (a dimension beyond d is computed and not written)
  double mu[PSIG_DB];
#pragma unroll
  for (int i = 0; i < PSIG_DB; ++i) {
    kk[i] = k0 + i < d ? k0 + i : d - 1;
    mu[i] = tm[kk[i] * cs];
  }
  double S0 = 0.0, U0 = 0.0, S1[PSIG_DB], S2[PSIG_DB], U1[PSIG_DB], U2[PSIG_DB];
#pragma unroll
  for (int i = 0; i < PSIG_DB; ++i) S1[i] = S2[i] = U1[i] = U2[i] = 0.0;
  const long r0 = psig_row(g, a.G, a.M), r1 = psig_row(g + 1, a.G, a.M);
  const T* y = a.Y + nn * a.P;
  for (long m = r0; m < r1; ++m) {
    const T* zm = a.z + m * d;
    double rho = 0.0;
    for (long c = 0; c < a.P; ++c) rho = __builtin_fma(a.R[m * a.P + c], (double)y[c], rho);
    double q1 = 0.0, q2 = 0.0;
    for (long k = 0; k < d; ++k) {
      const double t = tm[k * cs] - (double)zm[k];
      q1 = __builtin_fma(tm[(3 * d + k) * cs] * t, t, q1);
      q2 = __builtin_fma(tm[(d + k) * cs] * t, t, q2);
    }
    const double w1 = rho * psi1_value(lp1, -0.5 * q1), hm = -0.5 * q2;
    U0 += w1;
#pragma unroll
    for (int i = 0; i < PSIG_DB; ++i) {
      const double tau = mu[i] - (double)zm[kk[i]], wt = w1 * tau;
      U1[i] += wt;
      U2[i] = __builtin_fma(wt, tau, U2[i]);
    }
    const double* Qm = a.Q + m * a.M;
    for (long q = 0; q <= m; ++q) {
      const T* zq = a.z + q * d;
      double qq = 0.0, e = 0.0;
      for (long k = 0; k < d; ++k) {
        const double zqk = (double)zq[k], t = tm[k * cs] - zqk, dz = (double)zm[k] - zqk;
        qq = __builtin_fma(tm[(d + k) * cs] * t, t, qq);
        e = __builtin_fma(dz * dz, tm[(2 * d + k) * cs], e);
      }
      const double v = exp((lp2 + (hm + -0.5 * qq)) + e);
      const double w = (q == m ? 0.5 * Qm[q] : Qm[q]) * v;
      S0 += w;
#pragma unroll
      for (int i = 0; i < PSIG_DB; ++i) {
        const double t = mu[i] - 0.5 * ((double)zm[kk[i]] + (double)zq[kk[i]]), wt = w * t;
        S1[i] += wt;
        S2[i] = __builtin_fma(wt, t, S2[i]);
      }
    }
  }
  if (n >= a.nc) return;
#pragma unroll
  for (int i = 0; i < PSIG_DB; ++i) {
    if (k0 + i >= d) break;
    const long k = k0 + i;
    const double ak = tm[(d + k) * cs], a1 = tm[(3 * d + k) * cs];
    a.part[((g * 2 + 0) * d + k) * cs + n] = -2.0 * ak * S1[i] - a1 * U1[i];
    a.part[((g * 2 + 1) * d + k) * cs + n] = (-ak * S0 + 2.0 * ak * ak * S2[i]) + (-0.5 * a1 * U0 + 0.5 * a1 * a1 * U2[i]);
  }
}

// mubar, sbar of the chunk: the row splits' partials in split order
__global__ void __launch_bounds__(256) psi_grad_point_fold_kernel(const double* __restrict__ part, long nc, long d, long G, long cs,
                                                                  double* __restrict__ mubar, double* __restrict__ sbar) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nc * d) return;
  const long k = i / nc, n = i % nc;   // consecutive threads: consecutive points of one dimension (coalesced reads)
  double sm = 0.0, ss = 0.0;
  for (long g = 0; g < G; ++g) {
    sm += part[((g * 2 + 0) * d + k) * cs + n];
    ss += part[((g * 2 + 1) * d + k) * cs + n];
  }
  mubar[n * d + k] = sm;
  sbar[n * d + k] = ss;
}

// ---- pair-major passes: zbar, ellbar --------------------------------------------------------------------------------------
template <typename T>
struct PsiGradPairArgs {
  PsiArgs<T> s;       // the staging arguments of the statistics pass
  const double* Q;     // [M, M]
  const double* R;     // [M, P]
  double* rowpart;     // [splits][T_][64][d]
  double* colpart;     // [splits][T_][64][d]
  double* epart;       // [splits][T_][d]
  double* z1part;      // [splits][M][d]
  double* e1part;      // [splits][nmb][d]
  int pb1;             // points staged per step of psi1_grad_kernel
};

// D > 0: all D dimensions from registers (DB == D).  D == 0: any d, blockIdx.y takes DB = PSIG_ZB dimensions and z is read
// from global memory for the exponents
template <typename T, int D, int DB>
__global__ void __launch_bounds__(PSI_THREADS) psi_grad_pair_kernel(PsiGradPairArgs<T> ga) {
  extern __shared__ double psm[];
  __shared__ double red[PSI_THREADS];
  __shared__ double red16[16];
  const PsiArgs<T>& a = ga.s;
  const int d = (int)a.d, stride = 4 * d + 2;
  const long sp = (long)blockIdx.x / a.T_, t = (long)blockIdx.x % a.T_;
  const long k0 = D ? 0 : (long)blockIdx.y * DB;
  long ti, tj;
  psi_tile_of(t, &ti, &tj);
  const bool diag = ti == tj;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const long kbeg = sp * a.ks, kend = kbeg + a.ks < a.N ? kbeg + a.ks : a.N;

  int kk[DB];   // the block's dimensions, clamped (a dimension beyond d is computed and not written)
  double iu[DB];
#pragma unroll
  for (int c = 0; c < DB; ++c) {
    kk[c] = k0 + c < d ? (int)(k0 + c) : d - 1;
    const double l = (double)a.ell[a.dl == 1 ? 0 : kk[c]];
    iu[c] = 1.0 / (l * l);
  }
  // the thread's 4 columns stay in registers for the whole kernel, its 4 rows take turns (below); rows and columns beyond
  // M are clamped and get the weight 0
  long gj[4];
  bool vj[4];
  double zc[4][DB], cacc[4][DB], eacc[DB];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    gj[j] = tj * PSI_BT + tx + 16 * j;
    vj[j] = gj[j] < a.M;
    if (!vj[j]) gj[j] = a.M - 1;
#pragma unroll
    for (int c = 0; c < DB; ++c) {
      zc[j][c] = (double)a.z[gj[j] * a.d + kk[c]];
      cacc[j][c] = 0.0;
    }
  }
#pragma unroll
  for (int c = 0; c < DB; ++c) eacc[c] = 0.0;
  const long blk = sp * a.T_ + t;

  // ONE ROW OF THE REGISTER BLOCK PER WALK over the split's points: 4 exponentials in flight and the point-invariant
  // factors of 4 pairs live, not 16 -- with the whole block in one walk the compiler keeps dz^2 and the midpoints of all
  // 16 pairs in registers next to the temporaries of 16 exponentials, and the accumulators go to scratch (DESIGN.md 3,
  // "Bayesian GP-LVM").  The price: the points are staged 4 times and the 4 half exponents of the columns are formed again
  // per row (d fused multiply-adds each, against the exponential).  On a diagonal tile the pairs of a row that lie in
  // register blocks wholly above the diagonal (j > i) are left out at compile time.
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    long gi = ti * PSI_BT + ty + 16 * i;
    const bool vi = gi < a.M;
    if (!vi) gi = a.M - 1;
    double zr[DB], racc[DB], qw[4], C0[4];
#pragma unroll
    for (int c = 0; c < DB; ++c) {
      zr[c] = (double)a.z[gi * a.d + kk[c]];
      racc[c] = 0.0;
    }
    // the weights: Q below the diagonal, Q / 2 on it, 0 above it and beyond M
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double q = ga.Q[gi * a.M + gj[j]];
      qw[j] = (vi && vj[j] && gj[j] <= gi) ? (gj[j] == gi ? 0.5 * q : q) : 0.0;
      C0[j] = 0.0;
    }
    auto points = [&](auto DIAG, int np) {
      for (int p = 0; p < np; ++p) {
        const double* pt = psm + p * stride;
        const double lp2 = pt[4 * d];
        const double hr = D ? psi_half<D>(pt, pt + d, zr, d) : psi_half<0>(pt, pt + d, a.z + gi * a.d, d);
        double csum = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (decltype(DIAG)::value && j > i) continue;
          double v;
          if (D)
            v = psi2_value<D>(lp2, hr, psi_half<D>(pt, pt + d, zc[j], d), zr, zc[j], pt + 2 * d, d);
          else
            v = psi2_value<0>(lp2, hr, psi_half<0>(pt, pt + d, a.z + gj[j] * a.d, d), a.z + gi * a.d, a.z + gj[j] * a.d,
                              pt + 2 * d, d);
          const double w = qw[j] * v;
          C0[j] += w;
          csum += w;
#pragma unroll
          for (int c = 0; c < DB; ++c) {
            const double at = pt[d + kk[c]] * (pt[kk[c]] - 0.5 * (zr[c] + zc[j][c])), wat = w * at;
            racc[c] += wat;
            cacc[j][c] += wat;
            eacc[c] = __builtin_fma(wat, at, eacc[c]);
          }
        }
#pragma unroll
        for (int c = 0; c < DB; ++c) eacc[c] = __builtin_fma(csum, -2.0 * pt[2 * d + kk[c]], eacc[c]);   // s a / u = -2 g
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
    // the terms in dz do not depend on the point: from C0 = sum_n w
#pragma unroll
    for (int c = 0; c < DB; ++c)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double dz = zr[c] - zc[j][c], h = 0.5 * iu[c] * dz * C0[j];
        racc[c] -= h;
        cacc[j][c] += h;
        eacc[c] = __builtin_fma(0.5 * iu[c] * dz, h, eacc[c]);   // dz^2 / (4 u^2) C0
      }
    // the row: the 16 threads tx = 0 .. 15 of one ty, in lane order
#pragma unroll
    for (int c = 0; c < DB; ++c) {
      __syncthreads();
      red[tid] = racc[c];
      __syncthreads();
      if (tx == 0 && k0 + c < d) {
        double s = 0.0;
        for (int x = 0; x < 16; ++x) s += red[ty * 16 + x];
        ga.rowpart[(blk * PSI_BT + ty + 16 * i) * a.d + k0 + c] = s;
      }
    }
  }
  // the columns: the 16 threads ty = 0 .. 15 of one tx, in order; ellbar: the whole workgroup
#pragma unroll
  for (int c = 0; c < DB; ++c) {
    const bool live = k0 + c < d;   // uniform over the workgroup
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      __syncthreads();
      red[tid] = cacc[j][c];
      __syncthreads();
      if (ty == 0 && live) {
        double s = 0.0;
        for (int y = 0; y < 16; ++y) s += red[y * 16 + tx];
        ga.colpart[(blk * PSI_BT + tx + 16 * j) * a.d + k0 + c] = s;
      }
    }
    __syncthreads();
    const double e = block_sum(eacc[c], red16);
    if (tid == 0 && live) ga.epart[blk * a.d + k0 + c] = e;
  }
}

// the terms psi1_grad_kernel stages per point, 3 d + 1 doubles: [mu (d)][a1 (d)][g1 (d)][lp1], g1 = s a1 / (2 l^2)
template <typename T>
__device__ __forceinline__ void psi1_grad_stage(const PsiArgs<T>& a, long n0, int np, double* psm) {
  const int d = (int)a.d;
  __syncthreads();
  if ((int)threadIdx.x < np) {
    const T* xm = a.Xm + (n0 + threadIdx.x) * a.d;
    const T* xv = a.Xv + (n0 + threadIdx.x) * a.d;
    double* out = psm + threadIdx.x * (3 * d + 1);
    double lp1 = 0.0;
    for (int k = 0; k < d; ++k) {
      const double l = (double)a.ell[a.dl == 1 ? 0 : k], s = (double)xv[k];
      const double l2 = l * l, il2 = 1.0 / l2;
      const double a1 = 1.0 / (l2 + s);
      out[k] = (double)xm[k];
      out[d + k] = a1;
      out[2 * d + k] = 0.5 * (s * il2) * a1;
      lp1 += log1p(s * il2);
    }
    out[3 * d] = -0.5 * lp1;
  }
  __syncthreads();
}

template <typename T, int D, int DB>
__global__ void __launch_bounds__(PSI_THREADS) psi1_grad_kernel(PsiGradPairArgs<T> ga) {
  extern __shared__ double psm[];
  __shared__ double red[3][64];
  __shared__ double ered[64];
  const PsiArgs<T>& a = ga.s;
  const int d = (int)a.d, stride = 3 * d + 1;
  const long nmb = (a.M + 63) / 64;
  const long sp = (long)blockIdx.x / nmb, mb = (long)blockIdx.x % nmb;
  const long k0 = D ? 0 : (long)blockIdx.y * DB;
  const int tid = threadIdx.x, ml = tid & 63, nl = tid >> 6;
  const long m = mb * 64 + ml, mc = m < a.M ? m : a.M - 1;
  const long kbeg = sp * a.ks, kend = kbeg + a.ks < a.N ? kbeg + a.ks : a.N;
  int kk[DB];
  double zr[DB];
#pragma unroll
  for (int c = 0; c < DB; ++c) {
    kk[c] = k0 + c < d ? (int)(k0 + c) : d - 1;
    zr[c] = (double)a.z[mc * a.d + kk[c]];
  }
  const double* Rm = ga.R + mc * a.P;
  double zacc[DB], eacc[DB];
#pragma unroll
  for (int c = 0; c < DB; ++c) zacc[c] = eacc[c] = 0.0;
  for (long n0 = kbeg; n0 < kend; n0 += ga.pb1) {
    const int np = (int)(kend - n0 < ga.pb1 ? kend - n0 : ga.pb1);
    psi1_grad_stage(a, n0, np, psm);
    for (int p = nl; p < np; p += 4) {
      const double* pt = psm + p * stride;
      const double h = D ? psi_half<D>(pt, pt + d, zr, d) : psi_half<0>(pt, pt + d, a.z + mc * a.d, d);
      const T* y = a.Y + (n0 + p) * a.P;
      double rho = 0.0;
      for (long c = 0; c < a.P; ++c) rho = __builtin_fma(Rm[c], (double)y[c], rho);
      const double w = rho * psi1_value(pt[3 * d], h);
#pragma unroll
      for (int c = 0; c < DB; ++c) {
        const double at = pt[d + kk[c]] * (pt[kk[c]] - zr[c]), wat = w * at;
        zacc[c] += wat;
        eacc[c] = __builtin_fma(w, pt[2 * d + kk[c]], eacc[c]);
        eacc[c] = __builtin_fma(0.5 * wat, at, eacc[c]);
      }
    }
  }
  // the 4 point lanes in lane order, then (ellbar) the 64 inducing points in order
#pragma unroll
  for (int c = 0; c < DB; ++c) {
    const bool live = k0 + c < d;
    for (int which = 0; which < 2; ++which) {
      const double v = which ? eacc[c] : zacc[c];
      __syncthreads();
      if (nl > 0) red[nl - 1][ml] = v;
      __syncthreads();
      if (nl == 0) {
        const double s = ((v + red[0][ml]) + red[1][ml]) + red[2][ml];
        if (which == 0) {
          if (m < a.M && live) ga.z1part[(sp * a.M + m) * a.d + k0 + c] = s;
        } else {
          ered[ml] = m < a.M ? s : 0.0;
        }
      }
    }
    __syncthreads();
    if (tid == 0 && live) {
      double s = 0.0;
      for (int x = 0; x < 64; ++x) s += ered[x];
      ga.e1part[(sp * nmb + mb) * a.d + k0 + c] = s;
    }
  }
}

// blocks [0, ceil(M d / 256)): one entry of zbar per thread; the last block: ellbar
template <typename T>
__global__ void __launch_bounds__(256) psi_grad_fold_kernel(PsiGradPairArgs<T> ga, long splits, double* __restrict__ zbar,
                                                            double* __restrict__ ellbar) {
  __shared__ double red[16];
  const PsiArgs<T>& a = ga.s;
  const long M = a.M, d = a.d, T_ = a.T_;
  const long nt = (M + PSI_BT - 1) / PSI_BT, nmb = (M + 63) / 64;
  if ((long)blockIdx.x == (long)gridDim.x - 1) {
    double total = 0.0;
    for (long k = 0; k < d; ++k) {
      double s = 0.0;
      for (long i = threadIdx.x; i < splits * T_; i += blockDim.x) s += ga.epart[i * d + k];
      for (long i = threadIdx.x; i < splits * nmb; i += blockDim.x) s += ga.e1part[i * d + k];
      s = block_sum(s, red);
      const double l = (double)a.ell[a.dl == 1 ? 0 : k];
      if (a.dl == 1)
        total += 2.0 * l * s;
      else if (threadIdx.x == 0)
        ellbar[k] = 2.0 * l * s;
    }
    if (a.dl == 1 && threadIdx.x == 0) ellbar[0] = total;
    return;
  }
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= M * d) return;
  const long m = e / d, k = e % d, tb = m / PSI_BT, r = m % PSI_BT;
  double s = 0.0;
  for (long sp = 0; sp < splits; ++sp) {
    for (long tj = 0; tj <= tb; ++tj) s += ga.rowpart[((sp * T_ + tb * (tb + 1) / 2 + tj) * PSI_BT + r) * d + k];
    for (long ti = tb; ti < nt; ++ti) s += ga.colpart[((sp * T_ + ti * (ti + 1) / 2 + tb) * PSI_BT + r) * d + k];
    s += ga.z1part[(sp * M + m) * d + k];
  }
  zbar[e] = s;
}

// ---- host -----------------------------------------------------------------------------------------------------------------
static inline long psig_dim_blocks(long d, long db) { return d <= SGP_DREG ? 1 : (d + db - 1) / db; }
// splits of N of the pair passes: tiles x splits x blocks of dimensions about PSI_TARGET_WG
static inline long psig_max_splits(long M, long d) {
  const long s = PSI_TARGET_WG / (psi_tiles(M) * psig_dim_blocks(d, PSIG_ZB));
  return s > 1 ? s : 1;
}
static inline void psig_split(long N, long M, long d, long* ks, long* splits) {
  const long S = psig_max_splits(M, d);
  long k = (N + S - 1) / S;
  k = (k + PSI_PB - 1) / PSI_PB * PSI_PB;
  *ks = k;
  *splits = (N + k - 1) / k;
}
// points per launch of the point pass: a function of (M, d) alone, a multiple of 64
static inline long psig_chunk(long M, long d) {
  const long per = 2 * d * psig_groups(M) + (d > SGP_DREG ? 4 * d + 2 : 0);
  long c = PSIG_PART_DOUBLES / per / 64 * 64;
  if (c > PSIG_CHUNK) c = PSIG_CHUNK;
  return c < 64 ? 64 : c;
}
static inline int psig_stage1_points(long d) {
  const long pb = PSI_LDS_BYTES / ((3 * d + 1) * 8);
  return (int)(pb > PSI_PB ? PSI_PB : pb);
}
struct PsiGradWs {
  long rowpart, colpart, epart, z1part, e1part, part, terms, total;   // offsets in doubles
};
static inline PsiGradWs psig_ws(long M, long d) {
  const long S = psig_max_splits(M, d), T_ = psi_tiles(M), nmb = (M + 63) / 64, cs = psig_chunk(M, d);
  PsiGradWs w;
  long o = 0;
  w.rowpart = o; o += hb_round64(S * T_ * PSI_BT * d);
  w.colpart = o; o += hb_round64(S * T_ * PSI_BT * d);
  w.epart = o;   o += hb_round64(S * T_ * d);
  w.z1part = o;  o += hb_round64(S * M * d);
  w.e1part = o;  o += hb_round64(S * nmb * d);
  w.part = o;    o += hb_round64(psig_groups(M) * 2 * d * cs);
  w.terms = o;   o += d > SGP_DREG ? hb_round64((4 * d + 2) * cs) : 0;
  w.total = o;
  return w;
}

extern "C" long hb_sgp_psi_grad_ws_elems(long N, long M, long d, long P, int dtype_bytes) {
  (void)P;
  if (N <= 0 || M <= 0 || d <= 0 || d > PSI_DMAX || (dtype_bytes != 4 && dtype_bytes != 8)) return 0;
  return PSI_DOUBLES_AS(dtype_bytes, psig_ws(M, d).total);
}

template <typename T>
static int sgp_psi_grad(int kind, const T* Xmean, const T* Xvar, const T* Y, const T* z, const T* ell, long dl, const double* Q,
                        const double* R, double* mubar, double* sbar, double* zbar, double* ellbar, long N, long M, long d, long P,
                        T* ws, hipStream_t st) {
  const char* who = "hb_sgp_psi_grad";
  HB_REQUIRE(kind == HB_KERN_RBF, "%s: only the UnitRBF kernel has these closed forms (kind=%d)", who, kind);
  HB_REQUIRE(N >= 1 && M >= 1 && d >= 1 && P >= 1 && d <= PSI_DMAX, "%s: bad extents (N=%ld M=%ld d=%ld P=%ld; d <= %d)", who, N,
             M, d, P, PSI_DMAX);
  HB_REQUIRE(dl == 1 || dl == d, "%s: lengthscales must have 1 or d entries", who);
  HB_REQUIRE(Xmean && Xvar && Y && z && ell && Q && R, "%s: NULL input pointer", who);
  HB_REQUIRE(mubar && sbar && zbar && ellbar, "%s: NULL output pointer", who);
  HB_REQUIRE(ws && (uintptr_t)ws % 16 == 0, "%s: needs a 16-byte aligned workspace of %ld elements", who,
             hb_sgp_psi_grad_ws_elems(N, M, d, P, (int)sizeof(T)));
  HB_REQUIRE(M * M < 2147483647L, "%s: matrix too large (M=%ld)", who, M);
  const PsiGradWs w = psig_ws(M, d);
  double* base = (double*)ws;

  // pair-major passes: zbar, ellbar
  PsiGradPairArgs<T> ga;
  PsiArgs<T>& a = ga.s;
  a.Xm = Xmean; a.Xv = Xvar; a.Y = Y; a.z = z; a.ell = ell; a.dl = dl; a.N = N; a.M = M; a.d = d; a.P = P;
  long splits;
  psig_split(N, M, d, &a.ks, &splits);   // splits <= psig_max_splits(M, d): the workspace holds them
  a.T_ = psi_tiles(M);
  a.pb = psi_stage_points(d);
  a.part = nullptr; a.cpart = nullptr;
  ga.Q = Q; ga.R = R;
  ga.rowpart = base + w.rowpart; ga.colpart = base + w.colpart; ga.epart = base + w.epart;
  ga.z1part = base + w.z1part; ga.e1part = base + w.e1part;
  ga.pb1 = psig_stage1_points(d);
  const size_t lds2 = (size_t)a.pb * (4 * d + 2) * 8, lds1 = (size_t)ga.pb1 * (3 * d + 1) * 8;
  const long nmb = (M + 63) / 64;
  const unsigned zb = (unsigned)psig_dim_blocks(d, PSIG_ZB);
#define PSIG_LAUNCH_PAIR(D)                                                                                                       \
  do {                                                                                                                            \
    hipLaunchKernelGGL((psi_grad_pair_kernel<T, D, D ? D : PSIG_ZB>), dim3((unsigned)(a.T_ * splits), zb), dim3(PSI_THREADS), lds2, \
                       st, ga);                                                                                                   \
    hipLaunchKernelGGL((psi1_grad_kernel<T, D, D ? D : PSIG_ZB>), dim3((unsigned)(nmb * splits), zb), dim3(PSI_THREADS), lds1, st,  \
                       ga);                                                                                                       \
  } while (0)
  PSI_DISPATCH_D(d, PSIG_LAUNCH_PAIR);
#undef PSIG_LAUNCH_PAIR
  HB_LAUNCH_CHECK();
  hipLaunchKernelGGL((psi_grad_fold_kernel<T>), dim3((unsigned)((M * d + 255) / 256 + 1)), dim3(256), 0, st, ga, splits, zbar,
                     ellbar);
  HB_LAUNCH_CHECK();

  // point-major pass: mubar, sbar, a chunk of points per launch
  PsiGradPointArgs<T> pa;
  pa.z = z; pa.ell = ell; pa.Q = Q; pa.R = R; pa.dl = dl; pa.M = M; pa.d = d; pa.P = P;
  pa.G = psig_groups(M);
  pa.cs = psig_chunk(M, d);
  pa.part = base + w.part;
  pa.terms = base + w.terms;
  const unsigned db = (unsigned)psig_dim_blocks(d, PSIG_DB);
  for (long c0 = 0; c0 < N; c0 += pa.cs) {
    pa.nc = N - c0 < pa.cs ? N - c0 : pa.cs;
    pa.Xm = Xmean + c0 * d; pa.Xv = Xvar + c0 * d; pa.Y = Y + c0 * P;
    const dim3 grid((unsigned)((pa.nc + PSIG_PT - 1) / PSIG_PT), (unsigned)pa.G, db);
    switch (d <= SGP_DREG ? (int)d : 0) {
      case 1: hipLaunchKernelGGL((psi_grad_point_kernel<T, 1>), grid, dim3(PSIG_PT), 0, st, pa); break;
      case 2: hipLaunchKernelGGL((psi_grad_point_kernel<T, 2>), grid, dim3(PSIG_PT), 0, st, pa); break;
      case 3: hipLaunchKernelGGL((psi_grad_point_kernel<T, 3>), grid, dim3(PSIG_PT), 0, st, pa); break;
      case 4: hipLaunchKernelGGL((psi_grad_point_kernel<T, 4>), grid, dim3(PSIG_PT), 0, st, pa); break;
      default:
        hipLaunchKernelGGL((psi_grad_terms_kernel<T>), dim3((unsigned)((pa.nc + 255) / 256)), dim3(256), 0, st, pa);
        hipLaunchKernelGGL((psi_grad_point_loop_kernel<T>), grid, dim3(PSIG_PT), 0, st, pa);
        break;
    }
    HB_LAUNCH_CHECK();
    hipLaunchKernelGGL(psi_grad_point_fold_kernel, dim3((unsigned)((pa.nc * d + 255) / 256)), dim3(256), 0, st, pa.part, pa.nc, d,
                       pa.G, pa.cs, mubar + c0 * d, sbar + c0 * d);
    HB_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int hb_sgp_psi_grad_f32(int kind, const float* Xmean, const float* Xvar, const float* Y, const float* z,
                                   const float* ell, long dl, const double* Q, const double* R, double* mubar, double* sbar,
                                   double* zbar, double* ellbar, long N, long M, long d, long P, float* ws, void* stream) {
  return sgp_psi_grad<float>(kind, Xmean, Xvar, Y, z, ell, dl, Q, R, mubar, sbar, zbar, ellbar, N, M, d, P, ws,
                             (hipStream_t)stream);
}
extern "C" int hb_sgp_psi_grad_f64(int kind, const double* Xmean, const double* Xvar, const double* Y, const double* z,
                                   const double* ell, long dl, const double* Q, const double* R, double* mubar, double* sbar,
                                   double* zbar, double* ellbar, long N, long M, long d, long P, double* ws, void* stream) {
  return sgp_psi_grad<double>(kind, Xmean, Xvar, Y, z, ell, dl, Q, R, mubar, sbar, zbar, ellbar, N, M, d, P, ws,
                              (hipStream_t)stream);
}
