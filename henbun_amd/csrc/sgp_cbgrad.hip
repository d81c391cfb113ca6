// Streamed part of the gradient of the collapsed bound (hb_sgp_kgrad_*, include/henbun_hip.h).
//
// With K = K(z, X) [M, N] (UnitRBF) and the weights Q [M, M], R [M, P] the M^3 tail hands over:
//     Kbar = Q K + R Y^T,   E = Kbar o K,
//     zbar_id  = -sum_j E_ij (z_id - x_jd) / ell_d^2,     ellbar_d = sum_ij E_ij (z_id - x_jd)^2 / ell_d^3
// (a scalar lengthscale takes the sum over d).  The z gradient of the bound is the difference of this term and the one
// through K(z, z), each about 1000 times larger than their difference, and Q carries W = Lm^-1 twice (entries of order
// 1 / jitter): ALL arithmetic here is double whatever the storage type of X and Y ("Gradient of the
// collapsed bound"; float anywhere in the chain returns noise).  The _f32 / _f64 suffix is the storage type of X and Y
// only; they are converted as they are loaded.
//
// Fast form (M % 16 == 0, M <= 512, d <= 4, P <= 4): column strips.  The N columns are cut into steps of KG_NB = 32; at
// most KG_MAXG workgroups each take a contiguous run of steps, so the workspace does not depend on N.  A workgroup (8
// waves) owns ALL M rows of its step:
//   1. it synthesises K[:, step] in double into LDS with the library's one kernel value (gram_value.cuh), stored in the
//      operand order of v_mfma_f64_16x16x4_f64: fragment (k-step s, column tile jt) holds, for lane l, K[4 s + l / 16]
//      [16 jt + l % 16].  A wave's operand read is 512 contiguous bytes (no bank conflicts), and the SAME fragment
//      (s = 4 it + r) is, lane for lane, the K[i][j] of accumulator register r of row tile `it` -- the epilogue needs no
//      second layout.  M x 32 doubles = 128 KB at M = 512 of the 160 KB a CU has: one workgroup per CU.
//   2. wave w takes row tiles it = w, w + 8, ..: Q K on MFMA (Q repacked once per call into the same fragment order, a
//      coalesced 512-byte load per k-step feeding two MFMAs), then in registers: + R Y^T, times K, times the distances,
//      the 16 column lanes of a row folded with shuffles into the strip's zbar [M, d] in LDS (a row's slots belong to one
//      lane of one wave), ellbar per lane in registers.  Kbar is never written.
//   3. after the last step the strip's partial zbar [M, d] and ellbar [d] go to the workspace.
// A second launch (sgp_kgrad_fold_kernel) adds the strips' partials in strip order and applies -1 / ell^2 and 1 / ell^3.
// A launch boundary is the only synchronisation (no atomics, no flags): two runs return the same bits.
// Every other shape: sgp_kgrad_plain_kernel, plain double loops, one column at a time per workgroup (parity, not speed).
//
// Column-weighted form (hb_sgp_wkgrad_*, the template flag WT of both kernels): Kbar_ij = w_j (Q K)_ij + R_i r_j with
// per-point weights w, r [N] in double and P = 1 -- the gradient of the ELBO of a non-Gaussian likelihood through
// K(z, X) at a fixed q(u) ("Hyper-parameter gradient at fixed q(u)").  r takes the place of Y[:, 0] in ys,
// w is staged next to it and multiplies the accumulator before + R r; everything else is the code above, so w == 1,
// r = Y[:, 0] returns the bits of hb_sgp_kgrad_* at P = 1 (x * 1.0 is exact).  Columns beyond N hold K = 0 as before.
//
// Input gradient (hb_sgp_kgrad_x_*, hb_sgp_wkgrad_x_*, the template flag XG of both kernels): the products e (z - x) whose
// ROW sums are zbar have the input gradient as their COLUMN sums,
//     xbar_jd = + sum_i E_ij (z_id - x_jd) / ell_d^2          [N, d], double
// (every dependence of the bound on X goes through K(z, X): Kdiag == 1).  Strip form: a lane keeps one accumulator per
// (column tile, dimension) over its rows of a step; at the end of the step the four lane groups l / 16 are folded with two
// shuffles (xor 16, then 32), the 8 waves through an LDS array [KG_NW][KG_NB][D] in wave order (a wave without a row tile
// adds zeros), and thread (c, dd) writes the column.  A column belongs to one step of one workgroup and its sum runs over
// the rows in an order that depends on M alone: no atomics, no workspace, no fold launch, and the bits of a column do
// not depend on N or on the other columns of the call.  Plain form: the column's e_i go to LDS, every dimension is summed
// per thread over its strided rows, per wave by shuffles and over the 4 waves in wave order.  XG = false is the code
// without any of it (if constexpr): zbar and ellbar of the two entries are the same bits.
#include "host_calls.cuh"   // hb_round64, HB_REQUIRE_RBF_MODEL
#include "gram_value.cuh"

#define KG_NB 32         // columns per step (two MFMA column tiles)
#define KG_THREADS 512   // 8 waves
#define KG_NW 8
#define KG_MMAX 512
#define KG_DMAX 4
#define KG_PMAX 4
#define KG_MAXG 256      // strips (workgroups) at most: one per CU
#define KG_PLAIN_T 256

template <bool XG>
struct KgXbar {};
template <>
struct KgXbar<true> {
  double* xbar;        // [N, d] (the _x entries only: the other instantiations keep their argument block)
};

template <typename T, bool XG>
struct KgArgs : KgXbar<XG> {
  const T* X;          // [N, d]
  const T* Y;          // [N, P] (unweighted form)
  const double* w;     // [N], [N]: the column weights and r of the weighted form (P = 1), else unused
  const double* r;
  const double* z;     // [M, d]
  const double* ell;   // [dl]
  const double* Q;     // fast: fragment order; plain: row-major [M, M]
  const double* R;     // [M, P]
  double* part;        // [G][stride]
  long dl, N, M, d, P;
  long steps, per;     // column steps in all / per workgroup
  long stride;
};

// Qf[(it * M / 4 + s) * 64 + l] = Q[16 it + l % 16][4 s + l / 16]: the A operand of MFMA (it, s), lane l
__global__ void __launch_bounds__(256) sgp_kgrad_pack_kernel(const double* __restrict__ Q, double* __restrict__ Qf, long M) {
  const long total = M * M, stride = (long)gridDim.x * blockDim.x, nks = M / 4;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const long f = e >> 6, l = e & 63;
    const long it = f / nks, s = f % nks;
    Qf[e] = Q[(16 * it + (l & 15)) * M + 4 * s + (l >> 4)];
  }
}

// doubles of LDS the strip kernel takes: K, xs, ys, (weighted: wv), red, zs, (input gradient: the waves' column sums)
static constexpr size_t kg_strip_lds_elems(long M, int D, bool weighted, bool xg) {
  return (size_t)(M * KG_NB + KG_NB * D + KG_NB * KG_PMAX + (weighted ? KG_NB : 0) + KG_NW * D + M * D +
                  (xg ? KG_NW * KG_NB * D : 0));
}
static_assert(kg_strip_lds_elems(KG_MMAX, KG_DMAX, true, true) * sizeof(double) <= 160 * 1024,
              "the largest strip form must fit the 160 KB of LDS a CU has");

template <typename T, int D, bool WT, bool XG>
__global__ void __launch_bounds__(KG_THREADS) sgp_kgrad_strip_kernel(KgArgs<T, XG> a) {
  typedef Mma<double> MM;
  extern __shared__ __attribute__((aligned(16))) double kg_smem[];
  const long M = a.M, N = a.N, P = a.P, nrt = M / 16, nks = M / 4;
  double* Ks = kg_smem;                // [M / 4][2][64] fragments
  double* xs = Ks + M * KG_NB;         // [KG_NB][D]
  double* ys = xs + KG_NB * D;         // [KG_NB][KG_PMAX]
  double* wv = ys + KG_NB * KG_PMAX;   // [KG_NB] (weighted form only)
  double* red = wv + (WT ? KG_NB : 0); // [KG_NW][D]
  double* zs = red + KG_NW * D;        // [M][D]: zbar of the strip, every row's slots owned by one lane
  // (input gradient only: xr = zs + M * D, [KG_NW][KG_NB][D], the waves' column sums of a step)
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);

  double eacc[D];
#pragma unroll
  for (int dd = 0; dd < D; ++dd) eacc[dd] = 0.0;
  for (long q = tid; q < M * D; q += KG_THREADS) zs[q] = 0.0;   // read again only behind the barriers of the first step

  const long s0 = (long)blockIdx.x * a.per, s1 = s0 + a.per < a.steps ? s0 + a.per : a.steps;
  for (long st = s0; st < s1; ++st) {
    const long j0 = st * KG_NB;
    __syncthreads();   // the readers of the previous step are done
    if (tid < KG_NB * D) {
      const long j = j0 + tid / D;
      xs[tid] = j < N ? (double)a.X[j * D + tid % D] : 0.0;
    } else if (tid >= 128 && tid < 128 + KG_NB * KG_PMAX) {
      const int q = tid - 128, c = q / KG_PMAX, p = q % KG_PMAX;
      if (WT) ys[q] = (j0 + c < N && p == 0) ? a.r[j0 + c] : 0.0;
      else ys[q] = (j0 + c < N && p < P) ? (double)a.Y[(j0 + c) * P + p] : 0.0;
    } else if (WT && tid >= 256 && tid < 256 + KG_NB) {
      wv[tid - 256] = j0 + (tid - 256) < N ? a.w[j0 + (tid - 256)] : 0.0;
    }
    __syncthreads();
    // K[:, step] in fragment order; columns beyond N hold zeros (E = 0 there)
    for (long e = tid; e < M * KG_NB; e += KG_THREADS) {
      const long f = e >> 6;
      const long k = 4 * (f >> 1) + (lane >> 4);
      const int c = 16 * (int)(f & 1) + (lane & 15);
      Ks[e] = j0 + c < N ? gram_value<double>(HB_KERN_RBF, a.z + k * D, xs + c * D, a.ell, a.dl, D) : 0.0;
    }
    __syncthreads();
    double xacc[XG ? 2 : 1][XG ? D : 1];   // column sums of e (z - x) over this lane's rows of the step
    if constexpr (XG) {
#pragma unroll
      for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int dd = 0; dd < D; ++dd) xacc[jt][dd] = 0.0;
    }
    for (long it = w; it < nrt; it += KG_NW) {
      MM::Acc acc[2];
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[0][r] = acc[1][r] = 0.0;
      const double* qf = a.Q + it * nks * 64 + lane;
#pragma unroll 4
      for (long s = 0; s < nks; ++s) {
        const double av = qf[s * 64];
        acc[0] = MM::mma(av, Ks[(2 * s) * 64 + lane], acc[0]);
        acc[1] = MM::mma(av, Ks[(2 * s + 1) * 64 + lane], acc[1]);
      }
      // accumulator r of lane l: row i = 16 it + l / 16 + 4 r, column c = 16 jt + l % 16; K[i][c] is fragment
      // (s = 4 it + r, jt), lane l
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long i = 16 * it + (lane >> 4) + 4 * r;
        double zi[D], zb[D], ri[KG_PMAX];
#pragma unroll
        for (int dd = 0; dd < D; ++dd) {
          zi[dd] = a.z[i * D + dd];
          zb[dd] = 0.0;
        }
#pragma unroll
        for (int p = 0; p < KG_PMAX; ++p) ri[p] = p < P ? a.R[i * P + p] : 0.0;
#pragma unroll
        for (int jt = 0; jt < 2; ++jt) {
          const int c = 16 * jt + (lane & 15);
          double kb = WT ? acc[jt][r] * wv[c] : acc[jt][r];
#pragma unroll
          for (int p = 0; p < KG_PMAX; ++p) kb = __builtin_fma(ri[p], ys[c * KG_PMAX + p], kb);
          const double e = kb * Ks[((4 * it + r) * 2 + jt) * 64 + lane];
#pragma unroll
          for (int dd = 0; dd < D; ++dd) {
            const double diff = zi[dd] - xs[c * D + dd];
            const double ed = e * diff;
            zb[dd] += ed;
            eacc[dd] = __builtin_fma(ed, diff, eacc[dd]);
            if constexpr (XG) xacc[jt][dd] += ed;
          }
        }
        // the 16 column lanes of row i folded in a fixed order; lane l % 16 == 0 owns row i's slots of zs
#pragma unroll
        for (int dd = 0; dd < D; ++dd) {
          double v = zb[dd];
#pragma unroll
          for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off, 64);
          if ((lane & 15) == 0) zs[i * D + dd] += v;
        }
      }
    }
    if constexpr (XG) {
      // the four lane groups l / 16 hold the rows l / 16 + 4 r of every row tile: fold them (16, then 32), then the 8
      // waves in wave order; xr is read again only behind the barrier at the top of the next step
      double* xr = zs + M * D;
#pragma unroll
      for (int jt = 0; jt < 2; ++jt)
#pragma unroll
        for (int dd = 0; dd < D; ++dd) {
          double v = xacc[jt][dd];
          v += __shfl_xor(v, 16, 64);
          v += __shfl_xor(v, 32, 64);
          if (lane < 16) xr[(w * KG_NB + 16 * jt + lane) * D + dd] = v;
        }
      __syncthreads();
      if (tid < KG_NB * D) {
        const int c = tid / D, dd = tid % D;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < KG_NW; ++k) s += xr[(k * KG_NB + c) * D + dd];
        const double l = a.ell[a.dl == 1 ? 0 : dd];
        if (j0 + c < N) a.xbar[(j0 + c) * D + dd] = s / (l * l);
      }
    }
  }

  // the strip's partials
  double* out = a.part + (long)blockIdx.x * a.stride;
#pragma unroll
  for (int dd = 0; dd < D; ++dd) {
    const double v = wave_sum(eacc[dd]);
    if (lane == 0) red[w * D + dd] = v;
  }
  __syncthreads();
  for (long q = tid; q < M * D; q += KG_THREADS) out[q] = zs[q];
  if (tid < D) {
    double s = 0.0;
    for (int k = 0; k < KG_NW; ++k) s += red[k * D + tid];
    out[M * D + tid] = s;
  }
}

// plain form: a workgroup walks its columns one at a time; thread i (strided) owns row i and its slots of the partials
// ([M, d] for zbar, then [M, d] row partials of ellbar)
// doubles of LDS the plain kernel takes: Kc, xc, yc, (weighted: the weight), (input gradient: the column's e and the
// waves' sums)
static inline size_t kg_plain_lds_elems(long M, long d, long P, bool weighted, bool xg) {
  return (size_t)(M + d + P + (weighted ? 1 : 0) + (xg ? M + (KG_PLAIN_T / 64) * d : 0));
}

template <typename T, bool WT, bool XG>
__global__ void __launch_bounds__(KG_PLAIN_T) sgp_kgrad_plain_kernel(KgArgs<T, XG> a) {
  extern __shared__ __attribute__((aligned(16))) double kg_smem[];
  const long M = a.M, N = a.N, d = a.d, P = a.P;
  double* Kc = kg_smem;   // [M]
  double* xc = Kc + M;    // [d]
  double* yc = xc + d;    // [P], then the column's weight (weighted form)
  // (input gradient only: Ec = yc + P (+ 1 weighted), [M], the column of E; xr = Ec + M, [4][d], the waves' sums)
  const int tid = threadIdx.x;
  double* zp = a.part + (long)blockIdx.x * a.stride;
  double* ep = zp + M * d;
  // zeroed by thread q % 256; from the first column on row i's slots are touched by thread i % 256 only, behind the
  // barrier at the top of the column loop
  for (long q = tid; q < 2 * M * d; q += KG_PLAIN_T) zp[q] = 0.0;
  const long c0 = (long)blockIdx.x * a.per, c1 = c0 + a.per < N ? c0 + a.per : N;
  for (long j = c0; j < c1; ++j) {
    __syncthreads();
    for (long q = tid; q < d + P + (WT ? 1 : 0); q += KG_PLAIN_T) {
      if (q < d) xc[q] = (double)a.X[j * d + q];
      else if (q == d + P) yc[P] = a.w[j];
      else yc[q - d] = WT ? a.r[j] : (double)a.Y[j * P + (q - d)];
    }
    __syncthreads();
    for (long k = tid; k < M; k += KG_PLAIN_T) Kc[k] = gram_value<double>(HB_KERN_RBF, a.z + k * d, xc, a.ell, a.dl, d);
    __syncthreads();
    for (long i = tid; i < M; i += KG_PLAIN_T) {
      double kb = 0.0;
      const double* qi = a.Q + i * M;
      for (long k = 0; k < M; ++k) kb = __builtin_fma(qi[k], Kc[k], kb);
      if (WT) kb *= yc[P];
      for (long p = 0; p < P; ++p) kb = __builtin_fma(a.R[i * P + p], yc[p], kb);
      const double e = kb * Kc[i];
      if constexpr (XG) yc[P + (WT ? 1 : 0) + i] = e;
      for (long dd = 0; dd < d; ++dd) {
        const double diff = a.z[i * d + dd] - xc[dd];
        const double ed = e * diff;
        zp[i * d + dd] += ed;
        ep[i * d + dd] = __builtin_fma(ed, diff, ep[i * d + dd]);
      }
    }
    if constexpr (XG) {
      // per dimension: this thread's strided rows, the wave by shuffles, the 4 waves in wave order (thread dd); Ec, xr
      // and xc are written again only behind the barriers at the top of the next column
      const double* Ec = yc + P + (WT ? 1 : 0);
      double* xr = yc + P + (WT ? 1 : 0) + M;
      __syncthreads();
      for (long dd = 0; dd < d; ++dd) {
        double s = 0.0;
        for (long i = tid; i < M; i += KG_PLAIN_T) {
          const double ed = Ec[i] * (a.z[i * d + dd] - xc[dd]);
          s += ed;
        }
        s = wave_sum(s);
        if ((tid & 63) == 0) xr[(tid >> 6) * d + dd] = s;
      }
      __syncthreads();
      if (tid < d) {
        double s = 0.0;
        for (int k = 0; k < KG_PLAIN_T / 64; ++k) s += xr[k * d + tid];
        const double l = a.ell[a.dl == 1 ? 0 : tid];
        a.xbar[j * d + tid] = s / (l * l);
      }
    }
  }
}

// zbar = -(sum over the strips) / ell^2, ellbar = (sum over the strips and the `ne` row partials) / ell^3 [summed over d
// for a scalar lengthscale], strip order.  The last block takes ellbar.
__global__ void __launch_bounds__(256) sgp_kgrad_fold_kernel(const double* __restrict__ part, long G, long stride, long M, long d,
                                                             long ne, const double* __restrict__ ell, long dl,
                                                             double* __restrict__ zbar, double* __restrict__ ellbar) {
  __shared__ double es[256];
  if (blockIdx.x == gridDim.x - 1) {
    // d <= 256 (checked by the host)
    if ((long)threadIdx.x < d) {
      const long dd = threadIdx.x;
      double s = 0.0;
      for (long g = 0; g < G; ++g)
        for (long r = 0; r < ne; ++r) s += part[g * stride + M * d + r * d + dd];
      const double l = ell[dl == 1 ? 0 : dd];
      es[dd] = s / (l * l * l);
    }
    __syncthreads();
    if (dl == 1) {
      if (threadIdx.x == 0) {
        double s = 0.0;
        for (long dd = 0; dd < d; ++dd) s += es[dd];
        ellbar[0] = s;
      }
    } else if ((long)threadIdx.x < d) {
      ellbar[threadIdx.x] = es[threadIdx.x];
    }
    return;
  }
  const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= M * d) return;
  double s = 0.0;
  for (long g = 0; g < G; ++g) s += part[g * stride + q];
  const double l = ell[dl == 1 ? 0 : q % d];
  zbar[q] = -s / (l * l);
}

static inline bool kg_is_fast(long M, long d, long P) {
  return M % 16 == 0 && M <= KG_MMAX && d <= KG_DMAX && P <= KG_PMAX && hb_debug_get("sgp_kgrad_plain", 0) == 0;
}

extern "C" long hb_sgp_kgrad_ws_elems(long N, long M, long d, long P) {
  (void)N;
  if (M <= 0 || d <= 0 || P <= 0) return 0;
  // the larger of the two forms, so that the diagnostic switch sgp_kgrad_plain needs no other workspace
  const long fast = hb_round64(M * M) + KG_MAXG * hb_round64(M * d + d), plain = KG_MAXG * hb_round64(2 * M * d);
  return fast > plain ? fast : plain;
}

template <typename T, int D, bool WT, bool XG>
static int kg_launch_strip(const KgArgs<T, XG>& a, long G, hipStream_t st) {
  const size_t lds = kg_strip_lds_elems(a.M, D, WT, XG) * sizeof(double);
  // once per instantiation: the largest M needs up to 150 KB (158 KB with the input gradient) of the CU's 160 KB
  static bool attr_set = false;
  if (!attr_set) {
    const size_t lds_max = kg_strip_lds_elems(KG_MMAX, D, WT, XG) * sizeof(double);
    HB_HIP(hipFuncSetAttribute((const void*)sgp_kgrad_strip_kernel<T, D, WT, XG>, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds_max));
    attr_set = true;
  }
  hipLaunchKernelGGL((sgp_kgrad_strip_kernel<T, D, WT, XG>), dim3((unsigned)G), dim3(KG_THREADS), lds, st, a);
  HB_LAUNCH_CHECK();
  return 0;
}

// WT: Y is NULL, P is 1 and w, r [N] are given (hb_sgp_wkgrad_*); else w, r are NULL (hb_sgp_kgrad_*).  XG: xbar [N, d]
// is written as well (the _x entries); else xbar is NULL and unused
template <typename T, bool WT, bool XG>
static int sgp_kgrad(int kind, const T* X, const T* Y, const double* w, const double* r, const double* z, const double* ell,
                     long dl, const double* Q, const double* R, double* zbar, double* ellbar, double* xbar, long N, long M,
                     long d, long P, double* ws, hipStream_t st) {
  const char* who = XG ? (WT ? "hb_sgp_wkgrad_x" : "hb_sgp_kgrad_x") : (WT ? "hb_sgp_wkgrad" : "hb_sgp_kgrad");
  HB_REQUIRE(N >= 1 && M >= 1 && d >= 1 && P >= 1, "%s: bad extents (N=%ld M=%ld d=%ld P=%ld)", who, N, M, d, P);
  HB_REQUIRE_RBF_MODEL(who, "is supported", kind, dl, d, (const void*)nullptr, M);   // (no Wfrag: W is not an operand)
  HB_REQUIRE(X && (WT ? (w && r) : Y != nullptr) && z && ell && Q && R, "%s: NULL input pointer", who);
  HB_REQUIRE(zbar && ellbar && (!XG || xbar), "%s: NULL output pointer", who);
  HB_REQUIRE(d <= 256 && P <= 256 && M + d + P <= 8000, "%s: M=%ld d=%ld P=%ld too large", who, M, d, P);
  HB_REQUIRE(ws && (uintptr_t)ws % 16 == 0, "%s: needs a 16-byte aligned workspace of %ld doubles", who,
             hb_sgp_kgrad_ws_elems(N, M, d, P));
  KgArgs<T, XG> a;
  if constexpr (XG) a.xbar = xbar;
  a.X = X; a.Y = Y; a.w = w; a.r = r; a.z = z; a.ell = ell; a.R = R; a.dl = dl; a.N = N; a.M = M; a.d = d; a.P = P;
  long G, ne;
  if (kg_is_fast(M, d, P)) {
    double* Qf = ws;
    hipLaunchKernelGGL(sgp_kgrad_pack_kernel, dim3(hb_stream_grid(M * M, 256)), dim3(256), 0, st, Q, Qf, M);
    HB_LAUNCH_CHECK();
    a.Q = Qf;
    a.part = ws + hb_round64(M * M);
    a.stride = hb_round64(M * d + d);
    a.steps = (N + KG_NB - 1) / KG_NB;
    a.per = (a.steps + KG_MAXG - 1) / KG_MAXG;
    G = (a.steps + a.per - 1) / a.per;   // <= KG_MAXG, every workgroup has at least one step
    ne = 1;
    int rc;
    switch (d) {
      case 1: rc = kg_launch_strip<T, 1, WT, XG>(a, G, st); break;
      case 2: rc = kg_launch_strip<T, 2, WT, XG>(a, G, st); break;
      case 3: rc = kg_launch_strip<T, 3, WT, XG>(a, G, st); break;
      default: rc = kg_launch_strip<T, 4, WT, XG>(a, G, st); break;
    }
    if (rc) return rc;
  } else {
    a.Q = Q;
    a.part = ws;
    a.stride = hb_round64(2 * M * d);
    a.steps = N;
    a.per = (N + KG_MAXG - 1) / KG_MAXG;
    G = (N + a.per - 1) / a.per;
    ne = M;
    const size_t lds = kg_plain_lds_elems(M, d, P, WT, XG) * sizeof(double);
    if constexpr (XG) {
      // the column of E doubles the footprint: up to 136 KB at the largest M + d + P the entry accepts
      static bool attr_set = false;
      if (!attr_set) {
        HB_HIP(hipFuncSetAttribute((const void*)sgp_kgrad_plain_kernel<T, WT, XG>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)(kg_plain_lds_elems(8000, 256, 0, WT, XG) * sizeof(double))));
        attr_set = true;
      }
    }
    hipLaunchKernelGGL((sgp_kgrad_plain_kernel<T, WT, XG>), dim3((unsigned)G), dim3(KG_PLAIN_T), lds, st, a);
    HB_LAUNCH_CHECK();
  }
  const long fb = (M * d + 255) / 256 + 1;
  hipLaunchKernelGGL(sgp_kgrad_fold_kernel, dim3((unsigned)fb), dim3(256), 0, st, (const double*)a.part, G, a.stride, M, d, ne,
                     ell, dl, zbar, ellbar);
  HB_LAUNCH_CHECK();
  return 0;
}

extern "C" int hb_sgp_kgrad_f32(int kind, const float* X, const float* Y, const double* z, const double* ell, long dl,
                                const double* Q, const double* R, double* zbar, double* ellbar, long N, long M, long d, long P,
                                double* ws, void* stream) {
  return sgp_kgrad<float, false, false>(kind, X, Y, nullptr, nullptr, z, ell, dl, Q, R, zbar, ellbar, nullptr, N, M, d, P, ws,
                                        (hipStream_t)stream);
}
extern "C" int hb_sgp_kgrad_f64(int kind, const double* X, const double* Y, const double* z, const double* ell, long dl,
                                const double* Q, const double* R, double* zbar, double* ellbar, long N, long M, long d, long P,
                                double* ws, void* stream) {
  return sgp_kgrad<double, false, false>(kind, X, Y, nullptr, nullptr, z, ell, dl, Q, R, zbar, ellbar, nullptr, N, M, d, P, ws,
                                         (hipStream_t)stream);
}
extern "C" int hb_sgp_wkgrad_f32(int kind, const float* X, const double* w, const double* r, const double* z, const double* ell,
                                 long dl, const double* Q, const double* R, double* zbar, double* ellbar, long N, long M, long d,
                                 double* ws, void* stream) {
  return sgp_kgrad<float, true, false>(kind, X, nullptr, w, r, z, ell, dl, Q, R, zbar, ellbar, nullptr, N, M, d, 1, ws,
                                       (hipStream_t)stream);
}
extern "C" int hb_sgp_wkgrad_f64(int kind, const double* X, const double* w, const double* r, const double* z, const double* ell,
                                 long dl, const double* Q, const double* R, double* zbar, double* ellbar, long N, long M, long d,
                                 double* ws, void* stream) {
  return sgp_kgrad<double, true, false>(kind, X, nullptr, w, r, z, ell, dl, Q, R, zbar, ellbar, nullptr, N, M, d, 1, ws,
                                        (hipStream_t)stream);
}
extern "C" int hb_sgp_kgrad_x_f32(int kind, const float* X, const float* Y, const double* z, const double* ell, long dl,
                                  const double* Q, const double* R, double* zbar, double* ellbar, double* xbar, long N, long M,
                                  long d, long P, double* ws, void* stream) {
  return sgp_kgrad<float, false, true>(kind, X, Y, nullptr, nullptr, z, ell, dl, Q, R, zbar, ellbar, xbar, N, M, d, P, ws,
                                       (hipStream_t)stream);
}
extern "C" int hb_sgp_kgrad_x_f64(int kind, const double* X, const double* Y, const double* z, const double* ell, long dl,
                                  const double* Q, const double* R, double* zbar, double* ellbar, double* xbar, long N, long M,
                                  long d, long P, double* ws, void* stream) {
  return sgp_kgrad<double, false, true>(kind, X, Y, nullptr, nullptr, z, ell, dl, Q, R, zbar, ellbar, xbar, N, M, d, P, ws,
                                        (hipStream_t)stream);
}
extern "C" int hb_sgp_wkgrad_x_f32(int kind, const float* X, const double* w, const double* r, const double* z,
                                   const double* ell, long dl, const double* Q, const double* R, double* zbar, double* ellbar,
                                   double* xbar, long N, long M, long d, double* ws, void* stream) {
  return sgp_kgrad<float, true, true>(kind, X, nullptr, w, r, z, ell, dl, Q, R, zbar, ellbar, xbar, N, M, d, 1, ws,
                                      (hipStream_t)stream);
}
extern "C" int hb_sgp_wkgrad_x_f64(int kind, const double* X, const double* w, const double* r, const double* z,
                                   const double* ell, long dl, const double* Q, const double* R, double* zbar, double* ellbar,
                                   double* xbar, long N, long M, long d, double* ws, void* stream) {
  return sgp_kgrad<double, true, true>(kind, X, nullptr, w, r, z, ell, dl, Q, R, zbar, ellbar, xbar, N, M, d, 1, ws,
                                       (hipStream_t)stream);
}
