// Input gradients of the exact GP's cached predictive and of its closed-form acquisition (hb_gram_predict_grad_*,
// include/henbun_hip.h; not in the reference).  With V = [P mean rows; S - P cache rows], K_ij = k(x2_i, x_j) the unit RBF
// and t[s, j] = scale sum_i V[s, i] K_ij the double hb_gram_predict holds,
//     u[s, j, k] = d t[s, j] / d x_jk = scale sum_i V[s, i] K_ij (x2_ik - x_jk) / ell_k^2
// is the value contraction with another right operand, B[r][c] (x2_rk - x_ck) (1 / ell_k^2): the operand of dimension k is
// formed in registers from the value tile as the MFMA loop reads it, from a small LDS table of the step's x2 rows per
// dimension and the coordinates of the lane's two columns -- the RBF step of sgp_pathwise_grad_kernel.  No second exp2, no
// second tile.  (1 + DG) accumulator sets: 32 right-hand sides per workgroup (two row tiles), 16 for double at d >= 3; d <= 4
// keeps all its dimensions in one workgroup, larger d takes them in groups of 4 on blockIdx.z, the K block synthesised
// again per group and the values stored by group 0.
//
// Phase 1 is gram_matvec_kernel's loop (gmv_tiles, csrc/gram_matvec.cuh, here with its derivative operands) -- the one
// K-block synthesis, V staging and K order, so every value accumulator tile sees the MFMA sequence it sees there and mean,
// var and val are the bits of hb_gram_predict -- on a grid of strips x chunks; every workgroup leaves its value partial
// and its d derivative partials in the workspace, plane q of it holding [chunks of the group, S, n] for the value (q = 0)
// and dimension q - 1.  Phase 2 folds the chunks of every plane in chunk order in double per column (carrying running
// sums [1 + d, S, n] between groups of GMV_GROUP chunks; one thread per dimension too, each folding the value rows
// itself) and on the last group emits
//     dmean[p, j, k] = (T) u[p, j, k]                           dvar[j, k] = (T) (-2 sum_{s >= P} t[s, j] u[s, j, k])
//     dval[j, k] = (T) (sgn a_mu u[0, j, k] + a_v (-2 sum ..))  (P = 1; a_mu, a_v: acq_point at (t[0, j], prior - q_j))
// with dvar exactly 0 where prior - q_j < 0 (the variance was clamped) and without cache rows.  No atomics; the order of
// every sum is fixed by N alone, so a column's outputs depend on nothing but the column.
#include "common.cuh"
#include "acq_tail.cuh"
#include "gram_matvec.cuh"
#include "../../include/henbun_hip.h"

#define GPG_SMAX 32      // right-hand sides per workgroup (2 row tiles of 16) ...
// ... but one row tile for double at d >= 3: (1 + d) sets of 2 x 2 double accumulator tiles spill (pwg_smax)
template <typename T> static inline long gpg_smax(long d) { return sizeof(T) == 8 && d >= 3 ? 16 : GPG_SMAX; }
#define GPG_DG 4         // dimensions per workgroup

template <typename T>
struct GpgArgs {
  GprArgs<T> p;    // p.g.ws: plane 0 of the partials, p.g.acc: plane 0 of the running sums; p.pkey, p.pcol unused
  long plane;      // elements of T from one plane of partials to the next
  long accplane;   // doubles from one plane of running sums to the next (S n)
  T* dmean;        // [P, n, d], nullable
  T* dvar;         // [n, d], nullable
  T* dval;         // [n, d], nullable
};

// D: as for gram_matvec_kernel; DG = D dimensions (all of them) for D in 1 .. 4, GPG_DG per blockIdx.z for D == 0
template <typename T, int D, int NST>
__global__ void __launch_bounds__(GMV_THREADS) gram_predict_grad_kernel(GpgArgs<T> ga) {
  typedef PwMma<T> MM;
  constexpr int DG = D ? D : GPG_DG;
  const GmvArgs<T>& a = ga.p.g;
  const int n = a.n, S = a.S, d = D ? D : a.d;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l16 = lane & 15;
  const int strip = blockIdx.x % a.nstrip, slot = blockIdx.x / a.nstrip;
  const int s0 = blockIdx.y * 16 * NST;          // (the host launches NST = its right-hand sides per workgroup / 16)
  const int k0 = D ? 0 : blockIdx.z * GPG_DG;    // first dimension of this workgroup
  const long col0 = (long)strip * GMV_CN + 32 * w;   // long: n may end within 128 of 2^31
  typename MM::Acc acc[NST][2], accd[DG][NST][2];
  gmv_tiles<T, D, NST, DG>(a, s0, k0, acc, accd);

  // masked store: register r of lane l is right-hand side s0 + 16 st + row(l, r), column col0 + 16 ct + l % 16
#pragma unroll
  for (int st = 0; st < NST; ++st)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int s = s0 + 16 * st + MM::row(lane, r);
        const long j = col0 + 16 * ct + l16;
        if (s < S && j < n) {
          const long e = ((long)slot * S + s) * n + j;
          if (k0 == 0) a.ws[e] = acc[st][ct][r];
#pragma unroll
          for (int k = 0; k < DG; ++k)
            if (k0 + k < d) a.ws[ga.plane * (1 + k0 + k) + e] = accd[k][st][ct][r];
        }
      }
}

// One thread per (column, dimension): the chunks of the value plane and of the dimension's plane added in chunk order in
// double, the running sums carried between groups; on the last group the column's outputs for that dimension, the thread
// of dimension 0 also those that have none (mean, var, val).  Every thread of a column folds the value rows itself -- the
// same additions, the same t -- so a column's d threads share nothing, and no per-thread array grows with d.  (Measured
// with one thread per column and the dimensions in registers: at n = N = 10^5, S = 257, d = 4, where the workspace limit
// cuts x into pieces of 11 000 columns, 44 workgroups of serial loops took 40 % of the call.)
template <typename T>
__global__ void __launch_bounds__(GPR_THREADS) gram_predict_grad_fold_kernel(GpgArgs<T> ga) {
  const GprArgs<T>& p = ga.p;
  const GmvArgs<T>& a = p.g;
  const long n = a.n, S = a.S, d = a.d, j = (long)blockIdx.x * GPR_THREADS + threadIdx.x;
  const bool first = a.c0 == 0, last = a.c0 + a.gchunks == a.nchunk;
  if (j >= n) return;
  const long cs = S * n;
  auto fold = [&](long q, long e) {   // plane q, element e = s n + j: 8 chunks' loads at a time, then their additions in order
    const T* __restrict__ part = a.ws + q * ga.plane + e;
    double sum = first ? 0.0 : a.acc[q * ga.accplane + e];
#pragma nounroll
    for (int c8 = 0; c8 < a.gchunks; c8 += 8) {
      T v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = c8 + i < a.gchunks ? part[(c8 + i) * cs] : T(0);
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (c8 + i < a.gchunks) sum += (double)v[i];
    }
    return sum;
  };
  for (long k = blockIdx.y; k < d; k += gridDim.y) {
    const bool lead = k == 0;
    double q = 0.0, t0 = 0.0, u0 = 0.0, dq = 0.0;
    for (long s = 0; s < S; ++s) {
      const long e = s * n + j;
      // before the last group only the thread of dimension 0 touches the value plane: it moves that running sum on
      const double sum = last || lead ? fold(0, e) : 0.0;
      const double su = fold(1 + k, e);
      if (!last) {
        if (lead) a.acc[e] = sum;
        a.acc[(1 + k) * ga.accplane + e] = su;
        continue;
      }
      const double t = a.scale * sum, u = a.scale * su;
      if (s == 0) t0 = t, u0 = u;
      if (s < p.P) {
        if (p.mean && lead) p.mean[e] = gmv_finish<T>(a.scale, 0.0, sum, 0.0);   // the bits of hb_gram_matvec
        if (ga.dmean) ga.dmean[e * d + k] = (T)u;
      } else {
#pragma clang fp contract(off)   // two roundings each, never an fma: a host can restate the sums exactly
        const double sq = t * t, tu = t * u;
        q = q + sq;
        dq = dq + tu;
      }
    }
    if (!last) continue;
    const double vr = p.prior - q;
    if (p.var && lead) p.var[j] = (T)(vr < 0.0 ? 0.0 : vr);
    AcqPoint pt;
    pt.val = 0.0, pt.a_mu = 0.0, pt.a_v = 0.0;
    if (p.t.acq != ACQ_NONE) {
      pt = acq_point(p.t, t0, vr);
      if (p.val && lead) p.val[j] = (T)pt.val;
    }
    const double dv = (vr < 0.0 || S == p.P) ? 0.0 : -2.0 * dq;
    if (ga.dvar) ga.dvar[j * d + k] = (T)dv;
    if (ga.dval) {
#pragma clang fp contract(off)   // each product and the sum rounded once
      const double am = (p.t.largest ? 1.0 : -1.0) * pt.a_mu * u0, av = pt.a_v * dv;
      ga.dval[j * d + k] = (T)(am + av);
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
template <typename T, int D>
static void gram_predict_grad_launch_d(const GpgArgs<T>& a, int nst, dim3 grid, hipStream_t st) {
  if constexpr (sizeof(T) == 8 && (D == 0 || D >= 3)) {   // gpg_smax: one row tile
    hipLaunchKernelGGL((gram_predict_grad_kernel<T, D, 1>), grid, dim3(GMV_THREADS), 0, st, a);
  } else {
    if (nst == 1)
      hipLaunchKernelGGL((gram_predict_grad_kernel<T, D, 1>), grid, dim3(GMV_THREADS), 0, st, a);
    else
      hipLaunchKernelGGL((gram_predict_grad_kernel<T, D, 2>), grid, dim3(GMV_THREADS), 0, st, a);
  }
}

// workspace, in elements of T: (1 + d) planes of a group's partials (each rounded up to 8 bytes) and, beyond one group,
// (1 + d) running double sums [S, n]
extern "C" long hb_gram_predict_grad_ws_elems(long n, long N, long d, long S, int dtype_bytes) {
  if (n <= 0 || N <= 0 || d <= 0 || S <= 0) return 0;
  const int bytes = dtype_bytes == 4 ? 4 : 8;
  const long per = 8 / bytes, nchunk = (N + GMV_CHUNK - 1) / GMV_CHUNK;
  return (1 + d) * (gpr_part_elems(n, N, S, bytes) + (nchunk > GMV_GROUP ? S * n * per : 0));
}

template <typename T>
static int gram_predict_grad(int kind, const T* x, const T* x2, const T* ell, long dl, const T* V, long P, double scale,
                             double prior, int acq, double best, double param, int largest, double var_floor, T* mean, T* var,
                             T* val, T* dmean, T* dvar, T* dval, long n, long N, long d, long S, T* ws, hipStream_t st) {
  HB_REQUIRE(kind == HB_KERN_RBF, "hb_gram_predict_grad: the UnitRBF kernel only (kind=%d)", kind);
  HB_REQUIRE(n >= 0 && N >= 1 && d >= 1 && S >= 1, "hb_gram_predict_grad: bad extents (n=%ld N=%ld d=%ld S=%ld)", n, N, d, S);
  HB_REQUIRE(P >= 1 && P <= S, "hb_gram_predict_grad: 1 <= P <= S mean rows expected (P=%ld S=%ld)", P, S);
  HB_REQUIRE(dl == 1 || dl == d, "hb_gram_predict_grad: lengthscales must have 1 or d entries");
  HB_REQUIRE(ell && x2 && V && (n == 0 || x), "hb_gram_predict_grad: NULL pointer");
  if (acq == ACQ_NONE) {
    HB_REQUIRE(!val && !dval, "hb_gram_predict_grad: val and dval need an acquisition (acq=%d)", acq);
    HB_REQUIRE(mean || var || dmean || dvar, "hb_gram_predict_grad: at least one of mean, var, dmean, dvar must be given");
  } else {
    HB_REQUIRE(acq == HB_ACQ_EI || acq == HB_ACQ_PI || acq == HB_ACQ_UCB, "hb_gram_predict_grad: unknown acquisition %d", acq);
    HB_REQUIRE(P == 1, "hb_gram_predict_grad: an acquisition is defined for one latent function only (P=%ld)", P);
    HB_REQUIRE(mean || var || val || dmean || dvar || dval, "hb_gram_predict_grad: at least one output must be given");
    HB_REQUIRE(var_floor >= 0.0 && best == best && param == param,
               "hb_gram_predict_grad: var_floor >= 0 and numbers for best and param expected (var_floor=%g best=%g param=%g)",
               var_floor, best, param);
  }
  HB_REQUIRE(prior == prior && scale == scale, "hb_gram_predict_grad: numbers for scale and prior expected");
  const long nstrip = (n + GMV_CN - 1) / GMV_CN, nchunk = (N + GMV_CHUNK - 1) / GMV_CHUNK;
  const long group = nchunk < GMV_GROUP ? nchunk : GMV_GROUP, smax = gpg_smax<T>(d);
  HB_REQUIRE(n <= 2147483647L && N <= 2147483647L && S <= 2147483647L && nstrip * group <= 2147483647L &&
                 hb_cdiv(S, smax) <= 65535 && d <= 65535L * GPG_DG && group * S <= (1L << 60) / ((1 + d) * (n ? n : 1)),
             "hb_gram_predict_grad: too large (n, N below 2^31, strips x chunks of a group below 2^31, S at most 16 x 65535, d at "
             "most 4 x 65535, the workspace below 2^60 elements)");
  if (n == 0) return 0;
  HB_REQUIRE(ws && (uintptr_t)ws % 16 == 0, "hb_gram_predict_grad: needs a 16-byte aligned workspace (hb_gram_predict_grad_ws_elems)");

  GpgArgs<T> ga;
  GprArgs<T>& p = ga.p;
  GmvArgs<T>& a = p.g;
  a.x = x; a.x2 = x2; a.ell = ell; a.dl = dl; a.V = V; a.scale = scale; a.shift = 0.0; a.shift_on = 0; a.out = nullptr;
  a.ws = ws; a.to_ws = 1;
  a.n = (int)n; a.N = (int)N; a.d = (int)d; a.S = (int)S; a.nstrip = (int)nstrip; a.nchunk = (int)nchunk;
  ga.plane = gpr_part_elems(n, N, S, (int)sizeof(T));
  ga.accplane = S * n;
  a.acc = nchunk > GMV_GROUP ? reinterpret_cast<double*>(ws + (1 + d) * ga.plane) : nullptr;
  p.pkey = nullptr; p.pcol = nullptr;
  p.P = (int)P; p.prior = prior; p.mean = mean; p.var = var; p.val = val;
  p.t.acq = acq; p.t.largest = largest != 0; p.t.best = best; p.t.param = param; p.t.scale = 1.0; p.t.var_floor = var_floor;
  ga.dmean = dmean; ga.dvar = dvar; ga.dval = dval;
  const long nb = (n + GPR_THREADS - 1) / GPR_THREADS;
  // every workgroup of the grid carries the same number of row tiles: those of min(S, gpg_smax) right-hand sides
  const int nst = hb_cdiv(S < smax ? S : smax, 16);
  for (long c0 = 0; c0 < nchunk; c0 += GMV_GROUP) {
    a.c0 = (int)c0;
    a.gchunks = (int)(nchunk - c0 < GMV_GROUP ? nchunk - c0 : GMV_GROUP);
    const dim3 grid((unsigned)(nstrip * a.gchunks), (unsigned)hb_cdiv(S, smax), d <= 4 ? 1u : (unsigned)hb_cdiv(d, GPG_DG));
    if (d == 1)
      gram_predict_grad_launch_d<T, 1>(ga, nst, grid, st);
    else if (d == 2)
      gram_predict_grad_launch_d<T, 2>(ga, nst, grid, st);
    else if (d == 3)
      gram_predict_grad_launch_d<T, 3>(ga, nst, grid, st);
    else if (d == 4)
      gram_predict_grad_launch_d<T, 4>(ga, nst, grid, st);
    else
      gram_predict_grad_launch_d<T, 0>(ga, nst, grid, st);
    HB_LAUNCH_CHECK();
    hipLaunchKernelGGL((gram_predict_grad_fold_kernel<T>), dim3((unsigned)nb, (unsigned)(d < 65535 ? d : 65535)), dim3(GPR_THREADS), 0,
                       st, ga);
    HB_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int hb_gram_predict_grad_f32(int kind, const float* x, const float* x2, const float* ell, long dl, const float* V, long P,
                                        double scale, double prior, int acq, double best, double param, int largest,
                                        double var_floor, float* mean, float* var, float* val, float* dmean, float* dvar,
                                        float* dval, long n, long N, long d, long S, float* ws, void* stream) {
  return gram_predict_grad<float>(kind, x, x2, ell, dl, V, P, scale, prior, acq, best, param, largest, var_floor, mean, var, val,
                                  dmean, dvar, dval, n, N, d, S, ws, (hipStream_t)stream);
}
extern "C" int hb_gram_predict_grad_f64(int kind, const double* x, const double* x2, const double* ell, long dl, const double* V,
                                        long P, double scale, double prior, int acq, double best, double param, int largest,
                                        double var_floor, double* mean, double* var, double* val, double* dmean, double* dvar,
                                        double* dval, long n, long N, long d, long S, double* ws, void* stream) {
  return gram_predict_grad<double>(kind, x, x2, ell, dl, V, P, scale, prior, acq, best, param, largest, var_floor, mean, var, val,
                                   dmean, dvar, dval, n, N, d, S, ws, (hipStream_t)stream);
}
