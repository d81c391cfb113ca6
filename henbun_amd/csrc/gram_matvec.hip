// Matrix-free kernel product (hb_gram_matvec_*), the exact GP's predictive pass built on the same kernel (hb_gram_predict_*:
// mean, cached variance bound, closed-form acquisition and its arg-max; further down) and the vector kernels of the
// lockstep preconditioned conjugate gradients (hb_pcg_*), include/henbun_hip.h; not in the reference; Gardner et al. 2018,
// Wang et al. 2019.
//
//     out[s, j] = scale * sum_{i < N} V[s, i] k(x2_i, x_j) + shift * V[s, j]
//
// K(x2, x) is never written to memory.  The kernel is the RBF section of sgp_pathwise_kernel -- a workgroup per strip of
// GMV_CN columns (a wave per 32 of them) walks rows in K-steps of GMV_KT, each wave synthesises the GMV_KT x 32 block of
// its own columns into LDS in the difference-then-scale exp2 form of sgp_strip.cuh, the workgroup stages the matching tile
// of V through registers, and the product runs on the 16 x 16 x 4 MFMA of the dtype with the right-hand sides on the rows
// -- with one change: the rows are cut into chunks of GMV_CHUNK and the grid is strips x chunks x tiles of GMV_SMAX
// right-hand sides.  n = N = 8192 is then 256 workgroups instead of 64, and no accumulator of the storage type ever sums
// more than GMV_CHUNK terms.  With more than one chunk a workgroup leaves its partial [S, strip] in the workspace and a
// second launch adds the chunks in chunk order in double, applies scale and shift and writes out; with one chunk the same
// finish runs in the kernel's epilogue and the workspace is not touched.  More than GMV_GROUP chunks are taken GMV_GROUP
// at a time, the fold carrying its running double sum [S, n] from one group to the next: the same additions in the same
// order, and a workspace of (GMV_GROUP sizeof(T) + 8) S n bytes whatever N.
//
// The order of every sum is fixed by N alone (K-steps inside a chunk, chunks in order): an output element does not
// depend on the other columns, on S or on n, so two calls, or x evaluated in pieces, return the same bits.
//
// K(X, X) is symmetric and the symmetric call synthesises every value twice; halving that needs the transposed
// accumulation of a block into other workgroups' columns ("Exact GP by conjugate gradients": the next step).
#include "common.cuh"
#include "sgp_pathwise.cuh"   // pw_takes: the arg-max rule
#include "acq_tail.cuh"
#include "gram_matvec.cuh"   // GMV_*, GmvArgs, gmv_tiles, gmv_finish, GPR_THREADS, GprArgs, gpr_part_elems: shared with gram_predict_grad.hip
#include "../../include/henbun_hip.h"

// D: the input dimension when it is at most 4 (the column's coordinates then live in registers), 0: any d, the
// coordinates re-read from memory at every use.  NST: row tiles of 16 right-hand sides per workgroup.
template <typename T, int D, int NST>
__global__ void __launch_bounds__(GMV_THREADS) gram_matvec_kernel(GmvArgs<T> a) {
  typedef PwMma<T> MM;
  const int n = a.n, N = a.N, S = a.S;
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l16 = lane & 15;
  const int strip = blockIdx.x % a.nstrip, slot = blockIdx.x / a.nstrip;
  const int s0 = blockIdx.y * GMV_SMAX;
  const long col0 = (long)strip * GMV_CN + 32 * w;   // long: n may end within 128 of 2^31
  typename MM::Acc acc[NST][2], none[1][NST][2];
  gmv_tiles<T, D, NST, 0>(a, s0, 0, acc, none);

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
          if (a.nchunk == 1 && !a.to_ws) {
            const double v = a.shift_on ? (double)a.V[(long)s * N + j] : 0.0;
            a.out[(long)s * n + j] = gmv_finish<T>(a.scale, a.shift, (double)acc[st][ct][r], v);
          } else {
            a.ws[((long)slot * S + s) * n + j] = acc[st][ct][r];
          }
        }
      }
}

// out[s, j] = scale * (the chunks' partials added in chunk order, in double) + shift * V[s, j]; one call per group of
// chunks, the running sum kept in a.acc from the first group to the last
template <typename T>
__global__ void __launch_bounds__(256) gram_matvec_fold_kernel(GmvArgs<T> a) {
  const long total = (long)a.S * a.n;
  const bool first = a.c0 == 0, last = a.c0 + a.gchunks == a.nchunk;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    double sum = first ? 0.0 : a.acc[e];
    for (int ch = 0; ch < a.gchunks; ++ch) sum += (double)a.ws[(long)ch * total + e];
    if (last) {
      const double v = a.shift_on ? (double)a.V[e] : 0.0;   // symmetric: N == n, V [S, n]
      a.out[e] = gmv_finish<T>(a.scale, a.shift, sum, v);
    } else {
      a.acc[e] = sum;
    }
  }
}

template <typename T, int D>
static void gram_matvec_launch_d(const GmvArgs<T>& a, int nst, dim3 grid, hipStream_t st) {
  if (nst == 1)
    hipLaunchKernelGGL((gram_matvec_kernel<T, D, 1>), grid, dim3(GMV_THREADS), 0, st, a);
  else if (nst == 2)
    hipLaunchKernelGGL((gram_matvec_kernel<T, D, 2>), grid, dim3(GMV_THREADS), 0, st, a);
  else if (nst == 3)
    hipLaunchKernelGGL((gram_matvec_kernel<T, D, 3>), grid, dim3(GMV_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL((gram_matvec_kernel<T, D, 4>), grid, dim3(GMV_THREADS), 0, st, a);
}

// phase 1 of one group of chunks: shared by hb_gram_matvec and hb_gram_predict
template <typename T>
static void gram_matvec_launch(const GmvArgs<T>& a, hipStream_t st) {
  // every workgroup of the grid carries the same number of row tiles: those of min(S, GMV_SMAX) right-hand sides
  const int nst = hb_cdiv(a.S < GMV_SMAX ? a.S : GMV_SMAX, 16);
  const dim3 grid((unsigned)((long)a.nstrip * a.gchunks), (unsigned)hb_cdiv(a.S, GMV_SMAX), 1);
  if (a.d == 1)
    gram_matvec_launch_d<T, 1>(a, nst, grid, st);
  else if (a.d == 2)
    gram_matvec_launch_d<T, 2>(a, nst, grid, st);
  else if (a.d == 3)
    gram_matvec_launch_d<T, 3>(a, nst, grid, st);
  else if (a.d == 4)
    gram_matvec_launch_d<T, 4>(a, nst, grid, st);
  else
    gram_matvec_launch_d<T, 0>(a, nst, grid, st);
}

extern "C" long hb_gram_matvec_chunk(void) { return GMV_CHUNK; }

extern "C" long hb_gram_matvec_ws_elems(long n, long N, long S, int dtype_bytes) {
  if (n <= 0 || N <= GMV_CHUNK || S <= 0) return 0;
  const long nchunk = (N + GMV_CHUNK - 1) / GMV_CHUNK;
  if (nchunk <= GMV_GROUP) return nchunk * S * n;
  return GMV_GROUP * S * n + S * n * (8 / (dtype_bytes == 4 ? 4 : 8));   // the partials of a group + the double running sum
}

template <typename T>
static int gram_matvec(int kind, const T* x, const T* x2, const T* ell, long dl, const T* V, double scale, double shift, T* out,
                       long n, long N, long d, long S, T* ws, hipStream_t st) {
  HB_REQUIRE(kind == HB_KERN_RBF, "hb_gram_matvec: the UnitRBF kernel only (kind=%d)", kind);
  HB_REQUIRE(n >= 0 && N >= 0 && d >= 1 && S >= 1, "hb_gram_matvec: bad extents (n=%ld N=%ld d=%ld S=%ld)", n, N, d, S);
  HB_REQUIRE(dl == 1 || dl == d, "hb_gram_matvec: lengthscales must have 1 or d entries");
  HB_REQUIRE(x2 || N == n || N == 0, "hb_gram_matvec: x2 == NULL is the symmetric form, N must equal n (n=%ld N=%ld)", n, N);
  HB_REQUIRE(!x2 || shift == 0.0, "hb_gram_matvec: shift != 0 is defined for the symmetric form (x2 == NULL) only");
  HB_REQUIRE(ell && (n == 0 || (x && out)) && (V || N == 0), "hb_gram_matvec: NULL pointer");
  const long nstrip = (n + GMV_CN - 1) / GMV_CN, nchunk = (N + GMV_CHUNK - 1) / GMV_CHUNK;
  HB_REQUIRE(n <= 2147483647L && N <= 2147483647L && d <= 2147483647L && S <= 2147483647L &&
                 nstrip * nchunk <= 2147483647L && hb_cdiv(S, GMV_SMAX) <= 65535,
             "hb_gram_matvec: too large (n, N below 2^31, strips x chunks below 2^31, S at most 64 x 65535)");
  HB_REQUIRE(ws || hb_gram_matvec_ws_elems(n, N, S, (int)sizeof(T)) == 0, "hb_gram_matvec: NULL workspace (hb_gram_matvec_ws_elems)");
  if (n == 0) return 0;
  if (N == 0) {
    HB_HIP(hb_zero_async(out, (size_t)S * (size_t)n * sizeof(T), st));
    return 0;
  }
  GmvArgs<T> a;
  a.x = x; a.x2 = x2 ? x2 : x; a.ell = ell; a.dl = dl; a.V = V; a.scale = scale; a.shift = shift;
  a.shift_on = x2 ? 0 : 1; a.out = out; a.ws = ws; a.to_ws = 0;
  a.n = (int)n; a.N = (int)N; a.d = (int)d; a.S = (int)S; a.nstrip = (int)nstrip; a.nchunk = (int)nchunk;
  a.acc = nchunk > GMV_GROUP ? reinterpret_cast<double*>(ws + (long)GMV_GROUP * S * n) : nullptr;
  for (long c0 = 0; c0 < nchunk; c0 += GMV_GROUP) {
    a.c0 = (int)c0;
    a.gchunks = (int)(nchunk - c0 < GMV_GROUP ? nchunk - c0 : GMV_GROUP);
    gram_matvec_launch<T>(a, st);
    HB_LAUNCH_CHECK();
    if (nchunk > 1) {
      hipLaunchKernelGGL((gram_matvec_fold_kernel<T>), dim3(hb_stream_grid(S * n, 256)), dim3(256), 0, st, a);
      HB_LAUNCH_CHECK();
    }
  }
  return 0;
}

extern "C" int hb_gram_matvec_f32(int kind, const float* x, const float* x2, const float* ell, long dl, const float* V,
                                  double scale, double shift, float* out, long n, long N, long d, long S, float* ws,
                                  void* stream) {
  return gram_matvec<float>(kind, x, x2, ell, dl, V, scale, shift, out, n, N, d, S, ws, (hipStream_t)stream);
}
extern "C" int hb_gram_matvec_f64(int kind, const double* x, const double* x2, const double* ell, long dl, const double* V,
                                  double scale, double shift, double* out, long n, long N, long d, long S, double* ws,
                                  void* stream) {
  return gram_matvec<double>(kind, x, x2, ell, dl, V, scale, shift, out, n, N, d, S, ws, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------
// hb_gram_predict: predictive mean rows, a cached predictive variance and a closed-form acquisition from ONE product.
// With t[s, j] the double hb_gram_matvec holds before its final rounding (the chunks' partials added in chunk order, times
// scale, no shift), V = [P mean rows; S - P cache rows]:
//     mean[p, j] = (T) t[p, j]            q_j = sum_{s >= P} t[s, j]^2  (double, s ascending)
//     var[j] = (T) max(prior - q_j, 0)    val[j] = (T) acq_point(t[0, j], prior - q_j)   (P = 1)
// Phase 1 is gram_matvec_kernel with to_ws set: every chunk, a single one too, leaves its partial in the workspace.
// Phase 2, one thread per column, folds the chunks of each row in double (carrying the running sum between groups, as
// gram_matvec_fold_kernel does) and, on the last group, emits the column's outputs and a per-workgroup arg-max partial;
// a one-workgroup launch folds those in block order (pw_takes).  No atomics; a column's outputs depend on nothing but
// the column.
template <typename T>
__global__ void __launch_bounds__(GPR_THREADS) gram_predict_fold_kernel(GprArgs<T> p) {
  __shared__ double Rk[GPR_THREADS];
  __shared__ long Rj[GPR_THREADS];
  const GmvArgs<T>& a = p.g;
  const int tid = threadIdx.x;
  const long n = a.n, S = a.S, j = (long)blockIdx.x * GPR_THREADS + tid;
  const bool first = a.c0 == 0, last = a.c0 + a.gchunks == a.nchunk;
  double key = 0.0;
  long jb = -1;
  if (j < n) {
    double q = 0.0, t0 = 0.0;
    for (long s = 0; s < S; ++s) {
      const long e = s * n + j;
      double sum = first ? 0.0 : a.acc[e];
      for (int ch = 0; ch < a.gchunks; ++ch) sum += (double)a.ws[(long)ch * S * n + e];
      if (!last) {
        a.acc[e] = sum;
        continue;
      }
      const double t = a.scale * sum;
      if (s == 0) t0 = t;
      if (s < p.P) {
        if (p.mean) p.mean[e] = gmv_finish<T>(a.scale, 0.0, sum, 0.0);   // the bits of hb_gram_matvec
      } else {
#pragma clang fp contract(off)   // two roundings, never an fma: a host can restate the sum exactly
        const double sq = t * t;
        q = q + sq;
      }
    }
    if (last) {
      const double vr = p.prior - q;
      if (p.var) p.var[j] = (T)(vr < 0.0 ? 0.0 : vr);
      if (p.t.acq != ACQ_NONE) {
        const T v = (T)acq_point(p.t, t0, vr).val;
        if (p.val) p.val[j] = v;
        key = (double)v;
        if (key == key) jb = j;
      }
    }
  }
  if (p.pkey && last) {   // (uniform)
    Rk[tid] = key, Rj[tid] = jb;
    __syncthreads();
    for (int m = GPR_THREADS / 2; m > 0; m >>= 1) {
      if (tid < m && pw_takes<double>(Rk[tid + m], Rj[tid + m], Rk[tid], Rj[tid])) Rk[tid] = Rk[tid + m], Rj[tid] = Rj[tid + m];
      __syncthreads();
    }
    if (tid == 0) p.pkey[blockIdx.x] = Rk[0], p.pcol[blockIdx.x] = Rj[0];
  }
}

// one workgroup: the blocks' partials in block order; no comparable value at all: idx = -1 and best_val = -inf
__global__ void __launch_bounds__(GPR_THREADS) gram_predict_argmax_kernel(const double* __restrict__ pkey, const long* __restrict__ pcol,
                                                                          long nb, double* __restrict__ best_val,
                                                                          long* __restrict__ best_idx) {
  __shared__ double Rk[GPR_THREADS];
  __shared__ long Rj[GPR_THREADS];
  const int tid = threadIdx.x;
  double bk = -INFINITY;
  long bj = -1;
  for (long b = tid; b < nb; b += GPR_THREADS)
    if (pw_takes<double>(pkey[b], pcol[b], bk, bj)) bk = pkey[b], bj = pcol[b];
  Rk[tid] = bk, Rj[tid] = bj;
  __syncthreads();
  for (int m = GPR_THREADS / 2; m > 0; m >>= 1) {
    if (tid < m && pw_takes<double>(Rk[tid + m], Rj[tid + m], Rk[tid], Rj[tid])) Rk[tid] = Rk[tid + m], Rj[tid] = Rj[tid + m];
    __syncthreads();
  }
  if (tid == 0) {
    if (best_val) *best_val = Rj[0] < 0 ? -INFINITY : Rk[0];
    if (best_idx) *best_idx = Rj[0];
  }
}

// workspace: gpr_part_elems (csrc/gram_matvec.cuh) for the partials, then the running sum and the arg-max partials
extern "C" long hb_gram_predict_ws_elems(long n, long N, long S, int dtype_bytes) {
  if (n <= 0 || N <= 0 || S <= 0) return 0;
  const int bytes = dtype_bytes == 4 ? 4 : 8;
  const long per = 8 / bytes, nchunk = (N + GMV_CHUNK - 1) / GMV_CHUNK;
  return gpr_part_elems(n, N, S, bytes) + (nchunk > GMV_GROUP ? S * n * per : 0) + 2 * per * ((n + GPR_THREADS - 1) / GPR_THREADS);
}

template <typename T>
static int gram_predict(int kind, const T* x, const T* x2, const T* ell, long dl, const T* V, long P, double scale, double prior,
                        int acq, double best, double param, int largest, double var_floor, T* mean, T* var, T* val,
                        double* best_val, long* best_idx, long n, long N, long d, long S, T* ws, hipStream_t st) {
  HB_REQUIRE(kind == HB_KERN_RBF, "hb_gram_predict: the UnitRBF kernel only (kind=%d)", kind);
  HB_REQUIRE(n >= 0 && N >= 1 && d >= 1 && S >= 1, "hb_gram_predict: bad extents (n=%ld N=%ld d=%ld S=%ld)", n, N, d, S);
  HB_REQUIRE(P >= 1 && P <= S, "hb_gram_predict: 1 <= P <= S mean rows expected (P=%ld S=%ld)", P, S);
  HB_REQUIRE(dl == 1 || dl == d, "hb_gram_predict: lengthscales must have 1 or d entries");
  HB_REQUIRE(ell && x2 && V && (n == 0 || x), "hb_gram_predict: NULL pointer");
  const bool amax = best_val || best_idx;
  if (acq == ACQ_NONE) {
    HB_REQUIRE(!val && !amax, "hb_gram_predict: val, best_val and best_idx need an acquisition (acq=%d)", acq);
    HB_REQUIRE(mean || var, "hb_gram_predict: at least one of mean, var must be given");
  } else {
    HB_REQUIRE(acq == HB_ACQ_EI || acq == HB_ACQ_PI || acq == HB_ACQ_UCB, "hb_gram_predict: unknown acquisition %d", acq);
    HB_REQUIRE(P == 1, "hb_gram_predict: an acquisition is defined for one latent function only (P=%ld)", P);
    HB_REQUIRE(mean || var || val || amax, "hb_gram_predict: at least one output must be given");
    HB_REQUIRE(var_floor >= 0.0 && best == best && param == param,
               "hb_gram_predict: var_floor >= 0 and numbers for best and param expected (var_floor=%g best=%g param=%g)", var_floor,
               best, param);
    HB_REQUIRE(!amax || n >= 1, "hb_gram_predict: an arg-max needs at least one candidate (n=%ld)", n);
  }
  HB_REQUIRE(prior == prior && scale == scale, "hb_gram_predict: numbers for scale and prior expected");
  const long nstrip = (n + GMV_CN - 1) / GMV_CN, nchunk = (N + GMV_CHUNK - 1) / GMV_CHUNK;
  HB_REQUIRE(n <= 2147483647L && N <= 2147483647L && d <= 2147483647L && S <= 2147483647L &&
                 nstrip * (nchunk < GMV_GROUP ? nchunk : GMV_GROUP) <= 2147483647L && hb_cdiv(S, GMV_SMAX) <= 65535,
             "hb_gram_predict: too large (n, N below 2^31, strips x chunks of a group below 2^31, S at most 64 x 65535)");
  if (n == 0) return 0;
  HB_REQUIRE(ws && (uintptr_t)ws % 16 == 0, "hb_gram_predict: needs a 16-byte aligned workspace (hb_gram_predict_ws_elems)");

  GprArgs<T> p;
  GmvArgs<T>& a = p.g;
  a.x = x; a.x2 = x2; a.ell = ell; a.dl = dl; a.V = V; a.scale = scale; a.shift = 0.0; a.shift_on = 0; a.out = nullptr;
  a.ws = ws; a.to_ws = 1;
  a.n = (int)n; a.N = (int)N; a.d = (int)d; a.S = (int)S; a.nstrip = (int)nstrip; a.nchunk = (int)nchunk;
  T* after = ws + gpr_part_elems(n, N, S, (int)sizeof(T));
  a.acc = nchunk > GMV_GROUP ? reinterpret_cast<double*>(after) : nullptr;
  if (a.acc) after += S * n * (long)(8 / sizeof(T));
  const long nb = (n + GPR_THREADS - 1) / GPR_THREADS;
  p.pkey = amax ? reinterpret_cast<double*>(after) : nullptr;
  p.pcol = amax ? reinterpret_cast<long*>(after) + nb : nullptr;
  p.P = (int)P; p.prior = prior; p.mean = mean; p.var = var; p.val = val;
  p.t.acq = acq; p.t.largest = largest != 0; p.t.best = best; p.t.param = param; p.t.scale = 1.0; p.t.var_floor = var_floor;
  for (long c0 = 0; c0 < nchunk; c0 += GMV_GROUP) {
    a.c0 = (int)c0;
    a.gchunks = (int)(nchunk - c0 < GMV_GROUP ? nchunk - c0 : GMV_GROUP);
    gram_matvec_launch<T>(a, st);
    HB_LAUNCH_CHECK();
    hipLaunchKernelGGL((gram_predict_fold_kernel<T>), dim3((unsigned)nb), dim3(GPR_THREADS), 0, st, p);
    HB_LAUNCH_CHECK();
  }
  if (amax) {
    hipLaunchKernelGGL(gram_predict_argmax_kernel, dim3(1), dim3(GPR_THREADS), 0, st, (const double*)p.pkey, (const long*)p.pcol, nb,
                       best_val, best_idx);
    HB_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int hb_gram_predict_f32(int kind, const float* x, const float* x2, const float* ell, long dl, const float* V, long P,
                                   double scale, double prior, int acq, double best, double param, int largest, double var_floor,
                                   float* mean, float* var, float* val, double* best_val, long* best_idx, long n, long N, long d,
                                   long S, float* ws, void* stream) {
  return gram_predict<float>(kind, x, x2, ell, dl, V, P, scale, prior, acq, best, param, largest, var_floor, mean, var, val, best_val,
                             best_idx, n, N, d, S, ws, (hipStream_t)stream);
}
extern "C" int hb_gram_predict_f64(int kind, const double* x, const double* x2, const double* ell, long dl, const double* V, long P,
                                   double scale, double prior, int acq, double best, double param, int largest, double var_floor,
                                   double* mean, double* var, double* val, double* best_val, long* best_idx, long n, long N,
                                   long d, long S, double* ws, void* stream) {
  return gram_predict<double>(kind, x, x2, ell, dl, V, P, scale, prior, acq, best, param, largest, var_floor, mean, var, val, best_val,
                              best_idx, n, N, d, S, ws, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------
// Lockstep preconditioned conjugate gradients: S independent iterations over rows of length N, one workgroup per row.
// Every dot product and every scalar (alpha, beta, |r|^2) is double whatever the storage type; a row's sums run in a
// fixed order (a thread's stride, then a tree over the workgroup), so two solves return the same bits.  A row whose
// |r|^2 has reached its threshold is skipped by both steps: its alpha is 0 and it stops moving.  The _coef entries log the
// recurrence: with coef [2 iterations, S] non-NULL the update of iteration `it` leaves alpha_s in row 2 it and the direction
// after it beta_s in row 2 it + 1 (a skipped row leaves nothing: the host pre-fills the log) -- the Lanczos tridiagonal of
// the stochastic log-determinant (henbun_amd/gp/exact.py) at no extra product.  Nothing else changes with coef.
#define PCG_THREADS 1024

__device__ __forceinline__ double pcg_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();   // red may still be read from the sum before
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int o = PCG_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}

// out[s] = sum_i a_si b_si
template <typename T>
__global__ void __launch_bounds__(PCG_THREADS) pcg_dot_kernel(const T* a, const T* b, double* out, long N) {
  __shared__ double red[PCG_THREADS];
  const long base = (long)blockIdx.x * N;
  double acc = 0.0;
  for (long i = threadIdx.x; i < N; i += PCG_THREADS) acc = fma((double)a[base + i], (double)b[base + i], acc);
  const double tot = pcg_block_sum(acc, red);
  if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

// alpha = rz / (p . Ap);  x += alpha p;  r -= alpha Ap;  rr = |r|^2
template <typename T>
__global__ void __launch_bounds__(PCG_THREADS) pcg_update_kernel(T* x, T* r, const T* p, const T* Ap, const double* rz, double* rr,
                                                                 const double* thr, long N, double* coef, int it) {
  __shared__ double red[PCG_THREADS];
  const int s = blockIdx.x;
  if (!(rr[s] > thr[s])) return;   // converged: alpha = 0
  const long base = (long)s * N;
  double acc = 0.0;
  for (long i = threadIdx.x; i < N; i += PCG_THREADS) acc = fma((double)p[base + i], (double)Ap[base + i], acc);
  const double pAp = pcg_block_sum(acc, red);
  const double alpha = pAp > 0.0 ? rz[s] / pAp : 0.0;   // a direction of no curvature moves nothing
  if (coef && threadIdx.x == 0) coef[(2L * it) * gridDim.x + s] = alpha;
  acc = 0.0;
  for (long i = threadIdx.x; i < N; i += PCG_THREADS) {
    const double rn = fma(-alpha, (double)Ap[base + i], (double)r[base + i]);
    x[base + i] = (T)fma(alpha, (double)p[base + i], (double)x[base + i]);
    const T rt = (T)rn;
    r[base + i] = rt;
    acc = fma((double)rt, (double)rt, acc);
  }
  const double tot = pcg_block_sum(acc, red);
  if (threadIdx.x == 0) rr[s] = tot;
}

// z = (r - wscale w) zscale (w == NULL: z = r);  beta = (r . z) / rz (first: 0);  p = z + beta p;  rz = r . z
template <typename T>
__global__ void __launch_bounds__(PCG_THREADS) pcg_direction_kernel(const T* r, const T* w, T* p, double* rz, const double* rr,
                                                                    const double* thr, double wscale, double zscale, int first,
                                                                    long N, double* coef, int it) {
  __shared__ double red[PCG_THREADS];
  const int s = blockIdx.x;
  if (!(rr[s] > thr[s])) return;
  const long base = (long)s * N;
  auto zval = [&](long i) {
    const double rv = (double)r[base + i];
    return w ? fma(-wscale, (double)w[base + i], rv) * zscale : rv;
  };
  double acc = 0.0;
  for (long i = threadIdx.x; i < N; i += PCG_THREADS) acc = fma((double)r[base + i], zval(i), acc);
  const double rzn = pcg_block_sum(acc, red);
  const double rzo = rz[s];
  const double beta = (first || !(rzo > 0.0)) ? 0.0 : rzn / rzo;
  if (coef && threadIdx.x == 0) coef[(2L * it + 1) * gridDim.x + s] = beta;
  for (long i = threadIdx.x; i < N; i += PCG_THREADS) {
    const double pv = first ? 0.0 : (double)p[base + i];
    p[base + i] = (T)fma(beta, pv, zval(i));
  }
  __syncthreads();   // every thread has read rz[s]
  if (threadIdx.x == 0) rz[s] = rzn;
}

template <typename T>
static int pcg_dot(const T* a, const T* b, double* out, long S, long N, hipStream_t st) {
  HB_REQUIRE(S >= 1 && S <= 2147483647L && N >= 0, "hb_pcg_dot: bad extents (S=%ld N=%ld)", S, N);
  HB_REQUIRE(out && ((a && b) || N == 0), "hb_pcg_dot: NULL pointer");
  hipLaunchKernelGGL((pcg_dot_kernel<T>), dim3((unsigned)S), dim3(PCG_THREADS), 0, st, a, b, out, N);
  HB_LAUNCH_CHECK();
  return 0;
}
template <typename T>
static int pcg_update(T* x, T* r, const T* p, const T* Ap, const double* rz, double* rr, const double* thr, long S, long N,
                      double* coef, long it, hipStream_t st) {
  HB_REQUIRE(S >= 1 && S <= 2147483647L && N >= 1, "hb_pcg_update: bad extents (S=%ld N=%ld)", S, N);
  HB_REQUIRE(x && r && p && Ap && rz && rr && thr, "hb_pcg_update: NULL pointer");
  HB_REQUIRE(it >= 0 && it <= 1073741823L, "hb_pcg_update: bad iteration index (it=%ld)", it);
  hipLaunchKernelGGL((pcg_update_kernel<T>), dim3((unsigned)S), dim3(PCG_THREADS), 0, st, x, r, p, Ap, rz, rr, thr, N, coef,
                     (int)it);
  HB_LAUNCH_CHECK();
  return 0;
}
template <typename T>
static int pcg_direction(const T* r, const T* w, T* p, double* rz, const double* rr, const double* thr, double wscale,
                         double zscale, int first, long S, long N, double* coef, long it, hipStream_t st) {
  HB_REQUIRE(S >= 1 && S <= 2147483647L && N >= 1, "hb_pcg_direction: bad extents (S=%ld N=%ld)", S, N);
  HB_REQUIRE(r && p && rz && rr && thr, "hb_pcg_direction: NULL pointer");
  HB_REQUIRE(it >= 0 && it <= 1073741823L, "hb_pcg_direction: bad iteration index (it=%ld)", it);
  hipLaunchKernelGGL((pcg_direction_kernel<T>), dim3((unsigned)S), dim3(PCG_THREADS), 0, st, r, w, p, rz, rr, thr, wscale, zscale,
                     first, N, coef, (int)it);
  HB_LAUNCH_CHECK();
  return 0;
}

extern "C" int hb_pcg_dot_f32(const float* a, const float* b, double* out, long S, long N, void* stream) {
  return pcg_dot<float>(a, b, out, S, N, (hipStream_t)stream);
}
extern "C" int hb_pcg_dot_f64(const double* a, const double* b, double* out, long S, long N, void* stream) {
  return pcg_dot<double>(a, b, out, S, N, (hipStream_t)stream);
}
extern "C" int hb_pcg_update_f32(float* x, float* r, const float* p, const float* Ap, const double* rz, double* rr,
                                 const double* thr, long S, long N, void* stream) {
  return pcg_update<float>(x, r, p, Ap, rz, rr, thr, S, N, nullptr, 0, (hipStream_t)stream);
}
extern "C" int hb_pcg_update_f64(double* x, double* r, const double* p, const double* Ap, const double* rz, double* rr,
                                 const double* thr, long S, long N, void* stream) {
  return pcg_update<double>(x, r, p, Ap, rz, rr, thr, S, N, nullptr, 0, (hipStream_t)stream);
}
extern "C" int hb_pcg_direction_f32(const float* r, const float* w, float* p, double* rz, const double* rr, const double* thr,
                                    double wscale, double zscale, int first, long S, long N, void* stream) {
  return pcg_direction<float>(r, w, p, rz, rr, thr, wscale, zscale, first, S, N, nullptr, 0, (hipStream_t)stream);
}
extern "C" int hb_pcg_direction_f64(const double* r, const double* w, double* p, double* rz, const double* rr, const double* thr,
                                    double wscale, double zscale, int first, long S, long N, void* stream) {
  return pcg_direction<double>(r, w, p, rz, rr, thr, wscale, zscale, first, S, N, nullptr, 0, (hipStream_t)stream);
}
// the same steps with the recurrence coefficients logged: coef [2 iterations, S] double (NULL: exactly the entries above)
extern "C" int hb_pcg_update_coef_f32(float* x, float* r, const float* p, const float* Ap, const double* rz, double* rr,
                                      const double* thr, long S, long N, double* coef, long it, void* stream) {
  return pcg_update<float>(x, r, p, Ap, rz, rr, thr, S, N, coef, it, (hipStream_t)stream);
}
extern "C" int hb_pcg_update_coef_f64(double* x, double* r, const double* p, const double* Ap, const double* rz, double* rr,
                                      const double* thr, long S, long N, double* coef, long it, void* stream) {
  return pcg_update<double>(x, r, p, Ap, rz, rr, thr, S, N, coef, it, (hipStream_t)stream);
}
extern "C" int hb_pcg_direction_coef_f32(const float* r, const float* w, float* p, double* rz, const double* rr,
                                         const double* thr, double wscale, double zscale, int first, long S, long N,
                                         double* coef, long it, void* stream) {
  return pcg_direction<float>(r, w, p, rz, rr, thr, wscale, zscale, first, S, N, coef, it, (hipStream_t)stream);
}
extern "C" int hb_pcg_direction_coef_f64(const double* r, const double* w, double* p, double* rz, const double* rr,
                                         const double* thr, double wscale, double zscale, int first, long S, long N,
                                         double* coef, long it, void* stream) {
  return pcg_direction<double>(r, w, p, rz, rr, thr, wscale, zscale, first, S, N, coef, it, (hipStream_t)stream);
}
