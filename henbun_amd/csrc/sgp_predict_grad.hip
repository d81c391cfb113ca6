// Input gradients of the closed-form predictive moments and the closed-form acquisition functions built on them
// (hb_sgp_predict_grad_*, hb_sgp_acq_*, include/henbun_hip.h).  One expert, one latent function, UnitRBF.
//
// With K_kj = k(z_k, x_j), t_kjd = (z_kd - x_jd) / ell_d^2 (so dK_kj / dx_jd = K_kj t_kjd), A = W K and C = S^T A,
// hb_sgp_predict's mean_j = m A_j and var_j = ||C_j||^2 + r_j have the gradients
//     dmean_jd = sum_k alpha_k K_kj t_kjd                   alpha = W^T m^T
//     dvar_jd  = 2 sum_k G_kj K_kj t_kjd                    G = W^T V,  V = S C - A diag rho
//     rho_j = sign(1 - sum_m A_mj^2) (DIAGONAL), 0 (NEGLECTED), 1 (FULLRANK);  S C = s^2 o A for a mean-field S.
// Like the variance, its gradient is formed from A itself, never as a quadratic form in Kmm^-1.
//
// Fused form (the conditions of the fused predict kernel for E = P = 1: fp32, Wfrag, M % 32 == 0, 32 <= M <= 512,
// d <= 4): one workgroup owns a 32-column strip.  Phases 1-3 are those of hb_sgp_predict (csrc/sgp_predict.cuh: the same
// code, so mean and var are its bits), with the tiles of C kept in registers until the fold buffer of the variance has
// been read.  Then, in the two 32 x 516 LDS buffers of the predict kernel and no third:
//   4. C -> the dead K buffer;  V = S C - A diag rho  (lower-triangular strip product from a fragment-major image of S,
//      elementwise for a mean-field S) overwrites A tile by tile: a tile of A is read only by the wave that finishes
//      that tile of V
//   5. G = W^T V  (upper-triangular strip product from the W^T half of Wfrag) -> the K buffer
//   6. the fold sum_k (.) K_kj t_kjd with K re-synthesised by SgpStripColumn::value (one v_exp_f32 per entry, as in the
//      prologue), 16 threads per column in a fixed order; then the tail of the column in double.
// Steps 4-6 run only where a gradient is asked for: hb_sgp_acq with values or the arg-max alone costs what predict costs.
// No [M, n] intermediate reaches memory.  The only synchronisation is the workgroup barrier and the launch boundary in
// front of the arg-max fold: two runs return the same bits and a column's results do not depend on the other columns.
//
// General form (fp64, other M, d > 4, no Wfrag): columns in chunks; hb_sgp_A_* and hb_matmul_* form A, C, V, G of the
// chunk (V and G only where a gradient is asked for), the column-statistics kernel of hb_sgp_predict gives mean and var,
// one column kernel does the fold and the tail.  Parity, not speed.
//
// Acquisition tail, per point in double whatever the storage type (an fp32 u Phi(u) + phi(u) cancels for u < -5): with
// sc = scale, k_var = sc^2, s = +1 (largest) or -1:  mu' = s sc mean,  v = max(k_var var, var_floor),  sigma = sqrt(v),
// u = (mu' - s best - xi) / sigma,  Phi(u) = erfc(-u / sqrt 2) / 2:
//     EI  = sigma (u Phi + phi)   d/dmu' = Phi         d/dv = phi / (2 sigma)
//     PI  = Phi                   d/dmu' = phi / sigma d/dv = -u phi / (2 v)
//     UCB = mu' + beta sigma      d/dmu' = 1           d/dv = beta / (2 sigma)
//     grad_jd = s sc a_mu' dmean_jd + k_var a_v dvar_jd      (a_v = 0 where v was clamped)
// Arg-max: every workgroup leaves (value, column) of its columns in the workspace, a second launch folds them by the
// rule of hb_sgp_pathwise_argmax (pw_takes: strict comparisons, ties to the lowest column, a NaN never chosen).
#include "sgp_predict.cuh"
#include "sgp_pathwise.cuh"
#include "acq_tail.cuh"   // AcqTail, AcqPoint, acq_point, ACQ_NONE: shared with hb_gram_predict

#define ACQ_FUSED_CHUNK (1L << 20)    // columns per launch of the fused form (bounds the arg-max partials)
#define ACQ_COL_THREADS 256           // columns per workgroup of the general form's column kernel
#define ACQ_CHUNK_ELEMS (1L << 24)    // scratch of one chunk of the general form (elements, at most): A, C / G, V
#define ACQ_WS_HEAD 4                 // the arg-max carry: key at element 0, the column (long) 8 or 16 bytes further on

// d acq / d x_jd from the gradients of hb_sgp_predict's mean and var
__device__ __forceinline__ double acq_grad(const AcqTail& t, const AcqPoint& q, double dmean, double dvar) {
  return (t.largest ? t.scale : -t.scale) * q.a_mu * dmean + t.scale * t.scale * q.a_v * dvar;
}

template <typename T>
__device__ __forceinline__ T acq_rho(int mode, T sa2) {
  const T q = T(1) - sa2;
  return mode == HB_SGP_DIAGONAL ? (q > T(0) ? T(1) : q < T(0) ? T(-1) : T(0)) : mode == HB_SGP_FULLRANK ? T(1) : T(0);
}

// ------------------------------------------------------------------------------------------------ fused form
struct PredGradArgs {
  PredArgs p;          // one expert, P = 1; p.mean / p.var nullable
  const float* Sf;     // fragment-major image of S (full rank), or nullptr
  const float* alpha;  // [M] = W^T m^T
  float* dmean;        // [n, d], nullable together with dvar
  float* dvar;
  float* val;          // [n], nullable
  float* grad;         // [n, d], nullable
  float* part;         // arg-max partials: values [strips], then columns within the strip [strips]; nullable
  AcqTail t;
};

template <int D>
__global__ void __launch_bounds__(PRED_THREADS) sgp_predict_grad_strip_kernel(PredGradArgs ga) {
  typedef Mma<float>::Acc Acc;
  __shared__ __attribute__((aligned(16))) float Ks[SGP_SN * SGP_SLD];   // K; the C^2 fold buffer; C; G
  __shared__ __attribute__((aligned(16))) float As[SGP_SN * SGP_SLD];   // A_strip, then V, column-major
  __shared__ __attribute__((aligned(16))) float zs[SGP_SM_MAX * D];
  __shared__ float rho[SGP_SN];
  __shared__ float Rk[SGP_SN];
  __shared__ int Rj[SGP_SN];
  const PredArgs& a = ga.p;
  const int M = (int)a.M, n = (int)a.n, nT = M / 32;
  const int col0 = blockIdx.x * SGP_SN;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 31, h = lane >> 5;
  const int t1w = nT - 1 - w;   // the wave's tiles: w (when w < t1w) and t1w (when w <= t1w), as pred_strip_product takes them
  const bool fullS = a.STf != nullptr;

  // ---- phases 1-3; the wave's (at most two) tiles of C stay in registers: the fold buffer of phase 3 lives in Ks
  Acc c0, c1;
#pragma unroll
  for (int r = 0; r < 16; ++r) c0[r] = 0.f, c1[r] = 0.f;
  PredMoments o;
  pred_strip_moments<D>(a, Ks, As, zs, 0, o, [&](int tile, const Acc& acc) {
    if (tile == w && w < t1w)
      c0 = acc;
    else
      c1 = acc;
  });
  const int c = tid >> 4, g = tid & 15;
  const float mean = o.mu[0], var = o.var(fullS, 0, a.mode, a.jitter);
  // ---- phases 4-6 only where a gradient is asked for (workgroup-uniform): values and the arg-max need phases 1-3 alone
  const bool want_grad = ga.dmean != nullptr || ga.grad != nullptr;
  float dm[D], dv[D];
#pragma unroll
  for (int dd = 0; dd < D; ++dd) dm[dd] = 0.f, dv[dd] = 0.f;
  if (want_grad) {
    if (g == 0) rho[c] = acq_rho<float>(a.mode, o.sa2);
    __syncthreads();   // the fold buffer has been read: Ks is free; rho is visible

    // ---- phase 4: V = S C - A diag rho, in place of A
    if (fullS) {
      if (w < t1w) {
#pragma unroll
        for (int r = 0; r < 16; ++r) Ks[pred_acc_col(r, h) * SGP_SLD + 32 * w + li] = c0[r];
      }
      if (w <= t1w) {
#pragma unroll
        for (int r = 0; r < 16; ++r) Ks[pred_acc_col(r, h) * SGP_SLD + 32 * t1w + li] = c1[r];
      }
      __syncthreads();
      pred_strip_product<false>(ga.Sf, Ks, nT, w, lane, [&](int tile, const Acc& acc) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int cc = pred_acc_col(r, h), i = cc * SGP_SLD + 32 * tile + li;
          As[i] = acc[r] - rho[cc] * As[i];
        }
      });
    } else {
      const float rc = rho[c];
      for (int k = g; k < M; k += 16) {
        const float sv = a.s[k], av = As[c * SGP_SLD + k];
        As[c * SGP_SLD + k] = __builtin_fmaf(sv * sv, av, -(rc * av));
      }
    }
    __syncthreads();

    // ---- phase 5: G = W^T V -> Ks (C is dead since the barrier above)
    pred_strip_product<true>(a.Wf + a.M * a.M, As, nT, w, lane, [&](int tile, const Acc& acc) {
#pragma unroll
      for (int r = 0; r < 16; ++r) Ks[pred_acc_col(r, h) * SGP_SLD + 32 * tile + li] = acc[r];
    });
    __syncthreads();

    // ---- phase 6: the fold against dK; 16 threads per column, rows g, g + 16, ..., then the fixed-order tree of phase 2
    SgpStripColumn<D> cj;
    cj.load(a.x, a.ell, a.dl, col0, n, c);   // (the column is taken from the low five bits of the last argument)
    float il2[D];
#pragma unroll
    for (int dd = 0; dd < D; ++dd) {
      const float el = a.ell[a.dl == 1 ? 0 : dd];
      il2[dd] = 1.f / (el * el);
    }
    for (int k = g; k < M; k += 16) {
      const float kv = cj.value(&zs[k * D]);
      const float ak = ga.alpha[k] * kv, gk = Ks[c * SGP_SLD + k] * kv;
#pragma unroll
      for (int dd = 0; dd < D; ++dd) {
        const float tt = (zs[k * D + dd] - cj.xs[dd]) * il2[dd];
        dm[dd] = __builtin_fmaf(ak, tt, dm[dd]);
        dv[dd] = __builtin_fmaf(gk, tt, dv[dd]);
      }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
#pragma unroll
      for (int dd = 0; dd < D; ++dd) {
        dm[dd] += __shfl_xor(dm[dd], off, 16);
        dv[dd] += __shfl_xor(dv[dd], off, 16);
      }
    }
#pragma unroll
    for (int dd = 0; dd < D; ++dd) dv[dd] *= 2.f;
  }

  // ---- the column's stores and its tail
  const int j = col0 + c;
  const bool live = g == 0 && j < n;
  if (live) {
    if (a.mean) a.mean[j] = mean;
    if (a.var) a.var[j] = var;
    if (ga.dmean) {
#pragma unroll
      for (int dd = 0; dd < D; ++dd) ga.dmean[(long)j * D + dd] = dm[dd], ga.dvar[(long)j * D + dd] = dv[dd];
    }
  }
  if (ga.t.acq != ACQ_NONE) {
    float key = 0.f;
    int jl = -1;
    if (live) {
      const AcqPoint q = acq_point(ga.t, (double)mean, (double)var);
      key = (float)q.val;
      if (key == key) jl = c;
      if (ga.val) ga.val[j] = key;
      if (ga.grad) {
#pragma unroll
        for (int dd = 0; dd < D; ++dd) ga.grad[(long)j * D + dd] = (float)acq_grad(ga.t, q, (double)dm[dd], (double)dv[dd]);
      }
    }
    if (ga.part) {   // (uniform) the strip's best column: the 32 columns on the lower half of wave 0, a butterfly over them
      if (g == 0) Rk[c] = key, Rj[c] = jl;
      __syncthreads();
      if (w == 0) {
        float bk = Rk[li];
        int bj = Rj[li];
#pragma unroll
        for (int m = 1; m < SGP_SN; m <<= 1) {
          const float ok = __shfl_xor(bk, m);
          const int oj = __shfl_xor(bj, m);
          if (pw_takes<float>(ok, oj, bk, bj)) bk = ok, bj = oj;
        }
        if (tid == 0) {
          ga.part[blockIdx.x] = bk;
          ga.part[gridDim.x + blockIdx.x] = (float)bj;
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ shared small kernels
// alpha = W^T m^T  [M]: thread k sums rows k .. M - 1 of the lower-triangular W in double
template <typename T>
__global__ void __launch_bounds__(256) acq_alpha_kernel(const T* __restrict__ W, const T* __restrict__ m, T* __restrict__ alpha,
                                                        int M) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= M) return;
  double acc = 0.0;
  for (int i = k; i < M; ++i) acc = fma((double)W[(long)i * M + k], (double)m[i], acc);
  alpha[k] = (T)acc;
}

// One workgroup folds the partials of one launch (ns workgroups of cn columns, the first of them column j0) into the carry
// (ckey, cidx) of the launches before it; the last launch's fold also writes the results.  No comparable value at all:
// idx = -1 and best_val = -inf.
template <typename T>
__global__ void __launch_bounds__(256) acq_fold_kernel(const T* __restrict__ part, int ns, int cn, long j0, int first, int last,
                                                       T* __restrict__ ckey, long* __restrict__ cidx, T* __restrict__ best_val,
                                                       long* __restrict__ best_idx) {
  __shared__ T Rk[256];
  __shared__ long Rj[256];
  const int tid = threadIdx.x;
  T bk = -INFINITY;
  long bj = -1;
  for (int b = tid; b < ns; b += 256) {
    const T k = part[b];
    const int cl = (int)part[ns + b];
    const long j = cl < 0 ? -1 : j0 + (long)b * cn + cl;
    if (pw_takes<T>(k, j, bk, bj)) bk = k, bj = j;
  }
  Rk[tid] = bk, Rj[tid] = bj;
  __syncthreads();
  for (int m = 128; m > 0; m >>= 1) {
    if (tid < m && pw_takes<T>(Rk[tid + m], Rj[tid + m], Rk[tid], Rj[tid])) Rk[tid] = Rk[tid + m], Rj[tid] = Rj[tid + m];
    __syncthreads();
  }
  if (tid == 0) {
    bk = Rk[0], bj = Rj[0];
    if (!first && !pw_takes<T>(bk, bj, *ckey, *cidx)) bk = *ckey, bj = *cidx;
    *ckey = bk, *cidx = bj;
    if (last) {
      if (best_val) *best_val = bj < 0 ? (T)-INFINITY : bk;
      if (best_idx) *best_idx = bj;
    }
  }
}

// ------------------------------------------------------------------------------------------------ general form
// V of one chunk, [M, nc]: V = S C - A diag rho with S C already in V (full rank), or (s^2 - rho) o A (mean-field, s given)
template <typename T>
__global__ void __launch_bounds__(256) acq_v_kernel(const T* __restrict__ A, T* __restrict__ V, const T* __restrict__ s,
                                                    const T* __restrict__ sa2, int mode, long M, long nc) {
  const long total = M * nc, stride = (long)gridDim.x * blockDim.x;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const long k = t / nc, j = t - k * nc;
    const T rc = acq_rho<T>(mode, sa2[j]), av = A[t];
    V[t] = s ? fma(s[k] * s[k], av, -(rc * av)) : V[t] - rc * av;
  }
}

template <typename T>
struct AcqColArgs {
  const T* x;      // [nc, d]: the chunk's rows
  const T* z;      // [M, d]
  const T* ell;    // [dl]
  long dl;
  const T* alpha;  // [M]
  const T* G;      // [M, nc]
  const T* meanc;  // [nc] of the chunk (pred_colstat_kernel)
  const T* varc;
  T* mean;         // the chunk's part of every output; each nullable
  T* var;
  T* dmean;
  T* dvar;
  T* val;
  T* grad;
  T* part;         // arg-max partials [2 workgroups]
  AcqTail t;
  long nc, M, d;
};

// one thread per column of the chunk: the fold in k order, four input dimensions at a time, then the tail
template <typename T>
__global__ void __launch_bounds__(ACQ_COL_THREADS) acq_col_kernel(AcqColArgs<T> a) {
  __shared__ T Rk[ACQ_COL_THREADS];
  __shared__ int Rj[ACQ_COL_THREADS];
  const int tid = threadIdx.x;
  const long j = (long)blockIdx.x * ACQ_COL_THREADS + tid, nc = a.nc, M = a.M, d = a.d;
  T key = T(0);
  int jl = -1;
  if (j < nc) {
    const T mean = a.meanc[j], var = a.varc[j];
    if (a.mean) a.mean[j] = mean;
    if (a.var) a.var[j] = var;
    AcqPoint q;
    q.val = q.a_mu = q.a_v = 0.0;
    if (a.t.acq != ACQ_NONE) {
      q = acq_point(a.t, (double)mean, (double)var);
      key = (T)q.val;
      if (key == key) jl = tid;
      if (a.val) a.val[j] = key;
    }
    if (a.dmean || a.grad) {
      const T* __restrict__ xj = a.x + j * d;
      for (long d0 = 0; d0 < d; d0 += 4) {
        T dm[4], dv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) dm[i] = T(0), dv[i] = T(0);
        for (long k = 0; k < M; ++k) {
          const T* __restrict__ zk = a.z + k * d;
          T r2 = T(0);
          for (long dd = 0; dd < d; ++dd) {
            const T tt = (zk[dd] - xj[dd]) * (T(SGP_EXP2_SCALE) / a.ell[a.dl == 1 ? 0 : dd]);
            r2 += tt * tt;
          }
          const T kv = hb_exp2_neg<T>(r2);
          const T ak = a.alpha[k] * kv, gk = a.G[k * nc + j] * kv;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (d0 + i < d) {
              const T el = a.ell[a.dl == 1 ? 0 : d0 + i];
              const T tt = (zk[d0 + i] - xj[d0 + i]) / (el * el);
              dm[i] += ak * tt;
              dv[i] += gk * tt;
            }
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (d0 + i < d) {
            const long o = j * d + d0 + i;
            const T dvv = T(2) * dv[i];
            if (a.dmean) a.dmean[o] = dm[i], a.dvar[o] = dvv;
            if (a.grad) a.grad[o] = (T)acq_grad(a.t, q, (double)dm[i], (double)dvv);
          }
        }
      }
    }
  }
  if (a.part) {   // (uniform)
    Rk[tid] = key, Rj[tid] = jl;
    __syncthreads();
    for (int m = ACQ_COL_THREADS / 2; m > 0; m >>= 1) {
      if (tid < m && pw_takes<T>(Rk[tid + m], Rj[tid + m], Rk[tid], Rj[tid])) Rk[tid] = Rk[tid + m], Rj[tid] = Rj[tid + m];
      __syncthreads();
    }
    if (tid == 0) {
      a.part[blockIdx.x] = Rk[0];
      a.part[gridDim.x + blockIdx.x] = (T)Rj[0];
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
static inline long acq_chunk_cols(long n, long M) { return hb_chunk_cols(ACQ_CHUNK_ELEMS, 3 * M, HB_PRED_CHUNK, n); }   // M >= 1
static inline long acq_ws_base(long M) { return ACQ_WS_HEAD + ((M + 3) & ~3L); }   // carry, alpha

static long acq_ws_elems(long n, long M, long d, int s_kind, int has_wfrag, int dtype_bytes) {
  if (n <= 0 || M <= 0 || d <= 0) return 0;
  if (pred_is_fused(1, n, M, d, 1, s_kind, has_wfrag != 0, dtype_bytes)) {
    const long nc = n < ACQ_FUSED_CHUNK ? n : ACQ_FUSED_CHUNK;
    return acq_ws_base(M) + (s_kind == HB_SGP_S_TRIL ? 2 * M * M : 0) + 2 * (long)hb_cdiv(nc, SGP_SN);
  }
  const long nc = acq_chunk_cols(n, M);
  return acq_ws_base(M) + nc * (3 * M + 3) + 2 * (long)hb_cdiv(nc, ACQ_COL_THREADS);
}
extern "C" long hb_sgp_predict_grad_ws_elems(long n, long M, long d, int s_kind, int has_wfrag, int dtype_bytes) {
  return acq_ws_elems(n, M, d, s_kind, has_wfrag, dtype_bytes);
}
extern "C" long hb_sgp_acq_ws_elems(long n, long M, long d, int s_kind, int has_wfrag, int dtype_bytes) {
  return acq_ws_elems(n, M, d, s_kind, has_wfrag, dtype_bytes);
}

static void acq_fused_launch(const PredGradArgs& a, long d, hipStream_t st) {
  const dim3 grid((unsigned)hb_cdiv(a.p.n, SGP_SN), 1, 1);
  if (d == 1)
    hipLaunchKernelGGL((sgp_predict_grad_strip_kernel<1>), grid, dim3(PRED_THREADS), 0, st, a);
  else if (d == 2)
    hipLaunchKernelGGL((sgp_predict_grad_strip_kernel<2>), grid, dim3(PRED_THREADS), 0, st, a);
  else if (d == 3)
    hipLaunchKernelGGL((sgp_predict_grad_strip_kernel<3>), grid, dim3(PRED_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL((sgp_predict_grad_strip_kernel<4>), grid, dim3(PRED_THREADS), 0, st, a);
}

template <typename T>
struct AcqOut {
  T* mean;
  T* var;
  T* dmean;
  T* dvar;
  T* val;
  T* grad;
  T* best_val;
  long* best_idx;
};
template <typename T>
static inline T* acq_at(T* p, long off) { return p ? p + off : nullptr; }

// both entries: every check, then alpha and the images (one launch each), then the columns in chunks
template <typename T>
static int sgp_acq_run(const char* who, int kind, const T* x, const T* z, const T* ell, long dl, const T* W, const T* Wf,
                       const T* m, const T* s, int s_kind, int mode, double jitter, const AcqTail& t, const AcqOut<T>& out,
                       long n, long M, long d, T* ws, hipStream_t st) {
  HB_REQUIRE(mode == HB_SGP_NEGLECTED || mode == HB_SGP_DIAGONAL || mode == HB_SGP_FULLRANK, "%s: unknown residual mode %d", who,
             mode);
  HB_REQUIRE(s_kind == HB_SGP_S_DIAG || s_kind == HB_SGP_S_TRIL, "%s: unknown s_kind %d", who, s_kind);
  HB_REQUIRE(n >= 0 && M >= 1 && d >= 1, "%s: bad extents (n=%ld M=%ld d=%ld)", who, n, M, d);
  HB_REQUIRE(x && z && ell && W && m && s, "%s: NULL pointer", who);
  HB_REQUIRE(n < 2147483647L && d < 2147483647L && n * d < 2147483647L, "%s: matrix too large", who);
  HB_REQUIRE_RBF_MODEL(who, "has a closed-form predictive", kind, dl, d, Wf, M);
  const bool amax = out.best_val || out.best_idx;
  if (t.acq == ACQ_NONE) {
    HB_REQUIRE(out.dmean && out.dvar, "%s: dmean and dvar must be given", who);
  } else {
    HB_REQUIRE(t.acq == HB_ACQ_EI || t.acq == HB_ACQ_PI || t.acq == HB_ACQ_UCB, "%s: unknown acquisition %d", who, t.acq);
    HB_REQUIRE(out.val || out.grad || amax, "%s: at least one of val, grad, best_val, best_idx must be given", who);
    HB_REQUIRE(t.scale > 0.0 && t.var_floor >= 0.0 && t.best == t.best && t.param == t.param,
               "%s: scale > 0, var_floor >= 0 and numbers for best and param expected (scale=%g var_floor=%g best=%g param=%g)",
               who, t.scale, t.var_floor, t.best, t.param);
    HB_REQUIRE(!amax || n >= 1, "%s: an arg-max needs at least one candidate (n=%ld)", who, n);
  }
  if (n == 0) return 0;
  const long need = acq_ws_elems(n, M, d, s_kind, Wf != nullptr, (int)sizeof(T));
  HB_REQUIRE(ws && (uintptr_t)ws % 16 == 0, "%s: needs a 16-byte aligned workspace of %ld elements", who, need);

  T* ckey = ws;
  long* cidx = reinterpret_cast<long*>(ws + 2);
  T* alpha = ws + ACQ_WS_HEAD;
  T* base = ws + acq_ws_base(M);
  const bool want_grad = out.dmean || out.grad;   // values and the arg-max alone need neither alpha nor V, G
  if (want_grad) {
    hipLaunchKernelGGL((acq_alpha_kernel<T>), dim3(hb_cdiv(M, 256)), dim3(256), 0, st, W, m, alpha, (int)M);
    HB_LAUNCH_CHECK();
  }
  const bool tril = s_kind == HB_SGP_S_TRIL;

  if constexpr (sizeof(T) == 4) {
    if (pred_is_fused(1, n, M, d, 1, s_kind, Wf != nullptr, 4)) {
      float* STf = tril ? base : nullptr;
      float* Sf = tril ? base + M * M : nullptr;
      float* part = amax ? base + (tril ? 2 * M * M : 0) : nullptr;
      if (tril) {
        hipLaunchKernelGGL(pred_s_image_kernel<true>, dim3(hb_stream_grid(M * M, 256)), dim3(256), 0, st, s, STf, M);
        HB_LAUNCH_CHECK();
        if (want_grad) {
          hipLaunchKernelGGL(pred_s_image_kernel<false>, dim3(hb_stream_grid(M * M, 256)), dim3(256), 0, st, s, Sf, M);
          HB_LAUNCH_CHECK();
        }
      }
      for (long j0 = 0; j0 < n; j0 += ACQ_FUSED_CHUNK) {
        const long nc = n - j0 < ACQ_FUSED_CHUNK ? n - j0 : ACQ_FUSED_CHUNK;
        PredGradArgs a;
        a.p.x = x + j0 * d; a.p.sx = 0; a.p.z = z; a.p.ell = ell; a.p.dl = dl; a.p.Wf = Wf; a.p.STf = STf; a.p.m = m;
        a.p.s = tril ? nullptr : s;
        a.p.mode = mode; a.p.jitter = (float)jitter; a.p.mean = acq_at(out.mean, j0); a.p.var = acq_at(out.var, j0);
        a.p.n = nc; a.p.M = M; a.p.P = 1;
        a.Sf = Sf; a.alpha = alpha; a.dmean = acq_at(out.dmean, j0 * d); a.dvar = acq_at(out.dvar, j0 * d);
        a.val = acq_at(out.val, j0); a.grad = acq_at(out.grad, j0 * d); a.part = part; a.t = t;
        acq_fused_launch(a, d, st);
        HB_LAUNCH_CHECK();
        if (amax) {
          hipLaunchKernelGGL((acq_fold_kernel<float>), dim3(1), dim3(256), 0, st, (const float*)part, hb_cdiv(nc, SGP_SN), SGP_SN,
                             j0, j0 == 0, j0 + nc >= n, ckey, cidx, out.best_val, out.best_idx);
          HB_LAUNCH_CHECK();
        }
      }
      return 0;
    }
  }

  const long nc_max = acq_chunk_cols(n, M);
  T* Abuf = base;
  T* Cbuf = Abuf + M * nc_max;   // C, then G
  T* Vbuf = Cbuf + M * nc_max;
  T* meanc = Vbuf + M * nc_max;
  T* varc = meanc + nc_max;
  T* sa2c = varc + nc_max;
  T* part = amax ? sa2c + nc_max : nullptr;
  for (long j0 = 0; j0 < n; j0 += nc_max) {
    const long nc = n - j0 < nc_max ? n - j0 : nc_max;
    int rc = hb_sgp_A(kind, x + j0 * d, 0, z, ell, dl, W, Wf, Abuf, 1, nc, M, d, st);
    if (rc) return rc;
    if (tril) {   // C = S^T A
      rc = hb_matmul(s, Abuf, Cbuf, 1, M, nc, M, M, nc, nc, 0, 0, 0, 1, st);
      if (rc) return rc;
    }
    hipLaunchKernelGGL((pred_colstat_kernel<T>), dim3(hb_stream_grid(nc, 256)), dim3(256), 0, st, (const T*)Abuf,
                       (const T*)(tril ? Cbuf : nullptr), m, s, mode, (T)jitter, meanc, varc, sa2c, 1L, 1L, M, M, nc, nc, 0L);
    HB_LAUNCH_CHECK();
    if (want_grad) {
      if (tril) {   // S C
        rc = hb_matmul(s, Cbuf, Vbuf, 1, M, nc, M, M, nc, nc, 0, 0, 0, 0, st);
        if (rc) return rc;
      }
      hipLaunchKernelGGL((acq_v_kernel<T>), dim3(hb_stream_grid(M * nc, 256)), dim3(256), 0, st, (const T*)Abuf, Vbuf,
                         tril ? (const T*)nullptr : s, (const T*)sa2c, mode, M, nc);
      HB_LAUNCH_CHECK();
      rc = hb_matmul(W, Vbuf, Cbuf, 1, M, nc, M, M, nc, nc, 0, 0, 0, 1, st);   // G = W^T V
      if (rc) return rc;
    }
    AcqColArgs<T> a;
    a.x = x + j0 * d; a.z = z; a.ell = ell; a.dl = dl; a.alpha = alpha; a.G = Cbuf; a.meanc = meanc; a.varc = varc;
    a.mean = acq_at(out.mean, j0); a.var = acq_at(out.var, j0); a.dmean = acq_at(out.dmean, j0 * d);
    a.dvar = acq_at(out.dvar, j0 * d); a.val = acq_at(out.val, j0); a.grad = acq_at(out.grad, j0 * d); a.part = part; a.t = t;
    a.nc = nc; a.M = M; a.d = d;
    const int nb = hb_cdiv(nc, ACQ_COL_THREADS);
    hipLaunchKernelGGL((acq_col_kernel<T>), dim3(nb), dim3(ACQ_COL_THREADS), 0, st, a);
    HB_LAUNCH_CHECK();
    if (amax) {
      hipLaunchKernelGGL((acq_fold_kernel<T>), dim3(1), dim3(256), 0, st, (const T*)part, nb, ACQ_COL_THREADS, j0, j0 == 0,
                         j0 + nc >= n, ckey, cidx, out.best_val, out.best_idx);
      HB_LAUNCH_CHECK();
    }
  }
  return 0;
}

template <typename T>
static int sgp_predict_grad(int kind, const T* x, const T* z, const T* ell, long dl, const T* W, const T* Wf, const T* m,
                            const T* s, int s_kind, int mode, double jitter, T* mean, T* var, T* dmean, T* dvar, long n, long M,
                            long d, T* ws, hipStream_t st) {
  AcqTail t;
  t.acq = ACQ_NONE; t.largest = 1; t.best = t.param = t.var_floor = 0.0; t.scale = 1.0;
  AcqOut<T> o;
  o.mean = mean; o.var = var; o.dmean = dmean; o.dvar = dvar; o.val = o.grad = o.best_val = nullptr; o.best_idx = nullptr;
  return sgp_acq_run<T>("hb_sgp_predict_grad", kind, x, z, ell, dl, W, Wf, m, s, s_kind, mode, jitter, t, o, n, M, d, ws, st);
}
template <typename T>
static int sgp_acq(int kind, const T* x, const T* z, const T* ell, long dl, const T* W, const T* Wf, const T* m, const T* s,
                   int s_kind, int mode, double jitter, int acq, double best, double param, double scale, int largest,
                   double var_floor, T* val, T* grad, T* best_val, long* best_idx, long n, long M, long d, T* ws,
                   hipStream_t st) {
  AcqTail t;
  t.acq = acq; t.largest = largest != 0; t.best = best; t.param = param; t.scale = scale; t.var_floor = var_floor;
  HB_REQUIRE(acq != ACQ_NONE, "hb_sgp_acq: unknown acquisition %d", acq);
  AcqOut<T> o;
  o.mean = o.var = o.dmean = o.dvar = nullptr; o.val = val; o.grad = grad; o.best_val = best_val; o.best_idx = best_idx;
  return sgp_acq_run<T>("hb_sgp_acq", kind, x, z, ell, dl, W, Wf, m, s, s_kind, mode, jitter, t, o, n, M, d, ws, st);
}

extern "C" int hb_sgp_predict_grad_f32(int kind, const float* x, const float* z, const float* ell, long dl, const float* W,
                                       const float* Wfrag, const float* m, const float* s, int s_kind, int mode, double jitter,
                                       float* mean, float* var, float* dmean, float* dvar, long n, long M, long d, float* ws,
                                       void* stream) {
  return sgp_predict_grad<float>(kind, x, z, ell, dl, W, Wfrag, m, s, s_kind, mode, jitter, mean, var, dmean, dvar, n, M, d, ws,
                                 (hipStream_t)stream);
}
extern "C" int hb_sgp_predict_grad_f64(int kind, const double* x, const double* z, const double* ell, long dl, const double* W,
                                       const double* Wfrag, const double* m, const double* s, int s_kind, int mode,
                                       double jitter, double* mean, double* var, double* dmean, double* dvar, long n, long M,
                                       long d, double* ws, void* stream) {
  return sgp_predict_grad<double>(kind, x, z, ell, dl, W, Wfrag, m, s, s_kind, mode, jitter, mean, var, dmean, dvar, n, M, d, ws,
                                  (hipStream_t)stream);
}
extern "C" int hb_sgp_acq_f32(int kind, const float* x, const float* z, const float* ell, long dl, const float* W,
                              const float* Wfrag, const float* m, const float* s, int s_kind, int mode, double jitter, int acq,
                              double best, double param, double scale, int largest, double var_floor, float* val, float* grad,
                              float* best_val, long* best_idx, long n, long M, long d, float* ws, void* stream) {
  return sgp_acq<float>(kind, x, z, ell, dl, W, Wfrag, m, s, s_kind, mode, jitter, acq, best, param, scale, largest, var_floor,
                        val, grad, best_val, best_idx, n, M, d, ws, (hipStream_t)stream);
}
extern "C" int hb_sgp_acq_f64(int kind, const double* x, const double* z, const double* ell, long dl, const double* W,
                              const double* Wfrag, const double* m, const double* s, int s_kind, int mode, double jitter, int acq,
                              double best, double param, double scale, int largest, double var_floor, double* val, double* grad,
                              double* best_val, long* best_idx, long n, long M, long d, double* ws, void* stream) {
  return sgp_acq<double>(kind, x, z, ell, dl, W, Wfrag, m, s, s_kind, mode, jitter, acq, best, param, scale, largest, var_floor,
                         val, grad, best_val, best_idx, n, M, d, ws, (hipStream_t)stream);
}
