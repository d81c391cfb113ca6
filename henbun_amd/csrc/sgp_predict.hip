// Closed-form predictive moments of SparseGP.samples (hb_sgp_predict_*, include/henbun_hip.h).
//
// samples() draws f = u^T A + residual with A = L^-1 K(z, x), u ~ N(m, S S^T) and L = chol(Kmm + jitter I)
// (reference gp/gp.py:99-143).  Its first two moments per column j are
//     mean_pj = m_p^T A_j
//     var_pj  = || S_p^T A_j ||^2 + r_j,   r_j = |1 - sum_m A_mj^2|  (DIAGONAL),  0  (NEGLECTED),
//                                          1 - sum_m A_mj^2 + jitter  (FULLRANK: the diagonal samples() factorises)
// The variance is formed from A itself: a quadratic form in Kmm^-1 cancels catastrophically in fp32 at cond(Kmm) ~ 1e5.
//
// Fused form (fp32, UnitRBF, M % 32 == 0, 32 <= M <= 512, d <= 4, P <= 4; full-rank S only for E P == 1): one workgroup
// owns a 32-column strip across all M rows.  It synthesises K(z, x_strip) in LDS (as the column-strip kernels of
// csrc/sgp.hip do), forms A_strip on MFMA from the fragment-major W image of the factorisation, stages A_strip in LDS
// (at most 64 KB) and finishes every column statistic inside the workgroup; for a full-rank S it also forms
// C = S^T A_strip on MFMA from a fragment-major image of S^T (upper triangular: its zero tiles are skipped).  A is never
// written to memory; the only scratch is the S^T image (M^2 elements).
//
// Chunked form (everything else the UnitRBF kernel takes: fp64, M > 512, d > 4, P > 4, full-rank S with E P > 1, or no
// Wfrag): columns in chunks of at most HB_PRED_CHUNK columns -- hb_sgp_A_* builds A of the chunk, hb_matmul_* forms
// S_ep^T A_e (full rank), one column-statistics kernel reduces them.  Scratch is bounded by the chunk, not by n.
//
// Multi-latent form (hb_sgp_predict_multi_*): C latent functions of ONE expert with independent full-rank q(u_c) that share
// x, z, ell and W.  A does not depend on the latent function, so the fused kernel forms A_strip once and runs phase 2 per
// group of PRED_PMAX means and phase 3 once per latent function against that function's S^T image: C + 1 strip products
// where C calls of the one-latent kernel take 2 C.  Every phase is the one-latent kernel's code (csrc/sgp_predict.cuh), so
// the moments are the bits of C calls of hb_sgp_predict_f32(HB_SGP_S_TRIL, P = 1).  Other shapes loop the chunked form.
#include "sgp_predict.cuh"

// One workgroup = 32 columns of one expert (blockIdx.x = strip, blockIdx.y = expert): phases 1-3 of csrc/sgp_predict.cuh,
// then the store of every latent function's mean and variance.
template <int D>
__global__ void __launch_bounds__(PRED_THREADS) sgp_predict_strip_kernel(PredArgs a) {
  __shared__ __attribute__((aligned(16))) float Ks[SGP_SN * SGP_SLD];   // K block; after phase 1 the C^2 fold buffer
  __shared__ __attribute__((aligned(16))) float As[SGP_SN * SGP_SLD];   // A_strip, column-major
  __shared__ __attribute__((aligned(16))) float zs[SGP_SM_MAX * D];
  const long e = blockIdx.y;
  PredMoments o;
  pred_strip_moments<D>(a, Ks, As, zs, e, o, [](int, const Mma<float>::Acc&) {});
  const int tid = threadIdx.x, c = tid >> 4, g = tid & 15, P = (int)a.P;
  const int j = blockIdx.x * SGP_SN + c;
  if (g == 0 && j < (int)a.n) {
#pragma unroll
    for (int p = 0; p < PRED_PMAX; ++p) {
      if (p < P) {
        const long q = (e * a.P + p) * a.n + j;
        a.mean[q] = o.mu[p];
        a.var[q] = o.var(a.STf != nullptr, p, a.mode, a.jitter);
      }
    }
  }
}

// The multi-latent strip kernel: one workgroup = 32 columns; a.m [C, M], a.STf C images M^2 apart, a.mean / a.var [C, n].
// Nothing per latent function lives in registers past its own trip: the means are stored group by group, the variances
// latent by latent; only sum A^2 (the residual) is carried.  The fold buffer overlays the dead K block and is reused by
// every latent function: a barrier stands between one function's fold and the next function's partials.
template <int D>
__global__ void __launch_bounds__(PRED_THREADS) sgp_predict_multi_strip_kernel(PredArgs a, int C) {
  __shared__ __attribute__((aligned(16))) float Ks[SGP_SN * SGP_SLD];   // K block; after phase 1 the C^2 fold buffer
  __shared__ __attribute__((aligned(16))) float As[SGP_SN * SGP_SLD];   // A_strip, column-major
  __shared__ __attribute__((aligned(16))) float zs[SGP_SM_MAX * D];
  pred_strip_A<D>(a, Ks, As, zs, 0);
  const int M = (int)a.M, nT = M / 32;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), c = tid >> 4, g = tid & 15;
  const int j = blockIdx.x * SGP_SN + c;
  const bool store = g == 0 && j < (int)a.n;
  float sa2 = 0.f;
#pragma nounroll
  for (int c0 = 0; c0 < C; c0 += PRED_PMAX) {
    const int P = C - c0 < PRED_PMAX ? C - c0 : PRED_PMAX;
    float s2, mu[PRED_PMAX], ss[PRED_PMAX];
    pred_strip_colsums(As, a.m + (long)c0 * M, nullptr, M, P, c, g, s2, mu, ss);
    sa2 = pred_col_tree(s2);   // (the same sum in every group)
#pragma unroll
    for (int p = 0; p < PRED_PMAX; ++p) {
      const float v = pred_col_tree(mu[p]);
      if (store && p < P) a.mean[(long)(c0 + p) * a.n + j] = v;
    }
  }
  const float res = pred_residual<float>(a.mode, sa2, a.jitter);
#pragma nounroll
  for (int l = 0; l < C; ++l) {
    if (l > 0) __syncthreads();   // every thread has read latent l - 1's partials out of the fold buffer
    pred_strip_c2(a.STf + (long)l * M * M, As, Ks, nT, w, lane, [](int, const Mma<float>::Acc&) {});
    __syncthreads();              // every wave's C^2 partials are in the fold buffer
    const float csum = pred_col_tree(pred_strip_c2_fold(Ks, c, g));
    if (store) a.var[(long)l * a.n + j] = csum + res;
  }
}

static inline long pred_chunk_cols(long E, long n, long M, long P, int s_kind) {
  const long per_col = E * M + (s_kind == HB_SGP_S_TRIL ? E * P * (E * P * M) : 0);
  return hb_chunk_cols(HB_PRED_CHUNK_ELEMS, per_col, HB_PRED_CHUNK, n);
}

extern "C" int hb_sgp_predict_fused(long E, long n, long M, long d, long P, int s_kind, int has_wfrag, int dtype_bytes) {
  return pred_is_fused(E, n, M, d, P, s_kind, has_wfrag != 0, dtype_bytes) ? 1 : 0;
}
extern "C" long hb_sgp_predict_ws_elems(long E, long n, long M, long d, long P, int s_kind, int has_wfrag, int dtype_bytes) {
  if (E <= 0 || n <= 0 || M <= 0 || P <= 0) return 0;
  if (pred_is_fused(E, n, M, d, P, s_kind, has_wfrag != 0, dtype_bytes)) return s_kind == HB_SGP_S_TRIL ? M * M : 0;
  const long nc = pred_chunk_cols(E, n, M, P, s_kind);
  return nc * (E * M + (s_kind == HB_SGP_S_TRIL ? E * P * (E * P * M) : 0));
}

static int pred_fused_launch(const PredArgs& a, long E, long d, hipStream_t st) {
  const dim3 grid((unsigned)hb_cdiv(a.n, SGP_SN), (unsigned)E, 1);
  if (d == 1)
    hipLaunchKernelGGL((sgp_predict_strip_kernel<1>), grid, dim3(PRED_THREADS), 0, st, a);
  else if (d == 2)
    hipLaunchKernelGGL((sgp_predict_strip_kernel<2>), grid, dim3(PRED_THREADS), 0, st, a);
  else if (d == 3)
    hipLaunchKernelGGL((sgp_predict_strip_kernel<3>), grid, dim3(PRED_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL((sgp_predict_strip_kernel<4>), grid, dim3(PRED_THREADS), 0, st, a);
  HB_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int sgp_predict(int kind, const T* x, long sx, const T* z, const T* ell, long dl, const T* W, const T* Wf, const T* m,
                       const T* s, int s_kind, int mode, double jitter, T* mean, T* var, long E, long n, long M, long d, long P,
                       T* ws, hipStream_t st) {
  HB_REQUIRE(mode == HB_SGP_NEGLECTED || mode == HB_SGP_DIAGONAL || mode == HB_SGP_FULLRANK,
             "hb_sgp_predict: unknown residual mode %d", mode);
  HB_REQUIRE(s_kind == HB_SGP_S_DIAG || s_kind == HB_SGP_S_TRIL, "hb_sgp_predict: unknown s_kind %d", s_kind);
  HB_REQUIRE(E >= 1 && n >= 0 && M >= 1 && d >= 1 && P >= 1, "hb_sgp_predict: bad extents (E=%ld n=%ld M=%ld d=%ld P=%ld)",
             E, n, M, d, P);
  HB_REQUIRE(sx == 0 || sx == n * d, "hb_sgp_predict: x is shared (sx = 0) or [E, n, d] (sx = n d), got sx=%ld", sx);
  HB_REQUIRE(x && z && ell && W && m && s && mean && var, "hb_sgp_predict: NULL pointer");
  HB_REQUIRE(E <= 65535, "hb_sgp_predict: too many experts");
  const long R = E * P * M;
  HB_REQUIRE(n * d < 2147483647L && (s_kind == HB_SGP_S_DIAG || R * R < 2147483647L),
             "hb_sgp_predict: matrix too large");
  HB_REQUIRE_RBF_MODEL("hb_sgp_predict", "has a closed-form predictive", kind, dl, d, Wf, M);
  if (n == 0) return 0;
  const bool fused = pred_is_fused(E, n, M, d, P, s_kind, Wf != nullptr, (int)sizeof(T));
  const long need = hb_sgp_predict_ws_elems(E, n, M, d, P, s_kind, Wf != nullptr, (int)sizeof(T));
  HB_REQUIRE(need == 0 || (ws && (uintptr_t)ws % 16 == 0), "hb_sgp_predict: needs a 16-byte aligned workspace of %ld elements",
             need);
  if constexpr (sizeof(T) == 4) {
    if (fused) {
      PredArgs a;
      a.x = x; a.sx = sx; a.z = z; a.ell = ell; a.dl = dl; a.Wf = Wf;
      a.STf = s_kind == HB_SGP_S_TRIL ? ws : nullptr;
      a.m = m; a.s = s_kind == HB_SGP_S_DIAG ? s : nullptr;
      a.mode = mode; a.jitter = (float)jitter; a.mean = mean; a.var = var; a.n = n; a.M = M; a.P = P;
      if (a.STf) {
        hipLaunchKernelGGL(pred_s_image_kernel<true>, dim3(hb_stream_grid(M * M, 256)), dim3(256), 0, st, s, ws, M);
        HB_LAUNCH_CHECK();
      }
      return pred_fused_launch(a, E, d, st);
    }
  }
  // chunked form
  const long nc_max = pred_chunk_cols(E, n, M, P, s_kind);
  T* Abuf = ws;
  T* Cbuf = s_kind == HB_SGP_S_TRIL ? ws + nc_max * E * M : nullptr;
  for (long j0 = 0; j0 < n; j0 += nc_max) {
    const long nc = n - j0 < nc_max ? n - j0 : nc_max;
    int rc = hb_sgp_A(kind, x + j0 * d, sx, z, ell, dl, W, Wf, Abuf, E, nc, M, d, st);
    if (rc) return rc;
    if (Cbuf) {
      // C_ep = S_ep^T A_e: op(A) of the product is the [M, R] row block of S transposed
      for (long e = 0; e < E; ++e) {
        rc = hb_matmul(s + e * P * M * R, Abuf + e * M * nc, Cbuf + e * P * R * nc, P, R, nc, M, R, nc, nc, M * R, 0, R * nc, 1, st);
        if (rc) return rc;
      }
    }
    hipLaunchKernelGGL((pred_colstat_kernel<T>), dim3(hb_stream_grid(E * P * nc, 256)), dim3(256), 0, st, Abuf, Cbuf, m, s, mode,
                       (T)jitter, mean, var, (T*)nullptr, E, P, M, R, nc, n, j0);
    HB_LAUNCH_CHECK();
  }
  return 0;
}

// ---- C latent functions of one expert, independent full-rank q(u_c) (hb_sgp_predict_multi_*)
static inline bool pred_multi_is_fused(long n, long M, long d, long C, bool has_wfrag, int dbytes) {
  return C >= 1 && C <= HB_PRED_MULTI_CMAX && pred_is_fused(1, n, M, d, 1, HB_SGP_S_TRIL, has_wfrag, dbytes);
}
extern "C" int hb_sgp_predict_multi_fused(long n, long M, long d, long C, int has_wfrag, int dtype_bytes) {
  return pred_multi_is_fused(n, M, d, C, has_wfrag != 0, dtype_bytes) ? 1 : 0;
}
extern "C" long hb_sgp_predict_multi_ws_elems(long n, long M, long d, long C, int has_wfrag, int dtype_bytes) {
  if (n <= 0 || M <= 0 || C <= 0) return 0;
  if (pred_multi_is_fused(n, M, d, C, has_wfrag != 0, dtype_bytes)) return C * M * M;
  return hb_sgp_predict_ws_elems(1, n, M, d, 1, HB_SGP_S_TRIL, has_wfrag, dtype_bytes);
}

template <typename T>
static int sgp_predict_multi(int kind, const T* x, const T* z, const T* ell, long dl, const T* W, const T* Wf, const T* m,
                             const T* S, int mode, T* mean, T* var, long n, long M, long d, long C, T* ws, hipStream_t st) {
  HB_REQUIRE(mode == HB_SGP_NEGLECTED || mode == HB_SGP_DIAGONAL,
             "hb_sgp_predict_multi: the residual mode must be HB_SGP_NEGLECTED or HB_SGP_DIAGONAL (got %d)", mode);
  HB_REQUIRE(C >= 1 && C <= HB_PRED_MULTI_CMAX, "hb_sgp_predict_multi: 1 <= C <= %d latent functions expected (C=%ld)",
             HB_PRED_MULTI_CMAX, C);
  HB_REQUIRE(n >= 0 && M >= 1 && d >= 1, "hb_sgp_predict_multi: bad extents (n=%ld M=%ld d=%ld)", n, M, d);
  HB_REQUIRE(x && z && ell && W && m && S && mean && var, "hb_sgp_predict_multi: NULL pointer");
  HB_REQUIRE(n * d < 2147483647L && C * n < 2147483647L, "hb_sgp_predict_multi: matrix too large");
  HB_REQUIRE_RBF_MODEL("hb_sgp_predict_multi", "has a closed-form predictive", kind, dl, d, Wf, M);
  if (n == 0) return 0;
  const bool fused = pred_multi_is_fused(n, M, d, C, Wf != nullptr, (int)sizeof(T));
  const long need = hb_sgp_predict_multi_ws_elems(n, M, d, C, Wf != nullptr, (int)sizeof(T));
  HB_REQUIRE(need == 0 || (ws && (uintptr_t)ws % 16 == 0),
             "hb_sgp_predict_multi: needs a 16-byte aligned workspace of %ld elements", need);
  if constexpr (sizeof(T) == 4) {
    if (fused) {
      PredArgs a;
      a.x = x; a.sx = 0; a.z = z; a.ell = ell; a.dl = dl; a.Wf = Wf; a.STf = ws; a.m = m; a.s = nullptr;
      a.mode = mode; a.jitter = 0.f; a.mean = mean; a.var = var; a.n = n; a.M = M; a.P = 1;
      hipLaunchKernelGGL(pred_s_image_kernel<true>, dim3(hb_stream_grid(M * M, 256), (unsigned)C), dim3(256), 0, st, S, ws, M);
      HB_LAUNCH_CHECK();
      const dim3 grid((unsigned)hb_cdiv(n, SGP_SN), 1, 1);
      if (d == 1)
        hipLaunchKernelGGL((sgp_predict_multi_strip_kernel<1>), grid, dim3(PRED_THREADS), 0, st, a, (int)C);
      else if (d == 2)
        hipLaunchKernelGGL((sgp_predict_multi_strip_kernel<2>), grid, dim3(PRED_THREADS), 0, st, a, (int)C);
      else if (d == 3)
        hipLaunchKernelGGL((sgp_predict_multi_strip_kernel<3>), grid, dim3(PRED_THREADS), 0, st, a, (int)C);
      else
        hipLaunchKernelGGL((sgp_predict_multi_strip_kernel<4>), grid, dim3(PRED_THREADS), 0, st, a, (int)C);
      HB_LAUNCH_CHECK();
      return 0;
    }
  }
  // every other shape: the one-latent form (chunked, or fused for a diagonal-free shape it takes) once per latent function
  for (long c = 0; c < C; ++c) {
    const int rc = sgp_predict<T>(kind, x, 0, z, ell, dl, W, Wf, m + c * M, S + c * M * M, HB_SGP_S_TRIL, mode, 0.0, mean + c * n,
                                  var + c * n, 1, n, M, d, 1, ws, st);
    if (rc) return rc;
  }
  return 0;
}

extern "C" int hb_sgp_predict_f32(int kind, const float* x, long sx, const float* z, const float* ell, long dl, const float* W,
                                  const float* Wfrag, const float* m, const float* s, int s_kind, int mode, double jitter,
                                  float* mean, float* var, long E, long n, long M, long d, long P, float* ws, void* stream) {
  return sgp_predict<float>(kind, x, sx, z, ell, dl, W, Wfrag, m, s, s_kind, mode, jitter, mean, var, E, n, M, d, P, ws,
                            (hipStream_t)stream);
}
extern "C" int hb_sgp_predict_f64(int kind, const double* x, long sx, const double* z, const double* ell, long dl,
                                  const double* W, const double* Wfrag, const double* m, const double* s, int s_kind, int mode,
                                  double jitter, double* mean, double* var, long E, long n, long M, long d, long P, double* ws,
                                  void* stream) {
  return sgp_predict<double>(kind, x, sx, z, ell, dl, W, Wfrag, m, s, s_kind, mode, jitter, mean, var, E, n, M, d, P, ws,
                             (hipStream_t)stream);
}
extern "C" int hb_sgp_predict_multi_f32(int kind, const float* x, const float* z, const float* ell, long dl, const float* W,
                                        const float* Wfrag, const float* m, const float* S, int mode, float* mean, float* var,
                                        long n, long M, long d, long C, float* ws, void* stream) {
  return sgp_predict_multi<float>(kind, x, z, ell, dl, W, Wfrag, m, S, mode, mean, var, n, M, d, C, ws, (hipStream_t)stream);
}
extern "C" int hb_sgp_predict_multi_f64(int kind, const double* x, const double* z, const double* ell, long dl, const double* W,
                                        const double* Wfrag, const double* m, const double* S, int mode, double* mean,
                                        double* var, long n, long M, long d, long C, double* ws, void* stream) {
  return sgp_predict_multi<double>(kind, x, z, ell, dl, W, Wfrag, m, S, mode, mean, var, n, M, d, C, ws, (hipStream_t)stream);
}
