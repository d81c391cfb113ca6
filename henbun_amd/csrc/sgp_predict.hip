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
#include "common.cuh"
#include "sgp_strip.cuh"
#include "../../include/henbun_hip.h"

#define PRED_THREADS 512          // 8 waves; wave w owns the row tiles w and nT - 1 - w (balanced triangular work)
#define PRED_PMAX 4               // latent functions whose means / variances the fused form keeps per thread
#define PRED_RED_LD 260           // floats per column in the fold of the S^T A statistics (8 waves x 32 lanes + 4)
#define HB_PRED_CHUNK 32768L      // columns per chunk of the chunked form (at most)
#define HB_PRED_CHUNK_ELEMS (1L << 24)  // scratch of one chunk (elements, at most): A chunk + S^T A chunk

struct PredArgs {
  const float* x;    // [E?, n, d]
  long sx;           // expert stride of x (0: shared)
  const float* z;    // [E, M, d]
  const float* ell;  // [E, dl]
  long dl;
  const float* Wf;   // fragment-major image of W = L^-1 (hb_cholesky_inverse's Wfrag)
  const float* STf;  // fragment-major image of S^T (full rank), or nullptr
  const float* m;    // [E, P, M]
  const float* s;    // [E, P, M] standard deviations (diagonal S), unused for a full-rank S
  int mode;
  float jitter;
  float* mean;       // [E, P, n]
  float* var;        // [E, P, n]
  long n, M, P;
};

// ---------------------------------------------------------------------------------------------------------------
// One triangular strip product on MFMA: for every 32-row tile of the M x M operand whose image is `img` (fragment-major,
// the layout of hb_cholesky_inverse's Wfrag: block (t, Q) = rows 32 t.., contraction indices 32 Q..), times the strip
// operand Bs[column][k] in LDS.  Lower (UPPER = false): tile t contracts chunks Q = 0..t; upper: Q = t..nT-1.  The tile
// product is computed transposed (operands swapped, as sgp_A_strip2t_kernel does): when tile `tile` is finished,
// register r of lane (li, h) holds  result[32 tile + li][column (r & 3) + 8 (r >> 2) + 4 h]  and done(tile, acc) is called.
// Double-buffered: the image fragments of step ts + 1 are requested before the MFMAs of step ts.
// ---------------------------------------------------------------------------------------------------------------
template <bool UPPER, typename Done>
__device__ __forceinline__ void pred_strip_product(const float* __restrict__ img, const float* __restrict__ Bs, int nT, int w,
                                                   int lane, Done done) {
  typedef float V4 __attribute__((ext_vector_type(4)));
  typedef Mma<float> MM;
  const int li = lane & 31, h = lane >> 5;
  const int t0 = w, t1 = nT - 1 - w;
  // (the middle tile of an odd count is taken once, as t1)
  const int d0 = w < t1 ? (UPPER ? nT - t0 : t0 + 1) : 0;
  const int d1 = w <= t1 ? (UPPER ? nT - t1 : t1 + 1) : 0;
  const int nts = d0 + d1;
  if (nts <= 0) return;
  auto where = [&](int ts, int& tile, int& Q) {
    if (ts < d0) {
      tile = t0;
      Q = (UPPER ? t0 : 0) + ts;
    } else {
      tile = t1;
      Q = (UPPER ? t1 : 0) + ts - d0;
    }
  };
  auto load = [&](V4 (&f)[4], int ts) {
    int tile, Q;
    where(ts < nts ? ts : nts - 1, tile, Q);   // past the end: re-read the last step (never used)
    const float* p = img + ((long)(tile * nT + Q) << 10) + 4 * lane;
#pragma unroll
    for (int v = 0; v < 4; ++v) f[v] = *reinterpret_cast<const V4*>(p + 256 * v);
  };
  typename MM::Acc acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  auto compute = [&](const V4 (&f)[4], int ts) {
    if (ts >= nts) return;   // (uniform) the odd tail of the two-step loop
    int tile, Q;
    where(ts, tile, Q);
    V4 bv[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) bv[v] = *reinterpret_cast<const V4*>(&Bs[li * SGP_SLD + 32 * Q + 16 * h + 4 * v]);
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = MM::mma(bv[v][s], f[v][s], acc);
    if (ts == d0 - 1 || ts == nts - 1) {
      done(tile, acc);
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    }
  };
  V4 fa[4], fb[4];
  load(fa, 0);
#pragma nounroll
  for (int ts = 0; ts < nts; ts += 2) {
    load(fb, ts + 1);
    compute(fa, ts);
    load(fa, ts + 2);
    compute(fb, ts + 1);
  }
}

// One workgroup = 32 columns of one expert (blockIdx.x = strip, blockIdx.y = expert).
//   phase 1: K(z, x_strip) -> Ks[column][k];  A_strip = W K -> As[column][m]   (MFMA, W image)
//   phase 2: per column: sum A^2, m_p^T A, sum s_p^2 A^2      (16 threads per column, fixed order)
//   phase 3 (full rank): C = S^T A_strip (MFMA, S^T image), per-lane sums of C^2 folded through LDS
template <int D>
__global__ void __launch_bounds__(PRED_THREADS) sgp_predict_strip_kernel(PredArgs a) {
  typedef float V4 __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) float Ks[SGP_SN * SGP_SLD];   // K block; after phase 1 the C^2 fold buffer
  __shared__ __attribute__((aligned(16))) float As[SGP_SN * SGP_SLD];   // A_strip, column-major
  __shared__ __attribute__((aligned(16))) float zs[SGP_SM_MAX * D];
  static_assert(SGP_SN * PRED_RED_LD <= SGP_SN * SGP_SLD, "the fold buffer overlays the K block");
  const long e = blockIdx.y;
  const int bx = blockIdx.x;
  const float* __restrict__ x = a.x + e * a.sx;
  const float* __restrict__ z = a.z + e * a.M * D;
  const float* __restrict__ ell = a.ell + e * a.dl;
  const int M = (int)a.M, n = (int)a.n, P = (int)a.P;
  const int col0 = bx * SGP_SN;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 31, h = lane >> 5;
  const int nT = M / 32;

  // ---- phase 1a: K(z, x[strip]) -> LDS (the strip prologue of csrc/sgp_strip.cuh)
  {
    SgpStripColumn<D> col;
    col.load(x, ell, a.dl, col0, n, tid);
    for (int i = tid; i < M * D; i += PRED_THREADS) zs[i] = z[i];
    __syncthreads();
    const int c = tid & 31, kq = tid >> 5;
    for (int k4 = kq * 4; k4 < M; k4 += PRED_THREADS / 8) {
      V4 v;
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = col.value(&zs[(k4 + q) * D]);
      *reinterpret_cast<V4*>(&Ks[c * SGP_SLD + k4]) = v;
    }
  }
  __syncthreads();

  // ---- phase 1b: A_strip = W K on MFMA, finished tiles straight into As
  pred_strip_product<false>(a.Wf + e * a.M * a.M, Ks, nT, w, lane, [&](int tile, const Mma<float>::Acc& acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) As[((r & 3) + 8 * (r >> 2) + 4 * h) * SGP_SLD + 32 * tile + li] = acc[r];
  });
  __syncthreads();

  // ---- phase 3 (full rank, E P == 1): C = S^T A_strip; per-lane sums of C^2 in accumulator order
  if (a.STf) {
    float csq[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) csq[r] = 0.f;
    pred_strip_product<true>(a.STf, As, nT, w, lane, [&](int, const Mma<float>::Acc& acc) {
#pragma unroll
      for (int r = 0; r < 16; ++r) csq[r] = __builtin_fmaf(acc[r], acc[r], csq[r]);
    });
    // the K block is dead since the barrier above: it takes the fold of the 256 (wave, row-lane) partials per column
#pragma unroll
    for (int r = 0; r < 16; ++r) Ks[((r & 3) + 8 * (r >> 2) + 4 * h) * PRED_RED_LD + 32 * w + li] = csq[r];
  }

  // ---- phase 2: column statistics from As; 16 threads per column, rows g, g + 16, ...
  const int c = tid >> 4, g = tid & 15;
  const float* mp = a.m + e * a.P * a.M;
  const float* sp = a.s ? a.s + e * a.P * a.M : nullptr;
  float sa2 = 0.f, mu[PRED_PMAX], ss[PRED_PMAX];
#pragma unroll
  for (int p = 0; p < PRED_PMAX; ++p) mu[p] = 0.f, ss[p] = 0.f;
  for (int k = g; k < M; k += 16) {
    const float av = As[c * SGP_SLD + k];
    sa2 = __builtin_fmaf(av, av, sa2);
#pragma unroll
    for (int p = 0; p < PRED_PMAX; ++p) {
      if (p < P) {
        mu[p] = __builtin_fmaf(mp[(long)p * M + k], av, mu[p]);
        if (!a.STf) {
          const float t = sp[(long)p * M + k] * av;
          ss[p] = __builtin_fmaf(t, t, ss[p]);
        }
      }
    }
  }
  float csum = 0.f;
  if (a.STf) {
    __syncthreads();   // every wave's C^2 partials are in the fold buffer
#pragma unroll
    for (int i = 0; i < 16; ++i) csum += Ks[c * PRED_RED_LD + 16 * g + i];
  }
  // fixed-order tree over the 16 threads of the column (lanes 16 c' .. 16 c' + 15 of a wave)
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) {
    sa2 += __shfl_xor(sa2, off, 16);
    csum += __shfl_xor(csum, off, 16);
#pragma unroll
    for (int p = 0; p < PRED_PMAX; ++p) {
      mu[p] += __shfl_xor(mu[p], off, 16);
      ss[p] += __shfl_xor(ss[p], off, 16);
    }
  }
  const int j = col0 + c;
  if (g == 0 && j < n) {
    const float r = a.mode == HB_SGP_DIAGONAL ? fabsf(1.f - sa2) : a.mode == HB_SGP_FULLRANK ? (1.f - sa2) + a.jitter : 0.f;
#pragma unroll
    for (int p = 0; p < PRED_PMAX; ++p) {
      if (p < P) {
        const long o = (e * a.P + p) * a.n + j;
        a.mean[o] = mu[p];
        a.var[o] = (a.STf ? csum : ss[p]) + r;
      }
    }
  }
}

// Fragment-major image of S^T for the full-rank fused form, in the layout of Wfrag (csrc/linalg.hip, tril_inplace_kernel):
//   element (t, Q, v, lane = (li, h), s) = S^T[32 t + li][32 Q + 16 h + 4 v + s] = S[k][r],  r = 32 t + li, k = 32 Q + ...,
// zero where k < r (only the lower triangle of S is read).
__global__ void __launch_bounds__(256) pred_st_image_kernel(const float* __restrict__ S, float* __restrict__ STf, long M) {
  const int Mi = (int)M, nT = Mi / 32;
  const long total = M * M, stride = (long)gridDim.x * blockDim.x;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int rem = (int)t;
    const int s = rem & 3, lane = (rem >> 2) & 63, v = (rem >> 8) & 3, blk = rem >> 10;
    const int Q = blk % nT, tt = blk / nT, li = lane & 31, h = lane >> 5;
    const int r = 32 * tt + li, k = 32 * Q + 16 * h + 4 * v + s;
    STf[t] = k >= r ? S[(long)k * Mi + r] : 0.f;
  }
}

// Chunked form, column statistics of one chunk: one thread per (e, p, column j of the chunk).
//   A [E, M, nc];  C [E P, R, nc] (full rank: C_ep = S_ep^T A_e, S_ep = rows (e P + p) M .. of S) or nullptr
template <typename T>
__global__ void __launch_bounds__(256) pred_colstat_kernel(const T* __restrict__ A, const T* __restrict__ C,
                                                           const T* __restrict__ m, const T* __restrict__ s, int mode,
                                                           T jitter, T* __restrict__ mean, T* __restrict__ var, long E, long P,
                                                           long M, long R, long nc, long n, long j0) {
  const long total = E * P * nc, stride = (long)gridDim.x * blockDim.x;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const long j = t % nc, ep = t / nc, e = ep / P;
    const T* Ae = A + e * M * nc + j;
    const T* mp = m + ep * M;
    const T* sp = C ? nullptr : s + ep * M;
    T sa2 = T(0), mu = T(0), ss = T(0);
    for (long k = 0; k < M; ++k) {
      const T av = Ae[k * nc];
      sa2 += av * av;
      mu += mp[k] * av;
      if (!C) {
        const T q = sp[k] * av;
        ss += q * q;
      }
    }
    if (C) {
      const T* Cp = C + ep * R * nc + j;
      for (long k = 0; k < R; ++k) {
        const T cv = Cp[k * nc];
        ss += cv * cv;
      }
    }
    const T one = T(1);
    const T r = mode == HB_SGP_DIAGONAL ? (sa2 > one ? sa2 - one : one - sa2) : mode == HB_SGP_FULLRANK ? (one - sa2) + jitter : T(0);
    const long o = ep * n + j0 + j;
    mean[o] = mu;
    var[o] = ss + r;
  }
}

static inline bool pred_fused_ok(long E, long n, long M, long d, long P, int s_kind) {
  return M >= 32 && M <= SGP_SM_MAX && M % 32 == 0 && d >= 1 && d <= SGP_DREG && P >= 1 && P <= PRED_PMAX && n > 0 &&
         E >= 1 && E <= 65535 && (s_kind == HB_SGP_S_DIAG || E * P == 1);
}
static inline long pred_chunk_cols(long E, long n, long M, long P, int s_kind) {
  const long per_col = E * M + (s_kind == HB_SGP_S_TRIL ? E * P * (E * P * M) : 0);
  long c = HB_PRED_CHUNK_ELEMS / (per_col > 0 ? per_col : 1);
  c = c < HB_PRED_CHUNK ? c : HB_PRED_CHUNK;
  c = c & ~31L;
  if (c < 32) c = 32;
  const long n32 = (n + 31) & ~31L;
  return c < n32 ? c : (n32 > 0 ? n32 : 32);
}
static inline bool pred_is_fused(long E, long n, long M, long d, long P, int s_kind, bool has_wfrag, int dbytes) {
  return dbytes == 4 && has_wfrag && pred_fused_ok(E, n, M, d, P, s_kind);
}

extern "C" long hb_sgp_predict_ws_elems(long E, long n, long M, long d, long P, int s_kind, int has_wfrag, int dtype_bytes) {
  if (E <= 0 || n <= 0 || M <= 0 || P <= 0) return 0;
  if (pred_is_fused(E, n, M, d, P, s_kind, has_wfrag != 0, dtype_bytes)) return s_kind == HB_SGP_S_TRIL ? M * M : 0;
  const long nc = pred_chunk_cols(E, n, M, P, s_kind);
  return nc * (E * M + (s_kind == HB_SGP_S_TRIL ? E * P * (E * P * M) : 0));
}

static inline int pred_sgp_A(int kind, const float* x, long sx, const float* z, const float* ell, long dl, const float* W,
                             const float* Wf, float* A, long E, long n, long M, long d, hipStream_t st) {
  return hb_sgp_A_f32(kind, x, sx, z, ell, dl, W, Wf, HB_PREC_NATIVE, A, E, n, M, d, st);
}
static inline int pred_sgp_A(int kind, const double* x, long sx, const double* z, const double* ell, long dl, const double* W,
                             const double* Wf, double* A, long E, long n, long M, long d, hipStream_t st) {
  return hb_sgp_A_f64(kind, x, sx, z, ell, dl, W, Wf, HB_PREC_NATIVE, A, E, n, M, d, st);
}
static inline int pred_matmul(const float* A, const float* B, float* C, long batch, long Mo, long N, long K, long lda, long ldb,
                              long ldc, long sA, long sB, long sC, hipStream_t st) {
  return hb_matmul_f32(A, B, C, batch, Mo, N, K, lda, ldb, ldc, sA, sB, sC, 1, 0, 1.0, 0.0, nullptr, 0, HB_ACT_NONE, 0,
                       nullptr, 0, st);
}
static inline int pred_matmul(const double* A, const double* B, double* C, long batch, long Mo, long N, long K, long lda,
                              long ldb, long ldc, long sA, long sB, long sC, hipStream_t st) {
  return hb_matmul_f64(A, B, C, batch, Mo, N, K, lda, ldb, ldc, sA, sB, sC, 1, 0, 1.0, 0.0, nullptr, 0, HB_ACT_NONE, 0,
                       nullptr, 0, st);
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
  HB_REQUIRE(kind == HB_KERN_RBF, "hb_sgp_predict: only the UnitRBF kernel has a closed-form predictive (kind=%d)", kind);
  HB_REQUIRE(mode == HB_SGP_NEGLECTED || mode == HB_SGP_DIAGONAL || mode == HB_SGP_FULLRANK,
             "hb_sgp_predict: unknown residual mode %d", mode);
  HB_REQUIRE(s_kind == HB_SGP_S_DIAG || s_kind == HB_SGP_S_TRIL, "hb_sgp_predict: unknown s_kind %d", s_kind);
  HB_REQUIRE(E >= 1 && n >= 0 && M >= 1 && d >= 1 && P >= 1, "hb_sgp_predict: bad extents (E=%ld n=%ld M=%ld d=%ld P=%ld)",
             E, n, M, d, P);
  HB_REQUIRE(dl == 1 || dl == d, "hb_sgp_predict: lengthscales must have 1 or d entries");
  HB_REQUIRE(sx == 0 || sx == n * d, "hb_sgp_predict: x is shared (sx = 0) or [E, n, d] (sx = n d), got sx=%ld", sx);
  HB_REQUIRE(x && z && ell && W && m && s && mean && var, "hb_sgp_predict: NULL pointer");
  HB_REQUIRE(E <= 65535, "hb_sgp_predict: too many experts");
  const long R = E * P * M;
  HB_REQUIRE(M * M < 2147483647L && n * d < 2147483647L && (s_kind == HB_SGP_S_DIAG || R * R < 2147483647L),
             "hb_sgp_predict: matrix too large");
  HB_REQUIRE(!Wf || ((uintptr_t)Wf % 16 == 0 && M % 32 == 0), "hb_sgp_predict: Wfrag needs 16-byte alignment and M %% 32 == 0");
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
        hipLaunchKernelGGL(pred_st_image_kernel, dim3(hb_stream_grid(M * M, 256)), dim3(256), 0, st, s, ws, M);
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
    int rc = pred_sgp_A(kind, x + j0 * d, sx, z, ell, dl, W, Wf, Abuf, E, nc, M, d, st);
    if (rc) return rc;
    if (Cbuf) {
      // C_ep = S_ep^T A_e: op(A) of the product is the [M, R] row block of S transposed
      for (long e = 0; e < E; ++e) {
        rc = pred_matmul(s + e * P * M * R, Abuf + e * M * nc, Cbuf + e * P * R * nc, P, R, nc, M, R, nc, nc, M * R, 0, R * nc, st);
        if (rc) return rc;
      }
    }
    hipLaunchKernelGGL((pred_colstat_kernel<T>), dim3(hb_stream_grid(E * P * nc, 256)), dim3(256), 0, st, Abuf, Cbuf, m, s, mode,
                       (T)jitter, mean, var, E, P, M, R, nc, n, j0);
    HB_LAUNCH_CHECK();
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
