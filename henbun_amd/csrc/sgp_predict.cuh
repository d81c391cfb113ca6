// What the closed-form predictive kernels share (csrc/sgp_predict.hip: mean and variance; csrc/sgp_predict_grad.hip:
// their input gradients and the acquisition functions): the triangular strip product on MFMA, phases 1-3 of the fused
// strip kernel (the K fill, A = W K, C = S^T A and the column statistics), the residual term, the fragment-major image
// of S^T / S, the column-statistics kernel of the chunked form and the chunk rule.  One definition of each, so that
// every entry that reports a mean or a variance stores the same bits.
#ifndef HB_SGP_PREDICT_CUH
#define HB_SGP_PREDICT_CUH
#include "host_calls.cuh"   // hb_chunk_cols, hb_sgp_A, hb_matmul, HB_REQUIRE_RBF_MODEL
#include "sgp_strip.cuh"

#define PRED_THREADS 512          // 8 waves; wave w owns the row tiles w and nT - 1 - w (balanced triangular work)
#define PRED_PMAX 4               // latent functions whose means / variances the fused form keeps per thread
#define HB_PRED_MULTI_CMAX 64     // latent functions of one hb_sgp_predict_multi_* call (at most)
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

// the column of the strip that accumulator register r of lane half h holds (see pred_strip_product)
__device__ __forceinline__ int pred_acc_col(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// r_j of the variance from sum_m A_mj^2
template <typename T>
__device__ __forceinline__ T pred_residual(int mode, T sa2, T jitter) {
  const T one = T(1);
  return mode == HB_SGP_DIAGONAL ? (sa2 > one ? sa2 - one : one - sa2) : mode == HB_SGP_FULLRANK ? (one - sa2) + jitter : T(0);
}

// The statistics of one column as phases 2 and 3 leave them, complete on each of the column's 16 threads
// (column tid / 16 of the strip): sa2 = sum A^2, mu[p] = m_p^T A, ss[p] = sum s_p^2 A^2 (diagonal S), csum = ||S^T A||^2.
struct PredMoments {
  float sa2, csum, mu[PRED_PMAX], ss[PRED_PMAX];
  __device__ __forceinline__ float var(bool fullS, int p, int mode, float jitter) const {
    return (fullS ? csum : ss[p]) + pred_residual<float>(mode, sa2, jitter);
  }
};

// The phases of a 32-column strip (blockIdx.x = strip, expert e) on the workgroup's buffers Ks, As [SGP_SN * SGP_SLD] and
// zs [SGP_SM_MAX * D], one function each so that every kernel that reports a mean or a variance runs the same code:
//   pred_strip_A       phase 1: K(z, x_strip) -> Ks[column][k];  A_strip = W K -> As[column][m]   (MFMA, W image)
//   pred_strip_colsums phase 2: per column: sum A^2, m_p^T A, sum s_p^2 A^2      (16 threads per column, fixed order)
//   pred_strip_c2      phase 3 (full rank): C = S^T A_strip (MFMA, S^T image), per-lane sums of C^2 into the fold buffer
//                      that overlays the dead K block; every finished tile of C is also handed to tileC(tile, acc)
//   pred_strip_c2_fold the column's share of that fold;  pred_col_tree the fixed-order tree over a column's 16 threads
// pred_strip_moments runs them for one set of at most PRED_PMAX latent functions (one S); csrc/sgp_predict.hip's
// multi-latent kernel runs phase 1 once, phase 2 per group of PRED_PMAX means and phase 3 per latent function.
template <int D>
__device__ __forceinline__ void pred_strip_A(const PredArgs& a, float* Ks, float* As, float* zs, long e) {
  typedef float V4 __attribute__((ext_vector_type(4)));
  static_assert(SGP_SN * PRED_RED_LD <= SGP_SN * SGP_SLD, "the fold buffer overlays the K block");
  const int bx = blockIdx.x;
  const float* __restrict__ x = a.x + e * a.sx;
  const float* __restrict__ z = a.z + e * a.M * D;
  const float* __restrict__ ell = a.ell + e * a.dl;
  const int M = (int)a.M, n = (int)a.n;
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
    for (int r = 0; r < 16; ++r) As[pred_acc_col(r, h) * SGP_SLD + 32 * tile + li] = acc[r];
  });
  __syncthreads();
}

// phase 3 for the S^T image STf: C = S^T A_strip; per-lane sums of C^2 in accumulator order, left in the fold buffer (the
// first SGP_SN * PRED_RED_LD floats of Ks: 256 (wave, row-lane) partials per column).  The caller owns the barriers: none
// of Ks may still be read when this starts, and a barrier stands between it and pred_strip_c2_fold.
template <typename TileC>
__device__ __forceinline__ void pred_strip_c2(const float* __restrict__ STf, const float* As, float* Ks, int nT, int w, int lane,
                                              TileC tileC) {
  const int li = lane & 31, h = lane >> 5;
  float csq[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) csq[r] = 0.f;
  pred_strip_product<true>(STf, As, nT, w, lane, [&](int tile, const Mma<float>::Acc& acc) {
#pragma unroll
    for (int r = 0; r < 16; ++r) csq[r] = __builtin_fmaf(acc[r], acc[r], csq[r]);
    tileC(tile, acc);
  });
#pragma unroll
  for (int r = 0; r < 16; ++r) Ks[pred_acc_col(r, h) * PRED_RED_LD + 32 * w + li] = csq[r];
}

// thread (c, g)'s share of column c's fold: 16 of its 256 partials, in order
__device__ __forceinline__ float pred_strip_c2_fold(const float* Ks, int c, int g) {
  float csum = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) csum += Ks[c * PRED_RED_LD + 16 * g + i];
  return csum;
}

// phase 2: thread (c, g)'s share (rows g, g + 16, ...) of column c's statistics for P <= PRED_PMAX means mp [P, M] and,
// with sp (diagonal S), standard deviations sp [P, M]
__device__ __forceinline__ void pred_strip_colsums(const float* As, const float* __restrict__ mp, const float* __restrict__ sp,
                                                   int M, int P, int c, int g, float& sa2, float (&mu)[PRED_PMAX],
                                                   float (&ss)[PRED_PMAX]) {
  sa2 = 0.f;
#pragma unroll
  for (int p = 0; p < PRED_PMAX; ++p) mu[p] = 0.f, ss[p] = 0.f;
  for (int k = g; k < M; k += 16) {
    const float av = As[c * SGP_SLD + k];
    sa2 = __builtin_fmaf(av, av, sa2);
#pragma unroll
    for (int p = 0; p < PRED_PMAX; ++p) {
      if (p < P) {
        mu[p] = __builtin_fmaf(mp[(long)p * M + k], av, mu[p]);
        if (sp) {
          const float t = sp[(long)p * M + k] * av;
          ss[p] = __builtin_fmaf(t, t, ss[p]);
        }
      }
    }
  }
}

// fixed-order tree over the 16 threads of a column (lanes 16 c' .. 16 c' + 15 of a wave): every one ends with the sum
__device__ __forceinline__ float pred_col_tree(float v) {
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 16);
  return v;
}

// On return As holds A_strip, zs holds z, and Ks (its first SGP_SN * PRED_RED_LD floats the fold buffer of phase 3) is
// dead once every thread has passed a barrier.
template <int D, typename TileC>
__device__ __forceinline__ void pred_strip_moments(const PredArgs& a, float* Ks, float* As, float* zs, long e, PredMoments& o,
                                                   TileC tileC) {
  const int M = (int)a.M, P = (int)a.P;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  pred_strip_A<D>(a, Ks, As, zs, e);
  // (the K block is dead since the barrier that ends phase 1: it takes the fold of phase 3)
  if (a.STf) pred_strip_c2(a.STf, As, Ks, M / 32, w, lane, tileC);
  const int c = tid >> 4, g = tid & 15;
  float sa2, mu[PRED_PMAX], ss[PRED_PMAX];
  pred_strip_colsums(As, a.m + e * a.P * a.M, a.STf ? nullptr : a.s + e * a.P * a.M, M, P, c, g, sa2, mu, ss);
  float csum = 0.f;
  if (a.STf) {
    __syncthreads();   // every wave's C^2 partials are in the fold buffer
    csum = pred_strip_c2_fold(Ks, c, g);
  }
  o.sa2 = pred_col_tree(sa2), o.csum = pred_col_tree(csum);
#pragma unroll
  for (int p = 0; p < PRED_PMAX; ++p) o.mu[p] = pred_col_tree(mu[p]), o.ss[p] = pred_col_tree(ss[p]);
}

// Fragment-major image of a triangular factor for the full-rank fused forms, in the layout of Wfrag (csrc/linalg.hip,
// tril_inplace_kernel): element (t, Q, v, lane = (li, h), s) = X[32 t + li][32 Q + 16 h + 4 v + s], r = 32 t + li,
// k = 32 Q + ..., with X = S^T (TRANS: S[k][r], zero where k < r) or X = S (S[r][k], zero where k > r); only the lower
// triangle of S is read.  blockIdx.y = which of gridDim.y matrices S [gridDim.y, M, M] (one image each, M^2 apart).
template <bool TRANS>
__global__ void __launch_bounds__(256) pred_s_image_kernel(const float* __restrict__ S, float* __restrict__ Xf, long M) {
  const int Mi = (int)M, nT = Mi / 32;
  const long total = M * M, stride = (long)gridDim.x * blockDim.x;
  S += blockIdx.y * total;
  Xf += blockIdx.y * total;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int rem = (int)t;
    const int s = rem & 3, lane = (rem >> 2) & 63, v = (rem >> 8) & 3, blk = rem >> 10;
    const int Q = blk % nT, tt = blk / nT, li = lane & 31, h = lane >> 5;
    const int r = 32 * tt + li, k = 32 * Q + 16 * h + 4 * v + s;
    if (TRANS)
      Xf[t] = k >= r ? S[(long)k * Mi + r] : 0.f;
    else
      Xf[t] = k <= r ? S[(long)r * Mi + k] : 0.f;
  }
}

// Chunked form, column statistics of one chunk: one thread per (e, p, column j of the chunk).
//   A [E, M, nc];  C [E P, R, nc] (full rank: C_ep = S_ep^T A_e, S_ep = rows (e P + p) M .. of S) or nullptr
//   sa2_out [E P, nc] (nullable): sum_m A_mj^2 of the column
template <typename T>
__global__ void __launch_bounds__(256) pred_colstat_kernel(const T* __restrict__ A, const T* __restrict__ C,
                                                           const T* __restrict__ m, const T* __restrict__ s, int mode,
                                                           T jitter, T* __restrict__ mean, T* __restrict__ var,
                                                           T* __restrict__ sa2_out, long E, long P, long M, long R, long nc,
                                                           long n, long j0) {
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
    const T r = pred_residual<T>(mode, sa2, jitter);
    const long o = ep * n + j0 + j;
    mean[o] = mu;
    var[o] = ss + r;
    if (sa2_out) sa2_out[t] = sa2;
  }
}

static inline bool pred_fused_ok(long E, long n, long M, long d, long P, int s_kind) {
  return M >= 32 && M <= SGP_SM_MAX && M % 32 == 0 && d >= 1 && d <= SGP_DREG && P >= 1 && P <= PRED_PMAX && n > 0 &&
         E >= 1 && E <= 65535 && (s_kind == HB_SGP_S_DIAG || E * P == 1);
}
static inline bool pred_is_fused(long E, long n, long M, long d, long P, int s_kind, bool has_wfrag, int dbytes) {
  return dbytes == 4 && has_wfrag && pred_fused_ok(E, n, M, d, P, s_kind);
}

#endif  // HB_SGP_PREDICT_CUH
