// Full predictive covariance of SparseGP.samples (hb_sgp_predict_cov_*, include/henbun_hip.h).
//
// samples() draws f_p = u_p^T A + residual with A = L^-1 K(z, x), u_p ~ N(m_p, S_p S_p^T) (reference gp/gp.py:99-143).
// The covariance of that draw between test points i and j is
//     cov_p = A^T S_p S_p^T A + R,   R = K(x, x) - A^T A + jitter I  (FULLRANK: the matrix samples() factorises)
//                                        diag(|1 - sum_m A_m^2|)      (DIAGONAL: independent residuals)
//                                        0                            (NEGLECTED)
// and its diagonal is hb_sgp_predict's var.
//
// Pass 1 writes A_e [E, M, n] into the workspace with hb_sgp_A_* (from Wfrag when given), for a full-rank S (E P == 1)
// also C = S^T A [M, n] with hb_matmul_*, and the column sums a2 = sum_m A_m^2 (mode DIAGONAL) with the arithmetic of
// csrc/sgp_predict.hip's pred_colstat_kernel.
//
// Pass 2 (fp32) is a symmetric weighted product on MFMA with the RBF block synthesised in the epilogue: one workgroup
// per 128 x 128 lower-triangle tile (ti >= tj) of one (e, p).  The K-loop runs over the rows k of A with the weight
//     w_k = s_pk^2 - [FULLRANK]   (diagonal S)        w_k = -[FULLRANK]   (full-rank S; zero weights are skipped)
// on the row-panel operand, then (full-rank S) over the rows of C with weight 1, so one accumulator holds
// A^T diag(w) A (+ C^T C): the -A^T A of FULLRANK is folded into the weight, not subtracted from a second sum.  The
// epilogue adds k(x_i, x_j) (FULLRANK; gram_value.cuh, the function of the Gram kernels: the diagonal is exactly 1) and
// jitter or |1 - a2_i| on the diagonal, and writes the tile and its mirror image through LDS so both stores are
// coalesced.  Only lower-triangle values are ever stored, so cov is bitwise symmetric.  Every tile is independent.
//
// fp64 runs a plain FMA loop in the same order (parity, not speed).
#include "host_calls.cuh"   // hb_round64, hb_sgp_A, hb_matmul, HB_REQUIRE_RBF_MODEL
#include "gram_value.cuh"

#define COV_BT 128               // output tile (rows = cols)
#define COV_KB 16                // K rows per LDS stage
#define COV_THREADS 256          // 4 waves in 2 x 2; wave (wi, wj) owns rows 64 wi .., cols 64 wj .. of the tile
#define COV_TLD (COV_BT + 1)     // row stride of the epilogue's half tile [64][129]: column reads are conflict-free
#define COV_STAGE (2 * COV_KB * COV_BT)                       // one stage: row panel + column panel
#define COV_SMEM (2 * COV_STAGE > 64 * COV_TLD ? 2 * COV_STAGE : 64 * COV_TLD)
#define COV_NXCD 8
#define COV_F64_T 16             // fp64: 16 x 16 threads per block

struct CovArgs {
  const float* x;    // [n, d] of expert e at x + e sx
  long sx;
  const float* ell;  // [E, dl]
  long dl, d;
  const float* A;    // [E, M, n]; a full-rank S (E = 1): the rows of C = S^T A follow at A + M n + gap
  long gap;          // padding between the last row of A and the first row of C (elements)
  const float* s;    // [E, P, M] standard deviations (diagonal S) or nullptr
  const float* a2;   // [E, n] (DIAGONAL) or nullptr
  int mode;
  float jitter;
  float* cov;        // [E, P, n, n]
  long n, M, P;
  long kbeg, kend;   // K rows [kbeg, kend): k < M a row of A_e, k >= M row k - M of C
};

__global__ void __launch_bounds__(COV_THREADS) sgp_predict_cov_kernel(CovArgs a) {
  typedef Mma<float> MM;
  __shared__ __attribute__((aligned(16))) float smem[COV_SMEM];
  const long ep = blockIdx.y, e = ep / a.P;
  const long n = a.n;
  // XCD-aware remap of the triangular grid (cdna_hip_programming.md T1, bijective form): the blocks one XCD receives
  // (bid % 8 equal) take a contiguous run of tiles, which share row panels in its L2.  Speed only, never correctness.
  long t;
  {
    const long nwg = gridDim.x, bid = blockIdx.x, q = nwg / COV_NXCD, r = nwg % COV_NXCD, xcd = bid % COV_NXCD;
    t = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / COV_NXCD;
  }
  long ti = (long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (ti * (ti + 1) / 2 > t) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  const long tj = t - ti * (ti + 1) / 2;
  const long i0 = ti * COV_BT, j0 = tj * COV_BT;
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, hl = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), wi = w >> 1, wj = w & 1;
  const float fr = a.mode == HB_SGP_FULLRANK ? 1.f : 0.f;
  const float* sp = a.s ? a.s + ep * a.M : nullptr;

  // staging: thread tid loads elements tid + 256 q (q < 8) of each [16][128] panel: row 2 q + tid / 128, col tid % 128
  const int lc = tid & (COV_BT - 1), lr = tid >> 7;
  const bool iok = i0 + lc < n, jok = j0 + lc < n;
  const float* Ae = a.A + e * a.M * n;
  const long ci = iok ? i0 + lc : 0, cj = jok ? j0 + lc : 0;
  float ri[8], rj[8];
  auto load = [&](long k0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const long k = k0 + 2 * q + lr;
      float vi = 0.f, vj = 0.f;
      if (k < a.kend) {
        const float* row = Ae + k * n + (k < a.M ? 0 : a.gap);
        const float wk = k < a.M ? (sp ? sp[k] * sp[k] : 0.f) - fr : 1.f;
        vi = iok ? wk * row[ci] : 0.f;
        vj = jok ? row[cj] : 0.f;
      }
      ri[q] = vi;
      rj[q] = vj;
    }
  };
  auto store = [&](int buf) {
    float* Ai = smem + buf * COV_STAGE;
    float* Aj = Ai + COV_KB * COV_BT;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      Ai[(2 * q + lr) * COV_BT + lc] = ri[q];
      Aj[(2 * q + lr) * COV_BT + lc] = rj[q];
    }
  };

  MM::Acc acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[u][v][r] = 0.f;

  const long ns = (a.kend - a.kbeg + COV_KB - 1) / COV_KB;
  if (ns > 0) {
    load(a.kbeg);
    store(0);
  }
  __syncthreads();
  for (long st = 0; st < ns; ++st) {
    if (st + 1 < ns) load(a.kbeg + (st + 1) * COV_KB);   // in flight during this stage's MFMAs
    const float* Ai = smem + (st & 1) * COV_STAGE;
    const float* Aj = Ai + COV_KB * COV_BT;
#pragma unroll
    for (int kk = 0; kk < COV_KB; kk += 2) {
      // 32x32x2: lane (li, hl) supplies A-operand [i = li][k = hl] and B-operand [k = hl][j = li]
      const float* pi = Ai + (kk + hl) * COV_BT + 64 * wi + li;
      const float* pj = Aj + (kk + hl) * COV_BT + 64 * wj + li;
      const float a0 = pi[0], a1 = pi[32], b0 = pj[0], b1 = pj[32];
      acc[0][0] = MM::mma(a0, b0, acc[0][0]);
      acc[0][1] = MM::mma(a0, b1, acc[0][1]);
      acc[1][0] = MM::mma(a1, b0, acc[1][0]);
      acc[1][1] = MM::mma(a1, b1, acc[1][1]);
    }
    if (st + 1 < ns) store((st + 1) & 1);
    __syncthreads();
  }

  // epilogue, one 64-row half of the tile at a time through T[64][129] (overlays the staging buffers):
  // accumulators -> T; T += k(x_i, x_j) and the diagonal term; T -> the tile and its mirror image
  float* T = smem;
  const float* xe = a.x + e * a.sx;
  const float* elle = a.ell + e * a.dl;
  float* out = a.cov + ep * (n * n);
  const bool diag_tile = ti == tj;
  for (int hh = 0; hh < 2; ++hh) {
    if (wi == hh) {
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            T[(32 * u + MM::acc_row(lane, r)) * COV_TLD + 64 * wj + 32 * v + MM::acc_col(lane)] = acc[u][v][r];
    }
    __syncthreads();
    const long r0 = i0 + 64 * hh;
    if (a.mode != HB_SGP_NEGLECTED) {
#pragma nounroll
      for (int q = tid; q < 64 * COV_BT; q += COV_THREADS) {
        const int rl = q / COV_BT, c = q % COV_BT;
        const long gi = r0 + rl, gj = j0 + c;
        if (gi >= n || gj >= n) continue;
        float val = T[rl * COV_TLD + c];
        if (a.mode == HB_SGP_FULLRANK) val += gram_value<float>(HB_KERN_RBF, xe + gi * a.d, xe + gj * a.d, elle, a.dl, a.d);
        if (gi == gj) val += a.mode == HB_SGP_FULLRANK ? a.jitter : fabsf(1.f - a.a2[e * n + gi]);
        T[rl * COV_TLD + c] = val;
      }
      __syncthreads();
    }
    // the tile itself: row-major, 128 consecutive columns per row (the diagonal tile: its lower triangle only)
    for (int q = tid; q < 64 * COV_BT; q += COV_THREADS) {
      const int rl = q / COV_BT, c = q % COV_BT;
      const long gi = r0 + rl, gj = j0 + c;
      if (gi < n && gj < n && (!diag_tile || gi >= gj)) out[gi * n + gj] = T[rl * COV_TLD + c];
    }
    // its mirror image: row gj of cov takes column c of T, 64 consecutive entries (strictly lower elements only)
    for (int q = tid; q < 64 * COV_BT; q += COV_THREADS) {
      const int c = q / 64, rl = q % 64;
      const long gi = r0 + rl, gj = j0 + c;
      if (gi < n && gj < n && gi > gj) out[gj * n + gi] = T[rl * COV_TLD + c];
    }
    __syncthreads();
  }
}

// fp64: one thread per lower-triangle element (i >= j), the same weights and epilogue; writes (i, j) and (j, i).
__global__ void __launch_bounds__(COV_F64_T * COV_F64_T) sgp_predict_cov_f64_kernel(
    const double* __restrict__ x, long sx, const double* __restrict__ ell, long dl, long d, const double* __restrict__ A,
    long gap, const double* __restrict__ s, const double* __restrict__ a2, int mode, double jitter,
    double* __restrict__ cov, long n, long M, long P, long kbeg, long kend) {
  if (blockIdx.x > blockIdx.y) return;   // the tile lies above the diagonal
  const long ep = blockIdx.z, e = ep / P;
  const long i = (long)blockIdx.y * COV_F64_T + threadIdx.y, j = (long)blockIdx.x * COV_F64_T + threadIdx.x;
  if (i >= n || j > i) return;
  const double fr = mode == HB_SGP_FULLRANK ? 1.0 : 0.0;
  const double* sp = s ? s + ep * M : nullptr;
  double acc = 0.0;
  for (long k = kbeg; k < kend; ++k) {
    const double* row = A + (e * M + k) * n + (k < M ? 0 : gap);
    const double wk = k < M ? (sp ? sp[k] * sp[k] : 0.0) - fr : 1.0;
    acc = __builtin_fma(wk * row[i], row[j], acc);
  }
  if (mode == HB_SGP_FULLRANK) acc += gram_value<double>(HB_KERN_RBF, x + e * sx + i * d, x + e * sx + j * d, ell + e * dl, dl, d);
  if (i == j) acc += mode == HB_SGP_FULLRANK ? jitter : mode == HB_SGP_DIAGONAL ? fabs(1.0 - a2[e * n + i]) : 0.0;
  double* out = cov + ep * n * n;
  out[i * n + j] = acc;
  out[j * n + i] = acc;
}

// a2[e, j] = sum_k A[e, k, j]^2, the loop of pred_colstat_kernel (csrc/sgp_predict.hip)
template <typename T>
__global__ void __launch_bounds__(256) pred_cov_a2_kernel(const T* __restrict__ A, T* __restrict__ a2, long E, long M, long n) {
  const long total = E * n, stride = (long)gridDim.x * blockDim.x;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const long j = t % n, e = t / n;
    const T* Ae = A + e * M * n + j;
    T sa2 = T(0);
    for (long k = 0; k < M; ++k) {
      const T av = Ae[k * n];
      sa2 += av * av;
    }
    a2[t] = sa2;
  }
}

extern "C" long hb_sgp_predict_cov_ws_elems(long E, long n, long M, long P, int s_kind, int dtype_bytes) {
  (void)P;
  (void)dtype_bytes;
  if (E <= 0 || n <= 0 || M <= 0) return 0;
  return hb_round64(E * M * n) + (s_kind == HB_SGP_S_TRIL ? hb_round64(M * n) : 0) + hb_round64(E * n);
}

template <typename T>
static int sgp_predict_cov(int kind, const T* x, long sx, const T* z, const T* ell, long dl, const T* W, const T* Wf,
                           const T* s, int s_kind, int mode, double jitter, T* cov, long E, long n, long M, long d, long P,
                           T* ws, hipStream_t st) {
  HB_REQUIRE(mode == HB_SGP_NEGLECTED || mode == HB_SGP_DIAGONAL || mode == HB_SGP_FULLRANK,
             "hb_sgp_predict_cov: unknown residual mode %d", mode);
  HB_REQUIRE(s_kind == HB_SGP_S_DIAG || s_kind == HB_SGP_S_TRIL, "hb_sgp_predict_cov: unknown s_kind %d", s_kind);
  HB_REQUIRE(E >= 1 && n >= 0 && M >= 1 && d >= 1 && P >= 1,
             "hb_sgp_predict_cov: bad extents (E=%ld n=%ld M=%ld d=%ld P=%ld)", E, n, M, d, P);
  HB_REQUIRE(s_kind == HB_SGP_S_DIAG || E * P == 1, "hb_sgp_predict_cov: a full-rank S (s_kind TRIL) needs E P == 1 (E=%ld P=%ld)",
             E, P);
  HB_REQUIRE(sx == 0 || sx == n * d, "hb_sgp_predict_cov: x is shared (sx = 0) or [E, n, d] (sx = n d), got sx=%ld", sx);
  HB_REQUIRE(x && z && ell && W && s && cov, "hb_sgp_predict_cov: NULL pointer");
  HB_REQUIRE(E * P <= 65535, "hb_sgp_predict_cov: too many experts x latent functions (E P = %ld)", E * P);
  HB_REQUIRE(n * d < 2147483647L, "hb_sgp_predict_cov: matrix too large");
  HB_REQUIRE_RBF_MODEL("hb_sgp_predict_cov", "has a closed-form covariance", kind, dl, d, Wf, M);
  const long need = hb_sgp_predict_cov_ws_elems(E, n, M, P, s_kind, (int)sizeof(T));
  HB_REQUIRE(need == 0 || (ws && (uintptr_t)ws % 16 == 0),
             "hb_sgp_predict_cov: needs a 16-byte aligned workspace of %ld elements", need);
  if (n == 0) return 0;
  const long nt = (n + COV_BT - 1) / COV_BT;
  HB_REQUIRE(nt * (nt + 1) / 2 < 2147483647L, "hb_sgp_predict_cov: n=%ld too large", n);

  // pass 1: A [E, M, n]; C = S^T A [M, n] (full-rank S); a2 [E, n] (DIAGONAL)
  T* A = ws;
  T* C = s_kind == HB_SGP_S_TRIL ? ws + hb_round64(E * M * n) : nullptr;   // (E = 1)
  const long gap = hb_round64(E * M * n) - E * M * n;
  T* a2 = ws + hb_round64(E * M * n) + (C ? hb_round64(M * n) : 0);
  int rc = hb_sgp_A(kind, x, sx, z, ell, dl, W, Wf, A, E, n, M, d, st);
  if (rc) return rc;
  if (C) {
    rc = hb_matmul(s, A, C, 1, M, n, M, M, n, n, 0, 0, 0, 1, st);   // C = S^T A
    if (rc) return rc;
  }
  if (mode == HB_SGP_DIAGONAL) {
    hipLaunchKernelGGL((pred_cov_a2_kernel<T>), dim3(hb_stream_grid(E * n, 256)), dim3(256), 0, st, A, a2, E, M, n);
    HB_LAUNCH_CHECK();
  }
  // pass 2: K rows [kbeg, kend); a full-rank S outside FULLRANK gives the A rows weight 0: only C's rows remain
  const long kbeg = s_kind == HB_SGP_S_TRIL && mode != HB_SGP_FULLRANK ? M : 0;
  const long kend = s_kind == HB_SGP_S_TRIL ? 2 * M : M;
  const T* sd = s_kind == HB_SGP_S_DIAG ? s : nullptr;
  if constexpr (sizeof(T) == 4) {
    CovArgs a;
    a.x = x; a.sx = sx; a.ell = ell; a.dl = dl; a.d = d; a.A = A; a.gap = gap; a.s = sd;
    a.a2 = mode == HB_SGP_DIAGONAL ? a2 : nullptr;
    a.mode = mode; a.jitter = (float)jitter; a.cov = cov; a.n = n; a.M = M; a.P = P; a.kbeg = kbeg; a.kend = kend;
    hipLaunchKernelGGL(sgp_predict_cov_kernel, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)(E * P), 1), dim3(COV_THREADS), 0,
                       st, a);
    HB_LAUNCH_CHECK();
  } else {
    const long nb = (n + COV_F64_T - 1) / COV_F64_T;
    HB_REQUIRE(nb <= 65535, "hb_sgp_predict_cov: n=%ld too large for the fp64 form", n);
    hipLaunchKernelGGL(sgp_predict_cov_f64_kernel, dim3((unsigned)nb, (unsigned)nb, (unsigned)(E * P)),
                       dim3(COV_F64_T, COV_F64_T), 0, st, x, sx, ell, dl, d, A, gap, sd, mode == HB_SGP_DIAGONAL ? a2 : nullptr,
                       mode, jitter, cov, n, M, P, kbeg, kend);
    HB_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int hb_sgp_predict_cov_f32(int kind, const float* x, long sx, const float* z, const float* ell, long dl,
                                      const float* W, const float* Wfrag, const float* s, int s_kind, int mode, double jitter,
                                      float* cov, long E, long n, long M, long d, long P, float* ws, void* stream) {
  return sgp_predict_cov<float>(kind, x, sx, z, ell, dl, W, Wfrag, s, s_kind, mode, jitter, cov, E, n, M, d, P, ws,
                                (hipStream_t)stream);
}
extern "C" int hb_sgp_predict_cov_f64(int kind, const double* x, long sx, const double* z, const double* ell, long dl,
                                      const double* W, const double* Wfrag, const double* s, int s_kind, int mode,
                                      double jitter, double* cov, long E, long n, long M, long d, long P, double* ws,
                                      void* stream) {
  return sgp_predict_cov<double>(kind, x, sx, z, ell, dl, W, Wfrag, s, s_kind, mode, jitter, cov, E, n, M, d, P, ws,
                                 (hipStream_t)stream);
}
