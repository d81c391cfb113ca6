// Sufficient statistics of the whole data set for the closed-form optimal q(u) and the collapsed bound
// (hb_sgp_stats_*, include/henbun_hip.h).
//
// With A = Lm^-1 K(z, X) [M, N] (the A of hb_sgp_fwd; W = Lm^-1 given):
//     Phi = A A^T [M, M],   b = (A Y)^T [P, M],   yy_p = sum_j Y_jp^2,   a2sum = tr Phi = sum_j sum_m A_mj^2.
// Outputs are double whatever the input type: Lambda = I + (k_var / var) Phi has eigenvalues from 1 to about N / var, so
// an error that grows with N in Phi would reach the directions the data barely inform.  Precision decision (measured,
// profiles/sgp_stats_errors.txt, tools/sgp_stats_errors.py): the fp32 entry forms A in FLOAT32 with hb_sgp_A_f32 -- at
// N = 1e5, M = 128, jitter 1e-5 float32 A keeps min eig(Lambda) at 0.9984 (float64: 1.0000) and moves the predictive
// mean by 2.4e-4; the up-converted hb_sgp_A_f64 form the issue held in reserve is not needed.
//
// One streaming pass, columns in chunks of at most ST_CHUNK (A of the whole data set is never held; the workspace does
// not depend on N beyond one chunk).  Per chunk:
//   1. A_c [M, nc] -> workspace, by hb_sgp_A_* (from Wfrag when given).
//   2. fp32, M % 32 == 0, P <= 4: sgp_stats_syrk_kernel, a split-K symmetric rank-nc update on MFMA.  Grid = (lower-
//      triangle 128 x 128 tiles of Phi) x (K-splits of the chunk), about three workgroups per CU; 256 threads = 2 x 2 waves of
//      32x32x2 MFMAs.  Both operands are row panels of A_c, contiguous along K: 16-byte global loads into registers one
//      stage ahead, 16-byte LDS stores into [row][K] panels (row stride 20 floats: conflict-free 16-byte reads), two LDS
//      stages.  The order of K inside a stage is permuted (lane half hl takes k = 8 s + 4 hl + c) so that one 16-byte LDS
//      read feeds four MFMAs; a sum does not care.  The fp32 accumulator never sums more than one K-split (at most
//      ks = 432 columns at M = 512); its tile goes to the workspace as a partial.  The workgroups of the diagonal tiles also
//      hold rows i0 .. i0 + 127 of A_c in LDS: they form their share of b_c = A_c Y_c from it (VALU, Y_c staged beside
//      the panels) -- b is not a second pass over A_c.
//   3. sgp_stats_fold_kernel: Phi += sum over the splits, in double, in split order; the same for b.  A launch boundary
//      is the only synchronisation (no atomics, no flags): every run adds the same numbers in the same order, so results
//      are bitwise reproducible.  Cost: the partials are written and read once, 4 bytes x 128^2 x tiles x splits per
//      chunk (50 MB at M = 512 against the 64 MB of A_c itself).
//   Other shapes (fp64; M % 32 != 0; P > 4): plain FMA loops over the chunk in double, one thread per lower-triangle
//   element (parity, not speed).
// After the last chunk: the strict upper triangle is copied from the lower one (Phi bitwise symmetric) and a2sum is the
// fold of diag(Phi) -- not computed a second way.  yy is summed chunk by chunk by one block of the fold launch.
#include "host_calls.cuh"   // hb_round64, hb_chunk_cols, hb_sgp_A, HB_REQUIRE_RBF_MODEL

#define ST_BT 128                // output tile (rows = cols)
#define ST_KB 16                 // K columns per LDS stage
#define ST_LD 20                 // row stride of an LDS panel [128][16 + 4]
#define ST_THREADS 256           // 4 waves in 2 x 2; wave (wi, wj) owns rows 64 wi .., cols 64 wj .. of the tile
#define ST_PANEL (ST_BT * ST_LD)
#define ST_STAGE (2 * ST_PANEL)  // row panel + column panel
#define ST_PMAX 4                // latent functions the MFMA form carries b for
#define ST_NXCD 8
#define ST_CHUNK 32768L          // columns per chunk (at most)
#define ST_CHUNK_ELEMS (1L << 24)  // elements of A_c (at most)
#define ST_TARGET_WG 768         // tiles x splits aimed at: three workgroups per CU, all resident at once (measured best)
#define ST_TILE (ST_BT * ST_BT)
#define ST_PLAIN_T 16

struct StatsArgs {
  const float* A;   // A_c [M, nc], row stride ld
  long ld;
  const float* Y;   // Y_c [nc, P]
  long P, M, nc;
  long ks;          // columns per K-split (multiple of ST_KB)
  long T, nt;       // lower-triangle tiles, tile rows
  float* part;      // [splits][T][128 x 128]
  float* bpart;     // [splits][nt][P][128]
  const float* w;   // WGT: weights of the chunk's columns [nc], 16-byte aligned
};

// WGT (hb_sgp_wstats_*): Phi_w = A diag(w) A^T.  The column panel is staged as A_c diag(w) -- one 16-byte load of w per
// thread and stage, the product taken on the way from the global load to LDS -- and the row panel as A_c itself, on the
// diagonal tiles too, so weights of either sign and zeros need no root; b comes from the unweighted row panel.
template <bool VEC, bool WGT>
__global__ void __launch_bounds__(ST_THREADS) sgp_stats_syrk_kernel(StatsArgs a) {
  typedef Mma<float> MM;
  __shared__ __attribute__((aligned(16))) float smem[2 * ST_STAGE];
  __shared__ float ys[2][ST_KB * ST_PMAX];
  // XCD-aware remap (cdna_hip_programming.md T1, bijective form; as sgp_predict_cov_kernel): the blocks one XCD receives
  // take a contiguous run of (split, tile) pairs, tile fastest: the tiles of one split share its row panels in that L2.
  long lin;
  {
    const long nwg = gridDim.x, bid = blockIdx.x, q = nwg / ST_NXCD, r = nwg % ST_NXCD, xcd = bid % ST_NXCD;
    lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / ST_NXCD;
  }
  const long sp = lin / a.T, t = lin % a.T;
  long ti = (long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (ti * (ti + 1) / 2 > t) --ti;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  const long tj = t - ti * (ti + 1) / 2;
  const long i0 = ti * ST_BT, j0 = tj * ST_BT;
  const bool diag = ti == tj;
  const long kbeg = sp * a.ks, kend = kbeg + a.ks < a.nc ? kbeg + a.ks : a.nc;
  const int tid = threadIdx.x, lane = tid & 63, li = lane & 31, hl = lane >> 5;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), wi = w >> 1, wj = w & 1;

  // staging: thread tid loads 4 consecutive k of rows tid / 4 and tid / 4 + 64 of each panel
  const int lr = tid >> 2, lk = (tid & 3) * 4;
  const int nY = ST_KB * (int)a.P;
  float4 ri[2], rj[2];
  float yreg = 0.f;
  auto load4 = [&](long row, long k) -> float4 {
    float4 v = {0.f, 0.f, 0.f, 0.f};
    if (row < a.M && k < kend) {
      const float* p = a.A + row * a.ld + k;
      if (VEC) {
        v = *(const float4*)p;   // ld, ks, k are multiples of 4 and kend is nc or a multiple of 16: k + 3 < kend
      } else {
        v.x = p[0];
        if (k + 1 < kend) v.y = p[1];
        if (k + 2 < kend) v.z = p[2];
        if (k + 3 < kend) v.w = p[3];
      }
    }
    return v;
  };
  auto load = [&](long k0) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      ri[q] = load4(i0 + lr + 64 * q, k0 + lk);
      rj[q] = diag ? ri[q] : load4(j0 + lr + 64 * q, k0 + lk);
    }
    if (WGT) {
      const long k = k0 + lk;
      float4 wq = {0.f, 0.f, 0.f, 0.f};
      if (k < kend) {
        if (VEC) {
          wq = *(const float4*)(a.w + k);
        } else {
          wq.x = a.w[k];
          if (k + 1 < kend) wq.y = a.w[k + 1];
          if (k + 2 < kend) wq.z = a.w[k + 2];
          if (k + 3 < kend) wq.w = a.w[k + 3];
        }
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        rj[q].x *= wq.x;
        rj[q].y *= wq.y;
        rj[q].z *= wq.z;
        rj[q].w *= wq.w;
      }
    }
    if (diag && tid < nY) yreg = k0 + tid / a.P < kend ? a.Y[k0 * a.P + tid] : 0.f;
  };
  auto store = [&](int buf) {
    float* Ai = smem + buf * ST_STAGE;
    float* Aj = Ai + ST_PANEL;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      *(float4*)(Ai + (lr + 64 * q) * ST_LD + lk) = ri[q];
      *(float4*)(Aj + (lr + 64 * q) * ST_LD + lk) = rj[q];
    }
    if (diag && tid < nY) ys[buf][tid] = yreg;
  };

  MM::Acc acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[u][v][r] = 0.f;
  float bacc[ST_PMAX] = {0.f, 0.f, 0.f, 0.f};

  const long ns = (kend - kbeg + ST_KB - 1) / ST_KB;
  if (ns > 0) {
    load(kbeg);
    store(0);
  }
  __syncthreads();
  for (long st = 0; st < ns; ++st) {
    if (st + 1 < ns) load(kbeg + (st + 1) * ST_KB);   // in flight during this stage's MFMAs
    const float* Ai = smem + (st & 1) * ST_STAGE;
    const float* Aj = Ai + ST_PANEL;
#pragma unroll
    for (int s2 = 0; s2 < ST_KB / 8; ++s2) {
      // 32x32x2: lane (li, hl) supplies A-operand [i = li][k slot hl] and B-operand [k slot hl][j = li]; slot hl of step c
      // is column 8 s2 + 4 hl + c of the stage for both operands
      const float4 a0 = *(const float4*)(Ai + (64 * wi + li) * ST_LD + 8 * s2 + 4 * hl);
      const float4 a1 = *(const float4*)(Ai + (64 * wi + 32 + li) * ST_LD + 8 * s2 + 4 * hl);
      const float4 b0 = *(const float4*)(Aj + (64 * wj + li) * ST_LD + 8 * s2 + 4 * hl);
      const float4 b1 = *(const float4*)(Aj + (64 * wj + 32 + li) * ST_LD + 8 * s2 + 4 * hl);
      const float av0[4] = {a0.x, a0.y, a0.z, a0.w}, av1[4] = {a1.x, a1.y, a1.z, a1.w};
      const float bv0[4] = {b0.x, b0.y, b0.z, b0.w}, bv1[4] = {b1.x, b1.y, b1.z, b1.w};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        acc[0][0] = MM::mma(av0[c], bv0[c], acc[0][0]);
        acc[0][1] = MM::mma(av0[c], bv1[c], acc[0][1]);
        acc[1][0] = MM::mma(av1[c], bv0[c], acc[1][0]);
        acc[1][1] = MM::mma(av1[c], bv1[c], acc[1][1]);
      }
    }
    if (diag) {
      // b: threads 2 r and 2 r + 1 take columns 0..7 and 8..15 of row r of the stage
      const int h = tid & 1;
      const float* Ar = Ai + (tid >> 1) * ST_LD + 8 * h;
      const float4 v0 = *(const float4*)Ar, v1 = *(const float4*)(Ar + 4);
      const float av[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
      const float* yb = ys[st & 1] + 8 * h * a.P;
#pragma unroll
      for (int c = 0; c < 8; ++c)
#pragma unroll
        for (int p = 0; p < ST_PMAX; ++p)
          if (p < a.P) bacc[p] = __builtin_fmaf(av[c], yb[c * a.P + p], bacc[p]);
    }
    if (st + 1 < ns) store((st + 1) & 1);
    __syncthreads();
  }

  // the partial tile, whole (rows / columns beyond M hold zeros; the fold reads the valid lower triangle only)
  float* out = a.part + (sp * a.T + t) * ST_TILE;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        out[(64 * wi + 32 * u + MM::acc_row(lane, r)) * ST_BT + 64 * wj + 32 * v + MM::acc_col(lane)] = acc[u][v][r];
  if (diag) {
#pragma unroll
    for (int p = 0; p < ST_PMAX; ++p) {
      const float s = bacc[p] + __shfl_xor(bacc[p], 1, 64);
      if (p < a.P && !(tid & 1)) a.bpart[((sp * a.nt + ti) * a.P + p) * ST_BT + (tid >> 1)] = s;
    }
  }
}

// yy[p] (+)= sum_j Y_c[j, p]^2 over one chunk: one block of 256 threads, a fixed order (rides in the last block of the
// fold / plain b launch of the chunk)
template <typename T>
__device__ __forceinline__ void st_yy_block(const T* __restrict__ Y, long nc, long P, double* __restrict__ yy, int accumulate,
                                            double* red) {
  for (long p = 0; p < P; ++p) {
    double s = 0.0;
    for (long j = threadIdx.x; j < nc; j += blockDim.x) {
      const double y = (double)Y[j * P + p];
      s = __builtin_fma(y, y, s);
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) yy[p] = accumulate ? yy[p] + s : s;
  }
}

// Phi (lower triangle) and b take the sum of the splits' partials in double, split order; `accumulate` = 0: first chunk.
// blocks [0, 64 T): one element of one tile per thread; the blocks after them: one entry of b per thread; the last
// block: yy of the chunk (yy == NULL, the weighted form: nothing).
__global__ void __launch_bounds__(256) sgp_stats_fold_kernel(const float* __restrict__ part, const float* __restrict__ bpart,
                                                             long T, long nt, long splits, long M, long P,
                                                             double* __restrict__ Phi, double* __restrict__ b,
                                                             const float* __restrict__ Y, long nc, double* __restrict__ yy,
                                                             int accumulate) {
  __shared__ double red[16];
  const long blk = blockIdx.x;
  if (blk == (long)gridDim.x - 1) {
    if (yy) st_yy_block(Y, nc, P, yy, accumulate, red);
  } else if (blk < 64 * T) {
    const long t = blk / 64, e = (blk % 64) * 256 + threadIdx.x;
    long ti = (long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (ti * (ti + 1) / 2 > t) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    const long tj = t - ti * (ti + 1) / 2;
    const long gi = ti * ST_BT + e / ST_BT, gj = tj * ST_BT + e % ST_BT;
    if (gi >= M || gj > gi) return;
    double s = 0.0;
    for (long k = 0; k < splits; ++k) s += (double)part[(k * T + t) * ST_TILE + e];
    Phi[gi * M + gj] = accumulate ? Phi[gi * M + gj] + s : s;
  } else {
    const long q = (blk - 64 * T) * 256 + threadIdx.x;
    if (q >= P * M) return;
    const long p = q / M, m = q % M;
    double s = 0.0;
    for (long k = 0; k < splits; ++k) s += (double)bpart[((k * nt + m / ST_BT) * P + p) * ST_BT + m % ST_BT];
    b[q] = accumulate ? b[q] + s : s;
  }
}

// plain forms (fp64; fp32 shapes the MFMA form does not take): the whole chunk per thread, in double
template <typename T, bool WGT>
__global__ void __launch_bounds__(ST_PLAIN_T * ST_PLAIN_T) sgp_stats_plain_phi_kernel(const T* __restrict__ A, long ld, long M,
                                                                                     long nc, const T* __restrict__ w,
                                                                                     double* __restrict__ Phi,
                                                                                     int accumulate) {
  if (blockIdx.x > blockIdx.y) return;   // the tile lies above the diagonal
  const long i = (long)blockIdx.y * ST_PLAIN_T + threadIdx.y, j = (long)blockIdx.x * ST_PLAIN_T + threadIdx.x;
  if (i >= M || j > i) return;
  const T* ai = A + i * ld;
  const T* aj = A + j * ld;
  double s = 0.0;
  for (long k = 0; k < nc; ++k)   // WGT: the weight on the column operand
    s = __builtin_fma((double)ai[k], WGT ? (double)w[k] * (double)aj[k] : (double)aj[k], s);
  Phi[i * M + j] = accumulate ? Phi[i * M + j] + s : s;
}
template <typename T>
__global__ void __launch_bounds__(256) sgp_stats_plain_b_kernel(const T* __restrict__ A, long ld, const T* __restrict__ Y, long M,
                                                                long P, long nc, double* __restrict__ b,
                                                                double* __restrict__ yy, int accumulate) {
  __shared__ double red[16];
  if (blockIdx.x == gridDim.x - 1) {   // the last block: yy of the chunk
    if (yy) st_yy_block(Y, nc, P, yy, accumulate, red);
    return;
  }
  const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= P * M) return;
  const long p = q / M, m = q % M;
  const T* am = A + m * ld;
  double s = 0.0;
  for (long k = 0; k < nc; ++k) s = __builtin_fma((double)am[k], (double)Y[k * P + p], s);
  b[q] = accumulate ? b[q] + s : s;
}

// the strict upper triangle takes the lower one's bits; block 0 also folds diag(Phi) into a2sum
__global__ void __launch_bounds__(256) sgp_stats_finish_kernel(double* __restrict__ Phi, long M, double* __restrict__ a2sum) {
  __shared__ double red[16];
  const long total = M * M, stride = (long)gridDim.x * blockDim.x;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += stride) {
    const long i = q / M, j = q % M;
    if (j > i) Phi[q] = Phi[j * M + i];
  }
  if (blockIdx.x == 0) {
    double s = 0.0;
    for (long i = threadIdx.x; i < M; i += blockDim.x) s += Phi[i * M + i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) a2sum[0] = s;
  }
}

static inline long st_chunk_cols(long N, long M) { return hb_chunk_cols(ST_CHUNK_ELEMS, M, ST_CHUNK, N); }   // N >= 1
static inline bool st_is_mfma(long M, long P, int dbytes) { return dbytes == 4 && M % 32 == 0 && P <= ST_PMAX; }
// K-splits of a chunk of nc columns: tiles x splits about ST_TARGET_WG, a split at least one stage long
// (never more than st_max_splits, which sizes the workspace)
static inline long st_max_splits(long T) {
  long wg = hb_debug_get("sgp_stats_target_wg", ST_TARGET_WG);   // diagnostic: another tiles x splits target
  wg = wg < 1 ? 1 : (wg > 4096 ? 4096 : wg);
  return wg / T > 1 ? wg / T : 1;
}
static inline void st_split(long M, long nc, long* T, long* nt, long* ks, long* splits) {
  *nt = (M + ST_BT - 1) / ST_BT;
  *T = *nt * (*nt + 1) / 2;
  const long S = st_max_splits(*T);
  long k = (nc + S - 1) / S;
  k = (k + ST_KB - 1) / ST_KB * ST_KB;
  *ks = k;
  *splits = (nc + k - 1) / k;
}

extern "C" long hb_sgp_stats_ws_elems(long N, long M, long d, long P, int dtype_bytes) {
  (void)d;
  if (N <= 0 || M <= 0 || P <= 0) return 0;
  const long nc = st_chunk_cols(N, M);
  long need = hb_round64(M * nc);
  if (st_is_mfma(M, P, dtype_bytes)) {
    long T, nt, ks, splits;
    st_split(M, nc, &T, &nt, &ks, &splits);
    need += hb_round64(st_max_splits(T) * T * ST_TILE) + hb_round64(st_max_splits(T) * nt * P * ST_BT);
  }
  return need;
}

// hb_sgp_stats_* (WGT false: w NULL) and hb_sgp_wstats_* (WGT true: Y is r [N], P = 1, yy NULL) share every launch.
// hb_sgp_mwstats_* is the weighted form for C weight sets: set c reads w + c ldw and r + c ldw and writes Phi + c M^2,
// b + c M, a2sum + c.  A_c is formed ONCE per chunk; the rank update and its fold then run set by set over it, through the
// one set of partial tiles (the stream orders fold c before update c + 1), so set c sees the launches -- chunk size,
// K-splits, fold order, mirror -- a hb_sgp_wstats_* call with its w and r would make, and returns its bits.  C = 1: the
// launches as they were.
template <typename T, bool WGT>
static int sgp_stats(const char* who, int kind, const T* X, const T* Y, const T* w, const T* z, const T* ell, long dl, const T* W,
                     const T* Wf, double* Phi, double* b, double* yy, double* a2sum, long N, long M, long d, long P, T* ws,
                     hipStream_t st, long C = 1, long ldw = 0) {
  HB_REQUIRE(N >= 1 && M >= 1 && d >= 1 && P >= 1, "%s: bad extents (N=%ld M=%ld d=%ld P=%ld)", who, N, M, d, P);
  HB_REQUIRE(X && Y && z && ell && W && (!WGT || w), "%s: NULL input pointer", who);
  HB_REQUIRE(Phi && b && (WGT || yy) && a2sum, "%s: NULL output pointer", who);
  HB_REQUIRE(M <= 16384, "%s: M=%ld too large", who, M);
  HB_REQUIRE_RBF_MODEL(who, "is supported", kind, dl, d, Wf, M);
  HB_REQUIRE(!WGT || (uintptr_t)w % 16 == 0, "%s: the weights need 16-byte alignment", who);
  HB_REQUIRE(C >= 1 && (C == 1 || (WGT && P == 1 && ldw >= N)), "%s: bad weight sets (C=%ld ldw=%ld N=%ld)", who, C, ldw, N);
  for (long c = 1; c < C; ++c)
    HB_REQUIRE((uintptr_t)(w + c * ldw) % 16 == 0, "%s: every row of the weights needs 16-byte alignment (ldw=%ld)", who, ldw);
  const long need = hb_sgp_stats_ws_elems(N, M, d, P, (int)sizeof(T));
  HB_REQUIRE(ws && (uintptr_t)ws % 16 == 0, "%s: needs a 16-byte aligned workspace of %ld elements", who, need);
  const long nc_max = st_chunk_cols(N, M);
  const bool mfma = st_is_mfma(M, P, (int)sizeof(T));
  T* Abuf = ws;
  const bool no_A = hb_debug_get("sgp_stats_no_A", 0) != 0, no_syrk = hb_debug_get("sgp_stats_no_syrk", 0) != 0;

  for (long c0 = 0; c0 < N; c0 += nc_max) {
    const long nc = N - c0 < nc_max ? N - c0 : nc_max;
    const int accumulate = c0 > 0;
    // diagnostic switches (tools/bench_sgp_stats.py times the two passes apart): without the A pass the second pass runs
    // on whatever the workspace holds, without the second pass Phi and b are not written
    if (!no_A) {
      const int rc = hb_sgp_A(kind, X + c0 * d, 0, z, ell, dl, W, Wf, Abuf, 1, nc, M, d, st);
      if (rc) return rc;
    }
    if (no_syrk) continue;
    for (long c = 0; c < C; ++c) {
      const T* Yc = Y + c * ldw + c0 * P;                       // C > 1: P == 1
      const T* wc = WGT ? w + c * ldw + c0 : nullptr;           // c0 is a multiple of 32: the chunk's weights stay 16-byte aligned
      double* Phic = Phi + c * M * M;
      double* bc = b + c * P * M;
      if constexpr (sizeof(T) == 4) {
        if (mfma) {
          long Tn, nt, ks, splits;
          st_split(M, nc, &Tn, &nt, &ks, &splits);   // splits <= st_max_splits(Tn): the workspace holds them
          StatsArgs a;
          a.A = Abuf; a.ld = nc; a.Y = Yc; a.P = P; a.M = M; a.nc = nc; a.ks = ks; a.T = Tn; a.nt = nt;
          a.w = wc;
          a.part = ws + hb_round64(M * nc_max);
          a.bpart = a.part + hb_round64(st_max_splits(Tn) * Tn * ST_TILE);
          const dim3 grid((unsigned)(Tn * splits), 1, 1);
          if (nc % 4 == 0)
            hipLaunchKernelGGL((sgp_stats_syrk_kernel<true, WGT>), grid, dim3(ST_THREADS), 0, st, a);
          else
            hipLaunchKernelGGL((sgp_stats_syrk_kernel<false, WGT>), grid, dim3(ST_THREADS), 0, st, a);
          HB_LAUNCH_CHECK();
          const long fb = 64 * Tn + (P * M + 255) / 256 + 1;
          hipLaunchKernelGGL(sgp_stats_fold_kernel, dim3((unsigned)fb), dim3(256), 0, st, a.part, a.bpart, Tn, nt, splits, M, P,
                             Phic, bc, a.Y, nc, yy, accumulate);
          HB_LAUNCH_CHECK();
          continue;
        }
      }
      const long nb = (M + ST_PLAIN_T - 1) / ST_PLAIN_T;
      hipLaunchKernelGGL((sgp_stats_plain_phi_kernel<T, WGT>), dim3((unsigned)nb, (unsigned)nb, 1), dim3(ST_PLAIN_T, ST_PLAIN_T),
                         0, st, Abuf, nc, M, nc, wc, Phic, accumulate);
      HB_LAUNCH_CHECK();
      hipLaunchKernelGGL((sgp_stats_plain_b_kernel<T>), dim3((unsigned)((P * M + 255) / 256 + 1)), dim3(256), 0, st, Abuf, nc, Yc,
                         M, P, nc, bc, yy, accumulate);
      HB_LAUNCH_CHECK();
    }
  }
  for (long c = 0; c < C; ++c) {
    hipLaunchKernelGGL(sgp_stats_finish_kernel, dim3(hb_stream_grid(M * M, 256)), dim3(256), 0, st, Phi + c * M * M, M, a2sum + c);
    HB_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int hb_sgp_stats_f32(int kind, const float* X, const float* Y, const float* z, const float* ell, long dl,
                                const float* W, const float* Wfrag, double* Phi, double* b, double* yy, double* a2sum, long N,
                                long M, long d, long P, float* ws, void* stream) {
  return sgp_stats<float, false>("hb_sgp_stats", kind, X, Y, nullptr, z, ell, dl, W, Wfrag, Phi, b, yy, a2sum, N, M, d, P, ws, (hipStream_t)stream);
}
extern "C" int hb_sgp_stats_f64(int kind, const double* X, const double* Y, const double* z, const double* ell, long dl,
                                const double* W, const double* Wfrag, double* Phi, double* b, double* yy, double* a2sum,
                                long N, long M, long d, long P, double* ws, void* stream) {
  return sgp_stats<double, false>("hb_sgp_stats", kind, X, Y, nullptr, z, ell, dl, W, Wfrag, Phi, b, yy, a2sum, N, M, d, P, ws, (hipStream_t)stream);
}

// Weighted statistics of the natural-gradient step on q(u) (SparseGP.natgrad_q): Phi_w = A diag(w) A^T, b = (A r)^T,
// tr Phi_w -- hb_sgp_stats_* with the weight on the column operand and r in the place of Y (P = 1).
extern "C" long hb_sgp_wstats_ws_elems(long N, long M, long d, int dtype_bytes) {
  return hb_sgp_stats_ws_elems(N, M, d, 1, dtype_bytes);
}
extern "C" int hb_sgp_wstats_f32(int kind, const float* X, const float* w, const float* r, const float* z, const float* ell,
                                 long dl, const float* W, const float* Wfrag, double* Phi, double* b, double* tr, long N, long M,
                                 long d, float* ws, void* stream) {
  return sgp_stats<float, true>("hb_sgp_wstats", kind, X, r, w, z, ell, dl, W, Wfrag, Phi, b, nullptr, tr, N, M, d, 1, ws,
                                (hipStream_t)stream);
}
extern "C" int hb_sgp_wstats_f64(int kind, const double* X, const double* w, const double* r, const double* z, const double* ell,
                                 long dl, const double* W, const double* Wfrag, double* Phi, double* b, double* tr, long N,
                                 long M, long d, double* ws, void* stream) {
  return sgp_stats<double, true>("hb_sgp_wstats", kind, X, r, w, z, ell, dl, W, Wfrag, Phi, b, nullptr, tr, N, M, d, 1, ws,
                                 (hipStream_t)stream);
}

// Weighted statistics for C weight sets from ONE A (hb_sgp_mwstats_*; the data pass of a natural-gradient step on C
// independent q(u_c) that share z, the lengthscales and W: SparseGP.natgrad_q with a multi-latent likelihood).  The
// partial tiles are reused set by set, so the workspace is that of hb_sgp_wstats_*, whatever C.
extern "C" long hb_sgp_mwstats_ws_elems(long N, long M, long d, long C, int dtype_bytes) {
  (void)C;
  return hb_sgp_stats_ws_elems(N, M, d, 1, dtype_bytes);
}
extern "C" int hb_sgp_mwstats_f32(int kind, const float* X, const float* w, const float* r, long ldw, const float* z,
                                  const float* ell, long dl, const float* W, const float* Wfrag, double* Phi, double* b, double* tr,
                                  long N, long M, long d, long C, float* ws, void* stream) {
  return sgp_stats<float, true>("hb_sgp_mwstats", kind, X, r, w, z, ell, dl, W, Wfrag, Phi, b, nullptr, tr, N, M, d, 1, ws,
                                (hipStream_t)stream, C, ldw);
}
extern "C" int hb_sgp_mwstats_f64(int kind, const double* X, const double* w, const double* r, long ldw, const double* z,
                                  const double* ell, long dl, const double* W, const double* Wfrag, double* Phi, double* b,
                                  double* tr, long N, long M, long d, long C, double* ws, void* stream) {
  return sgp_stats<double, true>("hb_sgp_mwstats", kind, X, r, w, z, ell, dl, W, Wfrag, Phi, b, nullptr, tr, N, M, d, 1, ws,
                                 (hipStream_t)stream, C, ldw);
}
