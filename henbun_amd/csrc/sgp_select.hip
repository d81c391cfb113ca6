// Greedy conditional-variance selection of inducing points: a pivoted incomplete Cholesky of K(X, X)
// (hb_sgp_select_*, include/henbun_hip.h; Burt, Rasmussen, van der Wilk 2020).
//
// State: dvar [N] (the conditional variance of every point given the points chosen so far, kdiag = 1 at the start) and
// the history C [M, N], row j = column j of the pivoted factor.  For j = 0 .. M - 1:
//     i_j = argmax_i dvar_i (exact ties: the lowest index);  stop if dvar_{i_j} <= threshold;  pivots_j = dvar_{i_j};
//     C[j, i] = (k(x_i, x_{i_j}) - sum_{t < j} C[t, i] C[t, i_j]) / sqrt(pivots_j);
//     dvar_i <- max(dvar_i - C[j, i]^2, 0);  dvar_{i_j} <- 0.
// trace = sum_i dvar_i at the end = tr(K_XX - K_XZ K_ZZ^-1 K_ZX), in double, a fixed order.
//
// The history form was kept ("Inducing-point selection"): ONE launch per chosen point, no host
// synchronisation, no atomics, no grid-wide barrier inside a launch.  Launch j (sgp_select_step_kernel):
//   1. every workgroup folds the (max, lowest index) partials launch j - 1 left, redundantly -- the fold is a pure
//      function of the partial slots (greater value wins, equal values: the lower index), so every workgroup arrives at
//      the same i_j and the kernel boundary is the only synchronisation.  Launch 0 skips the fold: i_0 = 0, pivot = 1.
//   2. the pivot's history C[0 .. j-1, i_j] goes to LDS once per workgroup (j strided 4 / 8-byte reads).
//   3. each thread owns 16 bytes of points (4 floats / 2 doubles) of a tile of blockDim.x x 16 bytes; it streams
//      C[t, i ..] for t = 0 .. j - 1 with 16-byte loads, 8 rows of t in flight per step, times the LDS-broadcast pivot
//      entry (the sum runs in t order, one fused multiply-add per term), writes C[j, i ..] and the downdated dvar with
//      16-byte stores and reduces (max, lowest index) through the wave, then LDS, into the workgroup's partial slot.
//      The partial slots are double-buffered by launch parity: launch j reads set (j - 1) & 1 and writes set j & 1.
//   4. workgroup 0 alone writes idx[j], pivots[j].
// Early stop: the workgroups that find max dvar <= threshold write the sentinel -1 into their partial slots instead of
// streaming (dvar >= 0 always, so a real fold is never negative); workgroup 0 writes count = j and idx[j ..] = -1,
// pivots[j ..] = 0.  Every later launch folds -1, passes the sentinel on and returns at once.
// The last launch (sgp_select_finish_kernel, one workgroup) writes count = M unless the sentinel says it is frozen, and
// trace = sum dvar: thread-strided partial sums in double, then the block fold -- the same order every run.
//
// Traffic: row j reads j rows of C: N M^2 / 2 elements in all (524 GB at N = 1e6, M = 512, fp32): memory-bound.
// Workspace: C [M, ld], dvar [ld], the partial slots; ld = N rounded up to 64 (the pad columns hold zeros).
#include "common.cuh"
#include "gram_value.cuh"
#include "../../include/henbun_hip.h"

#define SEL_MAX_WG 2048          // workgroups (= partial slots per set) at most; tiles beyond are grid-strided
#define SEL_BIG_BLOCK 256
#define SEL_SMALL_BLOCK 64       // small N: one wave per workgroup so that the tiles still cover the CUs
#define SEL_BIG_MIN_TILES 512    // 256-thread workgroups from this many of their tiles on
#define SEL_MAX_M 8192           // the pivot's history sits in LDS: 64 KB in double
#define SEL_UNROLL 8             // rows of C in flight per thread
#define SEL_FIN_BLOCK 1024

template <typename T> struct SelVec;
template <> struct SelVec<float> { typedef float4 V; static constexpr int W = 4; };
template <> struct SelVec<double> { typedef double2 V; static constexpr int W = 2; };

template <typename T>
struct SelArgs {
  const T* X;
  const T* ell;
  long dl, N, M, d, ld;
  double threshold;
  T* C;            // [M, ld]
  T* dvar;         // [ld]
  T* pval;         // [2][SEL_MAX_WG]
  long* pidx;      // [2][SEL_MAX_WG]
  long* idx;       // [M]
  T* pivots;       // [M]
  long* count;     // [1]
  double* trace;   // [1]
  int kind;
};

// greater value wins; equal values: the lower index
template <typename T>
__device__ __forceinline__ void sel_better(T& bv, long& bi, T v, long i) {
  if (v > bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}
template <typename T>
__device__ __forceinline__ void sel_wave_best(T& bv, long& bi) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const T ov = __shfl_xor(bv, off, 64);
    const long long oi = __shfl_xor((long long)bi, off, 64);
    sel_better(bv, bi, ov, (long)oi);
  }
}
// (max, lowest index) over the block, valid in every thread; sv / si: one entry per wave
template <typename T>
__device__ __forceinline__ void sel_block_best(T& bv, long& bi, T* sv, long* si) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  sel_wave_best(bv, bi);
  __syncthreads();   // sv / si may still be read from an earlier call
  if (lane == 0) {
    sv[w] = bv;
    si[w] = bi;
  }
  __syncthreads();
  bv = sv[lane < nw ? lane : 0];
  bi = si[lane < nw ? lane : 0];
  sel_wave_best(bv, bi);
}

template <typename T>
__global__ void __launch_bounds__(SEL_BIG_BLOCK) sgp_select_step_kernel(SelArgs<T> a, long j) {
  typedef typename SelVec<T>::V V;
  constexpr int W = SelVec<T>::W;
  extern __shared__ __attribute__((aligned(16))) unsigned char sel_smem[];
  T* hist = (T*)sel_smem;   // [j]
  __shared__ T sv[SEL_BIG_BLOCK / 64];
  __shared__ long si[SEL_BIG_BLOCK / 64];
  const int tid = threadIdx.x;
  const long G = gridDim.x, wg = blockIdx.x;
  T* pv_out = a.pval + (j & 1) * SEL_MAX_WG;
  long* pi_out = a.pidx + (j & 1) * SEL_MAX_WG;

  // 1. the pivot of this step
  T piv = T(1);
  long ij = 0;
  if (j > 0) {
    const T* pv_in = a.pval + ((j - 1) & 1) * SEL_MAX_WG;
    const long* pi_in = a.pidx + ((j - 1) & 1) * SEL_MAX_WG;
    piv = T(-1);
    ij = 0x7fffffffffffffffL;
    for (long s = tid; s < G; s += blockDim.x) sel_better(piv, ij, pv_in[s], pi_in[s]);
    sel_block_best(piv, ij, sv, si);
  }
  const bool frozen = piv < T(0);
  if (frozen || (double)piv <= a.threshold) {
    if (tid == 0) {
      pv_out[wg] = T(-1);
      pi_out[wg] = -1;
    }
    if (frozen) return;
    // the first launch that stops
    if (j == 0) {   // nothing was written yet: dvar = kdiag, so that trace = N
      for (long i = wg * blockDim.x + tid; i < a.ld; i += G * blockDim.x) a.dvar[i] = i < a.N ? T(1) : T(0);
    }
    if (wg == 0) {
      for (long t = j + tid; t < a.M; t += blockDim.x) {
        a.idx[t] = -1;
        a.pivots[t] = T(0);
      }
      if (tid == 0) a.count[0] = j;
    }
    return;
  }
  if (wg == 0 && tid == 0) {
    a.idx[j] = ij;
    a.pivots[j] = piv;
  }

  // 2. the pivot's history
  for (long t = tid; t < j; t += blockDim.x) hist[t] = a.C[t * a.ld + ij];
  __syncthreads();

  // 3. stream the tiles
  const T rs = sqrt(piv);
  const T* xp = a.X + ij * a.d;
  T* Cj = a.C + j * a.ld;
  const long tile = (long)blockDim.x * W;
  T bv = T(-1);
  long bi = 0x7fffffffffffffffL;
  for (long i = wg * tile + (long)tid * W; i < a.ld; i += G * tile) {
    T acc[W];
#pragma unroll
    for (int v = 0; v < W; ++v) acc[v] = T(0);
    const T* cp = a.C + i;
    const long j8 = j / SEL_UNROLL * SEL_UNROLL;
    for (long t = 0; t < j8; t += SEL_UNROLL) {
      V c[SEL_UNROLL];
#pragma unroll
      for (int u = 0; u < SEL_UNROLL; ++u) c[u] = *(const V*)(cp + (t + u) * a.ld);
#pragma unroll
      for (int u = 0; u < SEL_UNROLL; ++u) {
        const T h = hist[t + u];
        const T* cu = (const T*)&c[u];
#pragma unroll
        for (int v = 0; v < W; ++v) acc[v] = hb_fma(cu[v], h, acc[v]);
      }
    }
    for (long t = j8; t < j; ++t) {
      const V c = *(const V*)(cp + t * a.ld);
      const T h = hist[t];
      const T* cu = (const T*)&c;
#pragma unroll
      for (int v = 0; v < W; ++v) acc[v] = hb_fma(cu[v], h, acc[v]);
    }
    V dv;
    T* dvp = (T*)&dv;
    if (j > 0) {
      dv = *(const V*)(a.dvar + i);
    } else {
#pragma unroll
      for (int v = 0; v < W; ++v) dvp[v] = T(1);
    }
    V cn;
    T* cnp = (T*)&cn;
#pragma unroll
    for (int v = 0; v < W; ++v) {
      const long p = i + v;
      T c = T(0), dn = T(0);
      if (p < a.N) {
        const T k = gram_value<T>(a.kind, a.X + p * a.d, xp, a.ell, a.dl, a.d);
        c = (k - acc[v]) / rs;
        dn = dvp[v] - c * c;
        dn = dn > T(0) ? dn : T(0);
        if (p == ij) dn = T(0);
        sel_better(bv, bi, dn, p);
      }
      cnp[v] = c;
      dvp[v] = dn;
    }
    *(V*)(Cj + i) = cn;
    *(V*)(a.dvar + i) = dv;
  }
  sel_block_best(bv, bi, sv, si);
  if (tid == 0) {
    pv_out[wg] = bv;
    pi_out[wg] = bi;
  }
}

template <typename T>
__global__ void __launch_bounds__(SEL_FIN_BLOCK) sgp_select_finish_kernel(SelArgs<T> a) {
  __shared__ double red[16];
  // slot 0 of the last step's set: -1 once the selection is frozen (count is written), else a real maximum (>= 0)
  if (threadIdx.x == 0 && !(a.pval[((a.M - 1) & 1) * SEL_MAX_WG] < T(0))) a.count[0] = a.M;
  double s = 0.0;
  for (long i = threadIdx.x; i < a.N; i += SEL_FIN_BLOCK) s += (double)a.dvar[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) a.trace[0] = s;
}

static inline long sel_ld(long N) { return (N + 63) & ~63L; }
// partial slots, in elements of T: [2][SEL_MAX_WG] values, then [2][SEL_MAX_WG] indices (8 bytes each)
static inline long sel_part_elems(int dbytes) { return 2L * SEL_MAX_WG + 2L * SEL_MAX_WG * 8 / dbytes; }

extern "C" long hb_sgp_select_ws_elems(long N, long M, long d, int dtype_bytes) {
  (void)d;
  if (N <= 0 || M <= 0 || (dtype_bytes != 4 && dtype_bytes != 8)) return 0;
  const long ld = sel_ld(N);
  return M * ld + ld + sel_part_elems(dtype_bytes);
}

template <typename T>
static int sgp_select(int kind, const T* X, const T* ell, long dl, long N, long M, long d, double threshold, long* idx,
                      T* pivots, long* count, double* trace, T* ws, hipStream_t st) {
  HB_REQUIRE(kind == HB_KERN_RBF, "hb_sgp_select: only the UnitRBF kernel is supported (kind=%d)", kind);
  HB_REQUIRE(N >= 1 && M >= 1 && d >= 1, "hb_sgp_select: bad extents (N=%ld M=%ld d=%ld)", N, M, d);
  HB_REQUIRE(M <= N, "hb_sgp_select: bad extents: M=%ld points cannot be chosen from N=%ld", M, N);
  HB_REQUIRE(M <= SEL_MAX_M, "hb_sgp_select: M=%ld too large (at most %d)", M, SEL_MAX_M);
  HB_REQUIRE(dl == 1 || dl == d, "hb_sgp_select: lengthscales must have 1 or d entries");
  HB_REQUIRE(threshold >= 0.0, "hb_sgp_select: threshold must be >= 0 (got %g)", threshold);   // false for a NaN too
  HB_REQUIRE(X && ell, "hb_sgp_select: NULL input pointer");
  HB_REQUIRE(idx && pivots && count && trace, "hb_sgp_select: NULL output pointer");
  const long need = hb_sgp_select_ws_elems(N, M, d, (int)sizeof(T));
  HB_REQUIRE(ws && (uintptr_t)ws % 16 == 0, "hb_sgp_select: needs a 16-byte aligned workspace of %ld elements", need);

  constexpr int W = SelVec<T>::W;
  SelArgs<T> a;
  a.X = X; a.ell = ell; a.dl = dl; a.N = N; a.M = M; a.d = d; a.ld = sel_ld(N);
  a.threshold = threshold;
  a.C = ws;
  a.dvar = ws + M * a.ld;
  a.pval = a.dvar + a.ld;                           // ld is a multiple of 64: pval and pidx are 16-byte aligned
  a.pidx = (long*)(a.pval + 2L * SEL_MAX_WG);
  a.idx = idx; a.pivots = pivots; a.count = count; a.trace = trace;
  a.kind = kind;

  long block = hb_debug_get("sgp_select_block", 0);   // diagnostic: force the workgroup size (64 or 256)
  if (block != SEL_SMALL_BLOCK && block != SEL_BIG_BLOCK)
    block = a.ld / (SEL_BIG_BLOCK * W) >= SEL_BIG_MIN_TILES ? SEL_BIG_BLOCK : SEL_SMALL_BLOCK;
  const long tile = block * W;
  long G = (a.ld + tile - 1) / tile;
  if (G > SEL_MAX_WG) G = SEL_MAX_WG;
  for (long j = 0; j < M; ++j) {
    const size_t lds = (size_t)j * sizeof(T);
    hipLaunchKernelGGL((sgp_select_step_kernel<T>), dim3((unsigned)G), dim3((unsigned)block), lds, st, a, j);
    HB_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL((sgp_select_finish_kernel<T>), dim3(1), dim3(SEL_FIN_BLOCK), 0, st, a);
  HB_LAUNCH_CHECK();
  return 0;
}

extern "C" int hb_sgp_select_f32(int kind, const float* X, const float* ell, long dl, long N, long M, long d, double threshold,
                                 long* idx, float* pivots, long* count, double* trace, float* ws, void* stream) {
  return sgp_select<float>(kind, X, ell, dl, N, M, d, threshold, idx, pivots, count, trace, ws, (hipStream_t)stream);
}
extern "C" int hb_sgp_select_f64(int kind, const double* X, const double* ell, long dl, long N, long M, long d,
                                 double threshold, long* idx, double* pivots, long* count, double* trace, double* ws,
                                 void* stream) {
  return sgp_select<double>(kind, X, ell, dl, N, M, d, threshold, idx, pivots, count, trace, ws, (hipStream_t)stream);
}
