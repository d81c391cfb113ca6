// Pieces of the column-strip sparse-GP kernels (csrc/sgp.hip, csrc/sgp_predict.hip) that every strip kernel repeats or
// that other translation units share: the strip constants, the exp2 form of the RBF value, the strip prologue (one
// column's coordinates and scale, register staging of z and u, the fp32 fill of the K block) and the fragment-major
// store of a finished 32 x 32 tile.
#ifndef HB_SGP_STRIP_CUH
#define HB_SGP_STRIP_CUH
#include "common.cuh"

// exp(-r2/2) = 2^(-(s*r)^2) with s = sqrt(log2(e)/2): the coordinate DIFFERENCE times s/ell makes the RBF value a
// single v_exp_f32 of the negated square.  The difference is taken on the raw coordinates and scaled afterwards:
// pre-scaled coordinates (round 1/2) carry |z| s/ell * 2^-24 of rounding each, which at cfg 2 (z up to 256
// lengthscales) is 1.5e-5 in a scaled difference of ~3, i.e. ~1e-4 relative in K -- two orders above the
// fp32 rounding of everything else in the step (tests/test_fp32_parity_gpu.py, profiles/r03_observed_errors.txt).
#define SGP_EXP2_SCALE 0.84932180028801904272
template <typename T> __device__ __forceinline__ T hb_exp2_neg(T x);
template <> __device__ __forceinline__ float hb_exp2_neg<float>(float x) { return __builtin_amdgcn_exp2f(-x); }
template <> __device__ __forceinline__ double hb_exp2_neg<double>(double x) { return exp2(-x); }

#define SGP_SN 32
#define SGP_SM_MAX 512
#define SGP_SLD (SGP_SM_MAX + 4)
#define SGP_DREG 4  // input dims held in registers by the operand loaders

// ---------------------------------------------------------------------------------------------------------------
// Strip prologue: K(z, x[strip]) -> LDS as Ks[column][k], M x 32, synthesised once per workgroup.  A kernel issues
// every global load (the column, the z / u requests, then loads of its own) before the first LDS store: a load -> LDS
// store loop pays one dependent round trip per iteration (five of them, ~5 us, in the first version), and z read
// straight from global inside the fill pays one per 16-byte group (~10 us).
//
// One column of the strip: thread tid works on column tid % 32; columns past n read a copy of the last one (never
// written out).  Coordinates stay RAW: value() takes the difference first and scales it afterwards (see SGP_EXP2_SCALE).
template <int D>
struct SgpStripColumn {
  float sc[D], xs[D];
  __device__ __forceinline__ void scale(const float* __restrict__ ell, long dl) {
#pragma unroll
    for (int dd = 0; dd < D; ++dd) sc[dd] = float(SGP_EXP2_SCALE) / ell[dl == 1 ? 0 : dd];
  }
  __device__ __forceinline__ void load(const float* __restrict__ x, const float* __restrict__ ell, long dl, int col0, int n,
                                       int tid) {
    const int c = col0 + (tid & 31), cc = c < n ? c : n - 1;
    scale(ell, dl);
#pragma unroll
    for (int dd = 0; dd < D; ++dd) xs[dd] = x[cc * D + dd];
  }
  // K(z_k, x) for the inducing point at zk[0 .. D-1]
  __device__ __forceinline__ float value(const float* zk) const {
    float r2 = 0.f;
#pragma unroll
    for (int dd = 0; dd < D; ++dd) {
      const float tt = (zk[dd] - xs[dd]) * sc[dd];
      r2 += tt * tt;
    }
    return hb_exp2_neg<float>(r2);
  }
};

// z [M, D] -> zs through registers: request() issues the loads, store() writes them to LDS (barrier at the caller).
template <int D, int NTH>
struct SgpStageZ {
  static constexpr int ZIT = (SGP_SM_MAX * D) / NTH;
  static_assert(ZIT >= 1, "staging loop");
  float zt[ZIT];
  __device__ __forceinline__ void request(const float* __restrict__ z, int M, int tid) {
#pragma unroll
    for (int it = 0, i = tid; it < ZIT; ++it, i += NTH) zt[it] = z[i < M * D ? i : 0];
  }
  __device__ __forceinline__ void store(float* zs, int M, int tid) const {
#pragma unroll
    for (int it = 0, i = tid; it < ZIT; ++it, i += NTH)
      if (i < M * D) zs[i] = zt[it];
  }
};
// The same for the first np <= 4 rows of this expert's u [P, M] (the column means of the epilogues).
template <int NTH>
struct SgpStageU {
  static constexpr int UIT = SGP_SM_MAX / NTH;
  static_assert(UIT >= 1, "staging loop");
  float ut[4][UIT];
  __device__ __forceinline__ void request(const float* __restrict__ u_e, int np, int M, int tid) {
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int it = 0, i = tid; it < UIT; ++it, i += NTH) ut[p][it] = p < np ? u_e[(long)p * M + (i < M ? i : 0)] : 0.f;
  }
  __device__ __forceinline__ void store(float (*us)[SGP_SM_MAX], int np, int M, int tid) const {
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int it = 0, i = tid; it < UIT; ++it, i += NTH)
        if (p < np && i < M) us[p][i] = ut[p][it];
  }
};

// fp32 fill of Ks[column][k] from the staged zs: thread (c = tid % 32, kq = tid / 32) takes the 16-byte
// groups kq, kq + NTH / 32, ... of its column.
template <int D, int NTH>
__device__ __forceinline__ void sgp_strip_fill(float (*Ks)[SGP_SLD], const float* zs, const SgpStripColumn<D>& col, int M, int tid) {
  typedef float V4 __attribute__((ext_vector_type(4)));
  const int c = tid & 31, kq = tid >> 5;
#pragma unroll 4
  for (int k4 = kq * 4; k4 < M; k4 += NTH / 8) {
    float zq[4 * D];
#pragma unroll
    for (int q = 0; q < 4 * D; q += 4) {
      const V4 zz = *reinterpret_cast<const V4*>(&zs[k4 * D + q]);
#pragma unroll
      for (int s = 0; s < 4; ++s) zq[q + s] = zz[s];
    }
    V4 v;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = col.value(&zq[q * D]);
    *reinterpret_cast<V4*>(&Ks[c][k4]) = v;
  }
}

// Fragment-major copy of a finished 32 x 32 tile (accumulator layout: column on the lane, rows in the registers) of
// an [M, n] operand of the Lbar contraction: block (row tile t, strip s) holds, for v = 0..3, lane (li, h), s' = 0..3,
//     X[32 t + li][32 s + 16 h + 4 v + s']
// i.e. the MFMA operand fragments of a contraction over the DATA axis, in load order: each of the four stores of a
// wave -- and each of the consumer's loads -- is one contiguous kilobyte.  The tile is turned row-per-lane through the
// wave's own LDS buffer (no barrier: a wave's LDS operations execute in order).  Columns past n are written as zeros.
#define SGP_TLD 36
__device__ __forceinline__ void sgp_store_frag_tile(float* __restrict__ Xf, float (*T)[SGP_TLD],
                                                    const Mma<float>::Acc& acc, long e, int nT, int nS, int tile, int strip,
                                                    int col0, int n, int lane) {
  typedef float V4 __attribute__((ext_vector_type(4)));
  const int li = lane & 31, h = lane >> 5;
#pragma unroll
  for (int r = 0; r < 16; ++r) T[Mma<float>::acc_row(lane, r)][li] = acc[r];
  float* blk = Xf + ((((long)e * nT + tile) * nS + strip) << 10) + 4 * lane;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    V4 q = *reinterpret_cast<const V4*>(&T[li][16 * h + 4 * v]);
#pragma unroll
    for (int s2 = 0; s2 < 4; ++s2)
      if (col0 + 16 * h + 4 * v + s2 >= n) q[s2] = 0.f;
    *reinterpret_cast<V4*>(blk + 256 * v) = q;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Transposed accumulators (round 3).  With the operands of the tile product swapped -- mma(K fragment, W fragment)
// instead of mma(W fragment, K fragment): the same products summed in the same order, so every element keeps its
// bits -- the 32 x 32 accumulator holds the tile TRANSPOSED: lane (li, h) owns tile ROW li and its 16 registers are
// the columns (r & 3) + 8 (r >> 2) + 4 h.  The row-per-lane view the fragment-major image and the row gradients want
// (lane (li, h): columns 16h .. 16h + 15) is then eight v_permlane32_swap with the half-wave partner -- no LDS
// transpose, no per-wave tile buffer (36.8 KB of LDS per workgroup in the first form, which also kept a second
// workgroup off the CU).
//
// sgp_acc_t_settle: the accumulator was written by MFMAs and is about to be read by inline asm, which the
// compiler's hazard recogniser does not look into: 19 wait states cover a 16-pass MFMA result (the count the compiler
// itself inserts in front of a VALU read).  The accumulator is an operand so that the MFMAs stay in front of it.
__device__ __forceinline__ void sgp_acc_t_settle(Mma<float>::Acc& acc) {
  asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc));
}
// After the call row16[4 v + s] = X[row li][16 h + 4 v + s] (acc is consumed).
__device__ __forceinline__ void sgp_acc_t_rows(Mma<float>::Acc& acc, float (&row16)[16]) {
  float lo[8], hi[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    lo[r] = acc[r], hi[r] = acc[8 + r];
    // lo's upper half-wave <-> hi's lower half-wave
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(lo[r]), "+v"(hi[r]));
  }
  // lane (li, h): lo[0..3] -> columns 16h + 0..3, hi[0..3] -> 16h + 4..7, lo[4..7] -> 16h + 8..11, hi[4..7] -> 16h + 12..15
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    row16[s] = lo[s];
    row16[4 + s] = hi[s];
    row16[8 + s] = lo[4 + s];
    row16[12 + s] = hi[4 + s];
  }
}
// fragment-major store of a row-per-lane tile (see sgp_store_frag_tile for the layout); columns past n as zeros
__device__ __forceinline__ void sgp_store_frag_rows(float* __restrict__ Xf, float (&row16)[16], long e, int nT, int nS,
                                                    int tile, int strip, int col0, int n, int lane) {
  typedef float V4 __attribute__((ext_vector_type(4)));
  const int h = lane >> 5;
  float* blk = Xf + ((((long)e * nT + tile) * nS + strip) << 10) + 4 * lane;
  // (only the last strip can hold columns past n: the per-element masks -- 32 vector instructions that compete with the
  // partner wave's fp32 MFMAs for the SIMD -- stay out of every other strip's way)
  if (col0 + 32 > n) {
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (col0 + 16 * h + i >= n) row16[i] = 0.f;
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const V4 q = {row16[4 * v], row16[4 * v + 1], row16[4 * v + 2], row16[4 * v + 3]};
    *reinterpret_cast<V4*>(blk + 256 * v) = q;
  }
}

typedef float SgpV4 __attribute__((ext_vector_type(4)));
// ---------------------------------------------------------------------------------------------------------------
// The backward's operand for ONE latent function, one row of a 32 x 32 tile per lane, four columns at a time: with
// a4[s] = A[k][16 h + 4 v + s] of the lane's row k and u = u_k,
//     ab4[s] = Abar[k][16 h + 4 v + s] = a4[s] c_j + u f_j ,      usum += sum_s f_j a4[s]
// (c_j in cjs[32], f_j = fbar_j in fbs[32]: LDS, zero for the columns past n).  This is the Abar statement of
// sgp_kbar_strip_kernel at P == 1 with the contraction the compiler gives it there spelled out -- the product A c
// rounded, then fma(u, f, .), and fma(f, a, usum): written plainly here, where P is a constant, the compiler fuses the
// other pair and Abar differs in the last place (seen on the device).  The shared form was tried in the backward kernel
// too and taken out again: either way of writing it cost that kernel ~100 selects per tile (cfg 5: 0.9 % of the step).
__device__ __forceinline__ SgpV4 sgp_abar_group1(const float* a4, float u, const float* cjs, const float* fbs, int h, int v,
                                                 float& usum) {
  const SgpV4 cj4 = *reinterpret_cast<const SgpV4*>(&cjs[16 * h + 4 * v]);
  const SgpV4 fb4 = *reinterpret_cast<const SgpV4*>(&fbs[16 * h + 4 * v]);
  SgpV4 ab4;
#pragma unroll
  for (int s2 = 0; s2 < 4; ++s2) {
    const float aval = a4[s2];
    ab4[s2] = __builtin_fmaf(u, fb4[s2], aval * cj4[s2]);
    usum = __builtin_fmaf(fb4[s2], aval, usum);
  }
  return ab4;
}

#endif  // HB_SGP_STRIP_CUH
