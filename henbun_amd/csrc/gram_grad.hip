// Bilinear contraction of the kernel matrix and of its lengthscale derivative against pairs of vectors
// (hb_gram_bilinear_grad_*), include/henbun_hip.h; not in the reference; Gardner et al. 2018.  With K = K(x, x) [N, N],
// A, B [S, N] and weights w [S]:
//
//     g[0]     = sum_s w_s sum_ij A_si B_sj K_ij
//     g[1 + k] = sum_s w_s sum_ij A_si B_sj K_ij (x_ik - x_jk)^2 / ell_k^3        (dl = 1: summed over k, ell_0^3)
//
// -- the traces the gradient of the exact GP's log marginal likelihood is made of (henbun_amd/gp/exact.py).  Neither K nor
// W = sum_s w_s A_s (x) B_s is written to memory.  The decomposition is that of gram_matvec_kernel, with its constants:
// a workgroup per strip of GMV_CN columns j (a wave per 32) and chunk of GMV_CHUNK rows i walks the rows in K-steps of
// GMV_KT.  Per K-step a wave forms the 32 x 32 tile of W on the 16 x 16 x 4 MFMA with the PAIR index as the contraction
// dimension -- the A tile staged through LDS, the wave's w_s B_sj fragments (w applied in double, rounded once) loaded once
// per chunk into registers -- and every lane then evaluates K_ij and the scaled squared differences at the 16 accumulator
// positions it owns (8 rows x 2 columns; the columns' coordinates in registers for d <= 4, the rows' in a small LDS tile)
// in the difference-then-scale exp2 form of sgp_strip.cuh, and adds W_ij K_ij [t_k^2] into 1 + dl per-lane sums kept in
// DOUBLE (the products of two storage-type values are exact there).  The factor 1 / (SGP_EXP2_SCALE^2 ell_k) that turns
// t_k^2 = (x_ik - x_jk)^2 SGP_EXP2_SCALE^2 / ell_k^2 into the derivative is applied once, in double, at the very end.
//
// No atomics: a workgroup leaves one partial [1 + dl]; a second launch of one workgroup adds the partials in a fixed
// order in double.  More than GMV_GROUP chunks are taken GMV_GROUP at a time and more than GMV_SMAX pairs GMV_SMAX at a
// time, the fold carrying its running sum in g from one launch to the next, so the workspace is
// min(chunks, GMV_GROUP) x strips x (1 + dl) doubles whatever S.  ARD lengthscales with d > 4 are handled four dimensions
// per blockIdx.z, K recomputed per group (the memory path: coordinates re-read, the scales divided once into LDS); dl = 1
// needs one accumulator whatever d.  Two calls return the same bits.
//
// Not done: K is symmetric and only its lower triangle with A_i B_j + A_j B_i would do; every value is synthesised twice
// here, as in gram_matvec.hip.
#include "common.cuh"
#include "mfma16.cuh"
#include "sgp_strip.cuh"
#include "../../include/henbun_hip.h"

#define GMV_THREADS 256   // the constants of gram_matvec.hip
#define GMV_CN 128
#define GMV_KT 32
#define GMV_SMAX 64
#define GMV_CHUNK 2048
#define GMV_GROUP 16
#define GMV_CLD (GMV_KT + 2)
#define GBG_DG 4          // lengthscale accumulators per workgroup
#define GBG_SCMAX 64      // memory path: the scales of the first GBG_SCMAX dimensions are divided once, into LDS

template <typename T>
struct GbgArgs {
  const T* x;        // [N, d]
  const T* ell;      // [dl]
  long dl;
  const T* A;        // [S, N]
  const T* B;        // [S, N]
  const double* w;   // [S]
  double* part;      // [gchunks * nstrip, 1 + dl]
  double* g;         // [1 + dl]: the running sum between launches, the result after the last
  int N, d, S, nstrip;
  int s0, sb;        // the pairs in flight: s0 .. s0 + sb - 1
  int c0, gchunks;   // the chunks in flight
  int first, last;
};

// D: the input dimension when it is at most 4, 0: any d (coordinates re-read from memory).  NST: tiles of 16 pairs.
// ARD: one sum per dimension (those of group blockIdx.z when D == 0) instead of one for all.
template <typename T, int D, int NST, bool ARD>
__global__ void __launch_bounds__(GMV_THREADS) gram_bilinear_grad_kernel(GbgArgs<T> a) {
  typedef PwMma<T> MM;
  constexpr int SP = 16 * NST, DR = D ? D : 1, NG = ARD ? (D ? D : GBG_DG) : 1;
  __shared__ __attribute__((aligned(16))) T As[SP][GMV_CLD];
  __shared__ T Xs[GMV_KT][DR];
  __shared__ double red[GMV_THREADS / 64][1 + NG];
  __shared__ T Scs[D ? 1 : GBG_SCMAX];
  const int N = a.N, d = D ? D : a.d, S1 = a.s0 + a.sb;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l16 = lane & 15, g = lane >> 4;
  const int strip = blockIdx.x % a.nstrip, slot = blockIdx.x / a.nstrip, chunk = a.c0 + slot;
  const int k0 = (ARD && !D) ? GBG_DG * (int)blockIdx.z : 0;             // first dimension of this workgroup's sums
  const int kn = (ARD && !D) ? (d - k0 < GBG_DG ? d - k0 : GBG_DG) : 0;  // and how many of them
  const long col0 = (long)strip * GMV_CN + 32 * w;
  const int i0 = chunk * GMV_CHUNK, iend = N - i0 < GMV_CHUNK ? N : i0 + GMV_CHUNK;

  // the wave's two columns per lane: coordinates (a column past N: a copy of the last one, its B is zero)
  long jc[2];
  T xs[2][DR], sc[DR];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const long j = col0 + 16 * ct + l16;
    jc[ct] = (j < N ? j : (long)N - 1) * d;
    if (D) {
#pragma unroll
      for (int k = 0; k < DR; ++k) xs[ct][k] = a.x[jc[ct] + k];
    }
  }
  if (D) {
#pragma unroll
    for (int k = 0; k < DR; ++k) sc[k] = T(SGP_EXP2_SCALE) / a.ell[a.dl == 1 ? 0 : k];
  } else {   // (read after the K-loop's first barrier)
    for (int k = tid; k < d && k < GBG_SCMAX; k += GMV_THREADS) Scs[k] = T(SGP_EXP2_SCALE) / a.ell[a.dl == 1 ? 0 : k];
  }

  // w_s B_sj for the wave's columns, as the MFMA's B operand: k-step kk, lane (g, l16) -> pair 4 kk + g, column 16 ct + l16
  T bf[4 * NST][2];
#pragma unroll
  for (int kk = 0; kk < 4 * NST; ++kk)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const int s = a.s0 + 4 * kk + g;
      const long j = col0 + 16 * ct + l16;
      bf[kk][ct] = (s < S1 && j < N) ? (T)(a.w[s] * (double)a.B[(long)s * N + j]) : T(0);
    }

  // A tile of a K-step through registers (gram_matvec_kernel's V tile): rows past the chunk's end and pairs past the
  // block are zeros, so W is zero there; the rows' coordinates ride along (a row past the end: a copy of the last one)
  constexpr int CIT = SP * GMV_KT / GMV_THREADS;
  T creg[CIT], xreg = T(0);
  auto v_request = [&](int kb) {
#pragma unroll
    for (int i = 0; i < CIT; ++i) {
      const int e = tid + GMV_THREADS * i, s = a.s0 + e / GMV_KT, k = e % GMV_KT;
      const bool ok = s < S1 && k < iend - kb;
      creg[i] = ok ? a.A[(long)s * N + kb + k] : T(0);
    }
    if (D && tid < GMV_KT * DR) {
      const int r = tid / DR, k = tid % DR;
      xreg = a.x[(long)(r < iend - kb ? kb + r : iend - 1) * d + k];
    }
  };
  auto v_store = [&]() {
#pragma unroll
    for (int i = 0; i < CIT; ++i) {
      const int e = tid + GMV_THREADS * i;
      As[e / GMV_KT][e % GMV_KT] = creg[i];
    }
    if (D && tid < GMV_KT * DR) Xs[tid / DR][tid % DR] = xreg;
  };

  double sum0 = 0.0, sumk[NG];
#pragma unroll
  for (int q = 0; q < NG; ++q) sumk[q] = 0.0;

  const int nK = (iend - i0 + GMV_KT - 1) / GMV_KT;
  v_request(i0);
#pragma nounroll
  for (int t = 0; t < nK; ++t) {
    const int kb = i0 + t * GMV_KT;
    __syncthreads();   // the step before has read both tiles
    v_store();
    if (t + 1 < nK) v_request(kb + GMV_KT);
    __syncthreads();
    typename MM::Acc acc[2][2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[rt][ct][r] = T(0);
#pragma unroll
    for (int kk = 0; kk < 4 * NST; ++kk) {
      const T a0 = As[4 * kk + g][l16], a1 = As[4 * kk + g][16 + l16];
      acc[0][0] = MM::mma(a0, bf[kk][0], acc[0][0]);
      acc[0][1] = MM::mma(a0, bf[kk][1], acc[0][1]);
      acc[1][0] = MM::mma(a1, bf[kk][0], acc[1][0]);
      acc[1][1] = MM::mma(a1, bf[kk][1], acc[1][1]);
    }
    // register r of tile (rt, ct) is W at row kb + 16 rt + row(lane, r), column col0 + 16 ct + l16
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * rt + MM::row(lane, r);
        const T* __restrict__ xi = a.x + (long)(row < iend - kb ? kb + row : iend - 1) * d;   // the memory path's row
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const double wv = (double)acc[rt][ct][r];
          if (D) {
            T r2 = T(0), t2[DR];
#pragma unroll
            for (int k = 0; k < DR; ++k) {
              const T tt = (Xs[row][k] - xs[ct][k]) * sc[k];
              t2[k] = tt * tt;
              r2 += t2[k];
            }
            const double wk = wv * (double)hb_exp2_neg<T>(r2);
            sum0 += wk;
            if (ARD) {
#pragma unroll
              for (int k = 0; k < DR; ++k) sumk[k < NG ? k : 0] = fma(wk, (double)t2[k], sumk[k < NG ? k : 0]);
            } else {
              sumk[0] = fma(wk, (double)r2, sumk[0]);
            }
          } else {
            const T* __restrict__ xj = a.x + jc[ct];
            T r2 = T(0), t2[NG];
#pragma unroll
            for (int q = 0; q < NG; ++q) t2[q] = T(0);
            for (int k = 0; k < d; ++k) {
              const T tt = (xi[k] - xj[k]) * (k < GBG_SCMAX ? Scs[k] : T(SGP_EXP2_SCALE) / a.ell[a.dl == 1 ? 0 : k]);
              const T v = tt * tt;
              r2 += v;
              if (ARD) {
#pragma unroll
                for (int q = 0; q < NG; ++q)
                  if (k == k0 + q) t2[q] = v;
              }
            }
            const double wk = wv * (double)hb_exp2_neg<T>(r2);
            sum0 += wk;
            if (ARD) {
#pragma unroll
              for (int q = 0; q < NG; ++q) sumk[q] = fma(wk, (double)t2[q], sumk[q]);
            } else {
              sumk[0] = fma(wk, (double)r2, sumk[0]);
            }
          }
        }
      }
  }

  // lanes -> wave (a fixed tree) -> the workgroup's four waves in order -> one partial per workgroup
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum0 += __shfl_down(sum0, o, 64);
#pragma unroll
    for (int q = 0; q < NG; ++q) sumk[q] += __shfl_down(sumk[q], o, 64);
  }
  if (lane == 0) {
    red[w][0] = sum0;
#pragma unroll
    for (int q = 0; q < NG; ++q) red[w][1 + q] = sumk[q];
  }
  __syncthreads();
  if (tid == 0) {
    double* __restrict__ out = a.part + (long)blockIdx.x * (1 + a.dl);
    if (k0 == 0) out[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    const int cnt = ARD ? (D ? D : kn) : 1;
    for (int q = 0; q < cnt; ++q) out[1 + k0 + q] = ((red[0][1 + q] + red[1][1 + q]) + red[2][1 + q]) + red[3][1 + q];
  }
}

// g[c] (+)= the partials of the launch before, added in a fixed order in double: a thread's stride, then a tree over the
// workgroup; the last fold applies 1 / (SGP_EXP2_SCALE^2 ell) to the lengthscale components.  One workgroup.
template <typename T>
__global__ void __launch_bounds__(256) gram_bilinear_grad_fold_kernel(GbgArgs<T> a) {
  __shared__ double red[256];
  const int tid = threadIdx.x, nc = 1 + (int)a.dl;
  const long np = (long)a.gchunks * a.nstrip;
  for (int c = 0; c < nc; ++c) {
    double acc = 0.0;
    for (long e = tid; e < np; e += 256) acc += a.part[e * nc + c];
    __syncthreads();   // red may still be read from the component before
    red[tid] = acc;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) {
      double v = (a.first ? 0.0 : a.g[c]) + red[0];
      if (a.last && c > 0) v /= (SGP_EXP2_SCALE * SGP_EXP2_SCALE) * (double)a.ell[a.dl == 1 ? 0 : c - 1];
      a.g[c] = v;
    }
  }
}

template <typename T, int D, bool ARD>
static void gram_bilinear_grad_launch(const GbgArgs<T>& a, int nst, dim3 grid, hipStream_t st) {
  if (nst == 1)
    hipLaunchKernelGGL((gram_bilinear_grad_kernel<T, D, 1, ARD>), grid, dim3(GMV_THREADS), 0, st, a);
  else if (nst == 2)
    hipLaunchKernelGGL((gram_bilinear_grad_kernel<T, D, 2, ARD>), grid, dim3(GMV_THREADS), 0, st, a);
  else if (nst == 3)
    hipLaunchKernelGGL((gram_bilinear_grad_kernel<T, D, 3, ARD>), grid, dim3(GMV_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL((gram_bilinear_grad_kernel<T, D, 4, ARD>), grid, dim3(GMV_THREADS), 0, st, a);
}
template <typename T, int D>
static void gram_bilinear_grad_launch_d(const GbgArgs<T>& a, int nst, dim3 grid, hipStream_t st) {
  if (a.dl == 1)
    gram_bilinear_grad_launch<T, D, false>(a, nst, grid, st);
  else
    gram_bilinear_grad_launch<T, D, true>(a, nst, grid, st);
}

extern "C" long hb_gram_bilinear_grad_ws_elems(long N, long dl) {
  if (N <= 0 || dl < 1) return 0;
  const long nstrip = (N + GMV_CN - 1) / GMV_CN, nchunk = (N + GMV_CHUNK - 1) / GMV_CHUNK;
  return (nchunk < GMV_GROUP ? nchunk : GMV_GROUP) * nstrip * (1 + dl);
}

template <typename T>
static int gram_bilinear_grad(int kind, const T* x, const T* ell, long dl, const T* A, const T* B, const double* w, double* g,
                              long N, long d, long S, double* ws, hipStream_t st) {
  HB_REQUIRE(kind == HB_KERN_RBF, "hb_gram_bilinear_grad: the UnitRBF kernel only (kind=%d)", kind);
  HB_REQUIRE(N >= 0 && d >= 1 && S >= 1, "hb_gram_bilinear_grad: bad extents (N=%ld d=%ld S=%ld)", N, d, S);
  HB_REQUIRE(dl == 1 || dl == d, "hb_gram_bilinear_grad: lengthscales must have 1 or d entries");
  HB_REQUIRE(ell && g && w && (N == 0 || (x && A && B)), "hb_gram_bilinear_grad: NULL pointer");
  const long nstrip = (N + GMV_CN - 1) / GMV_CN, nchunk = (N + GMV_CHUNK - 1) / GMV_CHUNK;
  HB_REQUIRE(N <= 2147483647L && d <= 2147483647L && S <= 2147483647L && nstrip * GMV_GROUP <= 2147483647L &&
                 hb_cdiv(d, GBG_DG) <= 65535,
             "hb_gram_bilinear_grad: too large (N, S below 2^31, d at most 4 x 65535)");
  HB_REQUIRE(ws || N == 0, "hb_gram_bilinear_grad: NULL workspace (hb_gram_bilinear_grad_ws_elems)");
  if (N == 0) {
    HB_HIP(hb_zero_async(g, (size_t)(1 + dl) * sizeof(double), st));
    return 0;
  }
  GbgArgs<T> a;
  a.x = x; a.ell = ell; a.dl = dl; a.A = A; a.B = B; a.w = w; a.part = ws; a.g = g;
  a.N = (int)N; a.d = (int)d; a.S = (int)S; a.nstrip = (int)nstrip;
  const unsigned nz = (dl > 1 && d > 4) ? (unsigned)hb_cdiv(d, GBG_DG) : 1u;
  for (long s0 = 0; s0 < S; s0 += GMV_SMAX) {
    a.s0 = (int)s0;
    a.sb = (int)(S - s0 < GMV_SMAX ? S - s0 : GMV_SMAX);
    const int nst = hb_cdiv(a.sb, 16);
    for (long c0 = 0; c0 < nchunk; c0 += GMV_GROUP) {
      a.c0 = (int)c0;
      a.gchunks = (int)(nchunk - c0 < GMV_GROUP ? nchunk - c0 : GMV_GROUP);
      a.first = s0 == 0 && c0 == 0;
      a.last = s0 + GMV_SMAX >= S && c0 + GMV_GROUP >= nchunk;
      const dim3 grid((unsigned)(nstrip * a.gchunks), 1, nz);
      if (d == 1)
        gram_bilinear_grad_launch_d<T, 1>(a, nst, grid, st);
      else if (d == 2)
        gram_bilinear_grad_launch_d<T, 2>(a, nst, grid, st);
      else if (d == 3)
        gram_bilinear_grad_launch_d<T, 3>(a, nst, grid, st);
      else if (d == 4)
        gram_bilinear_grad_launch_d<T, 4>(a, nst, grid, st);
      else
        gram_bilinear_grad_launch_d<T, 0>(a, nst, grid, st);
      HB_LAUNCH_CHECK();
      hipLaunchKernelGGL((gram_bilinear_grad_fold_kernel<T>), dim3(1), dim3(256), 0, st, a);
      HB_LAUNCH_CHECK();
    }
  }
  return 0;
}

extern "C" int hb_gram_bilinear_grad_f32(int kind, const float* x, const float* ell, long dl, const float* A, const float* B,
                                         const double* w, double* g, long N, long d, long S, double* ws, void* stream) {
  return gram_bilinear_grad<float>(kind, x, ell, dl, A, B, w, g, N, d, S, ws, (hipStream_t)stream);
}
extern "C" int hb_gram_bilinear_grad_f64(int kind, const double* x, const double* ell, long dl, const double* A, const double* B,
                                         const double* w, double* g, long N, long d, long S, double* ws, void* stream) {
  return gram_bilinear_grad<double>(kind, x, ell, dl, A, B, w, g, N, d, S, ws, (hipStream_t)stream);
}
