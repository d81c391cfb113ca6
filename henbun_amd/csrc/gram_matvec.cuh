// What the matrix-free kernel product and the exact GP's predictive pass (csrc/gram_matvec.hip) share with the input
// gradients of that pass (csrc/gram_predict_grad.hip): the tiling constants, the argument blocks of the two phases, the
// K-loop of the product (gmv_tiles), the finish and the size of a group's partials.
#ifndef HB_GRAM_MATVEC_CUH
#define HB_GRAM_MATVEC_CUH

#include "common.cuh"
#include "mfma16.cuh"
#include "sgp_strip.cuh"
#include "acq_tail.cuh"

#define GMV_THREADS 256   // 4 waves, 32 columns each
#define GMV_CN 128        // columns per workgroup
#define GMV_KT 32         // rows per K-step
#define GMV_SMAX 64       // right-hand sides per workgroup (4 row tiles of 16)
#define GMV_CHUNK 2048    // rows per workgroup: fixed, whatever n, N and the device
#define GMV_GROUP 16      // chunks per launch: bounds the workspace (fixed, like GMV_CHUNK)
#define GMV_BLD 48        // row stride of a wave's K tile (sgp_pathwise.hip: PW_BLD)
#define GMV_CLD (GMV_KT + 2)  // row stride of the V tile (PW_CLD)

template <typename T>
struct GmvArgs {
  const T* x;     // [n, d]
  const T* x2;    // [N, d]
  const T* ell;   // [dl]
  long dl;
  const T* V;     // [S, N]
  double scale, shift;
  int shift_on;   // the symmetric form: shift * V[s, j] joins the finish
  T* out;         // [S, n]
  T* ws;          // [min(nchunk, GMV_GROUP), S, n] when nchunk > 1: the partials of the group in flight
  double* acc;    // [S, n] when nchunk > GMV_GROUP: the fold's running sum between groups
  int n, N, d, S, nstrip, nchunk;
  int c0, gchunks;   // the group in flight: chunks c0 .. c0 + gchunks - 1
  int to_ws;         // hb_gram_predict: a single chunk leaves its partial in the workspace too (out is not written)
};

// scale * sum + shift * v, written so that the epilogue and the fold round alike
template <typename T> __device__ __forceinline__ T gmv_finish(double scale, double shift, double sum, double v) {
  return (T)fma(shift, v, scale * sum);
}

// The K-loop of a workgroup (blockIdx.x: strip and chunk slot, as the kernels decode it) for right-hand sides s0 .. and,
// with DG > 0 derivative operand sets, dimensions k0 .. k0 + DG - 1:
//     acc[st][ct]      = V[s0 + 16 st .., chunk rows] . K(x2[chunk rows], x[col0 + 16 ct ..])
//     accd[k][st][ct]  = the same with the right operand K_ij (x2_ik - x_jk) / ell_k^2 of dimension k0 + k
// for the wave's 32 columns, col0 = GMV_CN strip + 32 w: register r of lane l is right-hand side s0 + 16 st + row(l, r),
// column col0 + 16 ct + l % 16.  D: the input dimension when it is at most 4 (the column's coordinates then live in
// registers), 0: any d, the coordinates re-read from memory at every use.  NST: row tiles of 16 right-hand sides.  The
// derivative operand is formed in registers from the value tile as the MFMA loop reads it, from a small LDS table of the
// step's x2 rows per dimension and the coordinates of the lane's two columns; DG == 0 (values alone) compiles none of it and
// ignores accd.  Every caller runs these lines, so their value bits are equal by construction
// (tests/test_variance_cache_grad_gpu.py::test_values_are_the_bits_of_gram_predict still checks it).
template <typename T, int D, int NST, int DG>
__device__ __forceinline__ void gmv_tiles(const GmvArgs<T>& a, int s0, int k0, typename PwMma<T>::Acc (&acc)[NST][2],
                                          typename PwMma<T>::Acc (&accd)[DG ? DG : 1][NST][2]) {
  typedef PwMma<T> MM;
  constexpr int SP = 16 * NST, DR = D ? D : 1, DGR = DG ? DG : 1;
  __shared__ __attribute__((aligned(16))) T Bs[GMV_THREADS / 64][GMV_KT][GMV_BLD];
  __shared__ __attribute__((aligned(16))) T Cs[SP][GMV_CLD];
  const int n = a.n, N = a.N, S = a.S, d = D ? D : a.d;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 31, h = lane >> 5;        // synthesis: column of the wave's tile, row parity
  const int l16 = lane & 15, g = lane >> 4;      // MFMA operands
  const int strip = blockIdx.x % a.nstrip, chunk = a.c0 + blockIdx.x / a.nstrip;
  const long col0 = (long)strip * GMV_CN + 32 * w;   // long: n may end within 128 of 2^31
  const int i0 = chunk * GMV_CHUNK, iend = N - i0 < GMV_CHUNK ? N : i0 + GMV_CHUNK;   // this workgroup's rows
  const long jc = (col0 + c < n ? col0 + c : (long)n - 1) * d;   // columns past n: a copy of the last one (never written out)
  const T* __restrict__ xj = a.x + jc;

  T xs[DR], sc[DR];
#pragma unroll
  for (int k = 0; k < DR; ++k) {
    if (D) {
      xs[k] = xj[k];
      sc[k] = T(SGP_EXP2_SCALE) / a.ell[a.dl == 1 ? 0 : k];
    }
  }
  auto rbf = [&](const T* __restrict__ zm) {     // k(x2_i, x): the difference first, scaled afterwards (sgp_strip.cuh)
    T r2 = T(0);
    if (D) {
#pragma unroll
      for (int k = 0; k < DR; ++k) {
        const T tt = (zm[k] - xs[k]) * sc[k];
        r2 += tt * tt;
      }
    } else {
      for (int k = 0; k < d; ++k) {
        const T tt = (zm[k] - xj[k]) * (T(SGP_EXP2_SCALE) / a.ell[a.dl == 1 ? 0 : k]);
        r2 += tt * tt;
      }
    }
    return hb_exp2_neg<T>(r2);
  };

  // derivatives: the two columns this lane holds in the MFMA's B operand, their coordinates and 1 / ell^2 for the factor;
  // Fs: x2_rk of the step's rows, per dimension of this workgroup; this thread's entry of it: dimension k0 + fk, row fr
  __shared__ T Fs[DGR][GMV_KT];
  T xm[2][DGR], ie2[DGR];
  const int fk = tid / GMV_KT, fr = tid % GMV_KT;
  const bool fok = fk < DG && k0 + fk < d;
  if constexpr (DG > 0) {
#pragma unroll
    for (int k = 0; k < DG; ++k) {
      const bool ok = k0 + k < d;
      const T e = a.ell[a.dl == 1 || !ok ? 0 : k0 + k];
      ie2[k] = ok ? T(1) / (e * e) : T(0);
#pragma unroll
      for (int cc = 0; cc < 2; ++cc) {
        const long j = col0 + 16 * cc + l16;
        xm[cc][k] = ok ? a.x[(j < n ? j : (long)n - 1) * d + k0 + k] : T(0);
      }
    }
  }

  // V tile of a K-step through registers: element e = tid + GMV_THREADS i is (right-hand side e / GMV_KT, row
  // e % GMV_KT); rows past the chunk's end and right-hand sides past S are zeros
  constexpr int CIT = SP * GMV_KT / GMV_THREADS;
  T creg[CIT];
  auto v_request = [&](int kb) {
#pragma unroll
    for (int i = 0; i < CIT; ++i) {
      const int e = tid + GMV_THREADS * i, s = s0 + e / GMV_KT, k = e % GMV_KT;
      const bool ok = s < S && k < iend - kb;
      creg[i] = ok ? a.V[(long)s * N + kb + k] : T(0);
    }
  };
  auto v_store = [&]() {
#pragma unroll
    for (int i = 0; i < CIT; ++i) {
      const int e = tid + GMV_THREADS * i;
      Cs[e / GMV_KT][e % GMV_KT] = creg[i];
    }
  };

#pragma unroll
  for (int st = 0; st < NST; ++st)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[st][ct][r] = T(0);
        if constexpr (DG > 0) {
#pragma unroll
          for (int k = 0; k < DG; ++k) accd[k][st][ct][r] = T(0);
        }
      }

  const int nK = (iend - i0 + GMV_KT - 1) / GMV_KT;
  v_request(i0);
#pragma nounroll
  for (int t = 0; t < nK; ++t) {
    const int kb = i0 + t * GMV_KT;
    __syncthreads();   // the MFMAs of the step before have read both tiles (and the table)
    v_store();
#pragma unroll
    for (int i = 0; i < GMV_KT / 2; ++i) {
      const int r = h + 2 * i;
      const bool in = r < iend - kb;
      const T v = rbf(a.x2 + (long)(in ? kb + r : iend - 1) * d);
      Bs[w][r][c] = in ? v : T(0);
    }
    if constexpr (DG > 0) {
      if (fk < DG)   // rows past the chunk's end: the K value is 0, any finite coordinate will do
        Fs[fk][fr] = fok ? a.x2[(long)(fr < iend - kb ? kb + fr : iend - 1) * d + k0 + fk] : T(0);
    }
    if (t + 1 < nK) v_request(kb + GMV_KT);   // the next step's V tile is in flight during the MFMAs
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GMV_KT / 4; ++kk) {
      const int r = 4 * kk + g;
      const T b0 = Bs[w][r][l16], b1 = Bs[w][r][16 + l16];
      T e0[DGR], e1[DGR];
      if constexpr (DG > 0) {
#pragma unroll
        for (int k = 0; k < DG; ++k) {
          const T f = Fs[k][r];
          e0[k] = b0 * ((f - xm[0][k]) * ie2[k]), e1[k] = b1 * ((f - xm[1][k]) * ie2[k]);
        }
      }
#pragma unroll
      for (int st = 0; st < NST; ++st) {
        const T av = Cs[16 * st + l16][r];
        acc[st][0] = MM::mma(av, b0, acc[st][0]);
        acc[st][1] = MM::mma(av, b1, acc[st][1]);
        if constexpr (DG > 0) {
#pragma unroll
          for (int k = 0; k < DG; ++k) {
            accd[k][st][0] = MM::mma(av, e0[k], accd[k][st][0]);
            accd[k][st][1] = MM::mma(av, e1[k], accd[k][st][1]);
          }
        }
      }
    }
  }
}

#define GPR_THREADS 256   // columns per workgroup of the fold

template <typename T>
struct GprArgs {
  GmvArgs<T> g;
  int P;
  double prior;
  AcqTail t;
  T* mean;        // [P, n], nullable
  T* var;         // [n], nullable
  T* val;         // [n], nullable
  double* pkey;   // arg-max partials [blocks]: the best value of the block's columns ...
  long* pcol;     // ... and its column (-1: none comparable); nullable together
};

// workspace, in elements of T: the partials of a group (rounded up to 8 bytes), the running double sum [S, n] beyond one
// group, the arg-max partials (a double and a long per GPR_THREADS columns)
static inline long gpr_part_elems(long n, long N, long S, int bytes) {
  const long nchunk = (N + GMV_CHUNK - 1) / GMV_CHUNK, g = nchunk < GMV_GROUP ? nchunk : GMV_GROUP;
  const long e = g * S * n;
  return bytes == 4 ? (e + 1) & ~1L : e;
}

#endif  // HB_GRAM_MATVEC_CUH
