// Declarations shared by the matrix-free kernel product and the exact GP's predictive pass (csrc/gram_matvec.hip) and by
// the input gradients of that pass (csrc/gram_predict_grad.hip): the tiling constants, the argument blocks of the two
// phases, the finish and the size of a group's partials.  The kernels themselves live in the two sources.
#ifndef HB_GRAM_MATVEC_CUH
#define HB_GRAM_MATVEC_CUH

#include "common.cuh"
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
