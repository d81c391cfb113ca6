// Host-side helpers shared by the entries that stream an RBF sparse-GP model's A = W K(z, x) in column chunks
// (sgp_stats, sgp_predict, sgp_predict_grad / sgp_acq, sgp_predict_cov, sgp_kgrad, and sgp_bwd's products): ONE copy of
// the scratch rounding, of the column-chunk rule, of the by-type calls into hb_sgp_A_* / hb_matmul_*, and of what every
// entry requires of such a model's operands.  Host code only: nothing here is compiled for the device.
#ifndef HB_HOST_CALLS_CUH
#define HB_HOST_CALLS_CUH
#include "common.cuh"
#include "../../include/henbun_hip.h"

// scratch sections start on 64-element boundaries
static inline long hb_round64(long v) { return (v + 63) & ~63L; }

// Columns per chunk of a chunked entry: what `budget_elems` of scratch holds at `per_col_elems` per column, at most `cap`,
// a multiple of 32 and at least 32 -- and no more than n rounded up to 32 (32 for n <= 0, which no launch path reaches:
// the entries return, and their size queries answer 0, before they ask).
static inline long hb_chunk_cols(long budget_elems, long per_col_elems, long cap, long n) {
  long c = budget_elems / (per_col_elems > 0 ? per_col_elems : 1);
  c = c < cap ? c : cap;
  c &= ~31L;
  if (c < 32) c = 32;
  const long n32 = (n + 31) & ~31L;
  return c < n32 ? c : (n32 > 0 ? n32 : 32);
}

// A = W K(z, x) [E, M, n] in native precision
static inline int hb_sgp_A(int kind, const float* x, long sx, const float* z, const float* ell, long dl, const float* W,
                           const float* Wf, float* A, long E, long n, long M, long d, hipStream_t st) {
  return hb_sgp_A_f32(kind, x, sx, z, ell, dl, W, Wf, HB_PREC_NATIVE, A, E, n, M, d, st);
}
static inline int hb_sgp_A(int kind, const double* x, long sx, const double* z, const double* ell, long dl, const double* W,
                           const double* Wf, double* A, long E, long n, long M, long d, hipStream_t st) {
  return hb_sgp_A_f64(kind, x, sx, z, ell, dl, W, Wf, HB_PREC_NATIVE, A, E, n, M, d, st);
}

// C = alpha op(A) op(B): no bias, no activation, beta = 0
static inline int hb_matmul(const float* A, const float* B, float* C, long batch, long M, long N, long K, long lda, long ldb,
                            long ldc, long sA, long sB, long sC, int tA, int tB, double alpha, int flags, float* ws, long wse,
                            void* stream) {
  return hb_matmul_f32(A, B, C, batch, M, N, K, lda, ldb, ldc, sA, sB, sC, tA, tB, alpha, 0.0, nullptr, 0, HB_ACT_NONE, flags,
                       ws, wse, stream);
}
static inline int hb_matmul(const double* A, const double* B, double* C, long batch, long M, long N, long K, long lda, long ldb,
                            long ldc, long sA, long sB, long sC, int tA, int tB, double alpha, int flags, double* ws, long wse,
                            void* stream) {
  return hb_matmul_f64(A, B, C, batch, M, N, K, lda, ldb, ldc, sA, sB, sC, tA, tB, alpha, 0.0, nullptr, 0, HB_ACT_NONE, flags,
                       ws, wse, stream);
}
// the short form: C = op(A) B without a workspace of the caller's
template <typename T>
static inline int hb_matmul(const T* A, const T* B, T* C, long batch, long M, long N, long K, long lda, long ldb, long ldc,
                            long sA, long sB, long sC, int tA, hipStream_t st) {
  return hb_matmul(A, B, C, batch, M, N, K, lda, ldb, ldc, sA, sB, sC, tA, 0, 1.0, 0, (T*)nullptr, 0L, st);
}

// What every entry requires of an RBF model's operands: the UnitRBF kernel (`only`: what the entry says only that kernel
// has or is), 1 or d lengthscales, a Wfrag (if any) the strip kernels can read, M^2 within an int.
#define HB_REQUIRE_RBF_MODEL(who, only, kind, dl, d, Wf, M)                                                                  \
  do {                                                                                                                       \
    HB_REQUIRE((kind) == HB_KERN_RBF, "%s: only the UnitRBF kernel %s (kind=%d)", who, only, kind);                          \
    HB_REQUIRE((dl) == 1 || (dl) == (d), "%s: lengthscales must have 1 or d entries", who);                                  \
    HB_REQUIRE(!(Wf) || ((uintptr_t)(Wf) % 16 == 0 && (M) % 32 == 0), "%s: Wfrag needs 16-byte alignment and M %% 32 == 0", \
               who);                                                                                                         \
    HB_REQUIRE((long)(M) * (M) < 2147483647L, "%s: matrix too large", who);                                                  \
  } while (0)

#endif  // HB_HOST_CALLS_CUH
