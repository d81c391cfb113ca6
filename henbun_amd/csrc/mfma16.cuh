// The 16 x 16 x 4 MFMA of either dtype, as the kernels that put draws / right-hand sides on the rows use it
// (csrc/sgp_pathwise.hip, csrc/gram_matvec.hip).
#ifndef HB_MFMA16_CUH
#define HB_MFMA16_CUH

// lane l supplies A[row l % 16][k l / 16] and B[k l / 16][col l % 16]; accumulator register r of lane l holds
// C[row(l, r)][col l % 16] (the two dtypes differ in the row map only).
template <typename T> struct PwMma;
template <> struct PwMma<float> {
  typedef float Acc __attribute__((ext_vector_type(4)));
  __device__ static __forceinline__ Acc mma(float a, float b, Acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
  __device__ static __forceinline__ int row(int lane, int r) { return 4 * (lane >> 4) + r; }
};
template <> struct PwMma<double> {
  typedef double Acc __attribute__((ext_vector_type(4)));
  __device__ static __forceinline__ Acc mma(double a, double b, Acc c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
  __device__ static __forceinline__ int row(int lane, int r) { return (lane >> 4) + 4 * r; }
};

#endif  // HB_MFMA16_CUH
