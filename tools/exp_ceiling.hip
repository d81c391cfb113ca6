// A bare double-precision exp loop: the ceiling tools/bench_sgp_psi.py holds the psi-statistics kernel against, measured
// independently of the library.  Every thread keeps 16 independent sums and adds exp(e) to each, e = fma(i, step, base):
// one fma, one exp and one add per evaluation -- the least a (point, pair) evaluation of psi2 can cost.
//   hipcc -O3 -fPIC -shared --offload-arch=gfx950 tools/exp_ceiling.hip -o tools/_bin/libexp_ceiling.so
#include <hip/hip_runtime.h>

__global__ void __launch_bounds__(256) exp_ceiling_kernel(const double* __restrict__ base, double step, long iters,
                                                          double* __restrict__ out) {
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  double b[16], acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    b[k] = base[(t + k) & 1023];
    acc[k] = 0.0;
  }
  for (long i = 0; i < iters; ++i) {
    const double x = (double)i;
#pragma unroll
    for (int k = 0; k < 16; ++k) acc[k] += exp(__builtin_fma(x, step, b[k]));
  }
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) s += acc[k];
  out[t] = s;
}

// base: 1024 doubles, out: blocks * 256 doubles; evaluations = blocks * 256 * 16 * iters
extern "C" int exp_ceiling_launch(const double* base, double step, long iters, double* out, long blocks, void* stream) {
  hipLaunchKernelGGL(exp_ceiling_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, base, step, iters, out);
  return (int)hipGetLastError();
}
