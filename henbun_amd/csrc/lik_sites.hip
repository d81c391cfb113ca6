// Per-point sites of a factorising likelihood under Gaussian marginals, and the predictive of y
// (hb_lik_sites_*, hb_lik_predict_*, include/henbun_hip.h; SparseGP.natgrad_q, models.SVGPLik).
//
// For f_j ~ N(mu_j, v_j), mu_j = mscale mean_j, v_j = vscale var_j:
//     l_j = E[log p(y_j | f)],   g_j = E[d log p / df],   lam_j = E[-d2 log p / df2],   beta_j = g_j + lam_j mu_j.
// lam and beta are the weights of the conjugate update of q(u) (conjugate-computation VI, Khan & Lin 2017): they go
// into hb_sgp_wstats_* as w and r.  Arithmetic is double whatever the storage type T of y, mean, var, lam, beta; one
// rounding on output, saturated to the largest finite T (the Poisson moments at mu + v / 2 near 88 pass float's range).
//   HB_LIK_GAUSSIAN   closed form
//   HB_LIK_BERNOULLI  logit link, log p = y f - softplus(f): 20-node Gauss-Hermite, f_i = mu + sqrt(2 v) x_i.  sigmoid(f),
//                     sigmoid(-f) and their product come from e = exp(-|f|) (no 1 - sigmoid: the tails keep their digits)
//   HB_LIK_POISSON    exp link, closed form with e = exp(mu + v / 2)
// sum_j l_j: every block folds its threads' terms (a grid-stride loop, a fixed grid for a given N) into one partial, a
// second launch of one block adds the partials in block order.  No atomics: two runs give the same bits.
#include "common.cuh"
#include "../../include/henbun_hip.h"

#define LK_THREADS 256
#define LK_MAX_BLOCKS 1024
#define LK_GH 20

// Gauss-Hermite nodes x_i and weights w_i / sqrt(pi) of the 20-point rule (numpy.polynomial.hermite.hermgauss(20))
__device__ static const double LK_X[LK_GH] = {
    -5.38748089001123276e+00, -4.60368244955074424e+00, -3.94476404011562520e+00, -3.34785456738321630e+00,
    -2.78880605842813045e+00, -2.25497400208927568e+00, -1.73853771211658614e+00, -1.23407621539532308e+00,
    -7.37473728545394391e-01, -2.45340708300901239e-01, 2.45340708300901239e-01,  7.37473728545394391e-01,
    1.23407621539532308e+00,  1.73853771211658614e+00,  2.25497400208927568e+00,  2.78880605842813045e+00,
    3.34785456738321630e+00,  3.94476404011562520e+00,  4.60368244955074424e+00,  5.38748089001123276e+00};
__device__ static const double LK_W[LK_GH] = {
    1.25780067243792340e-13, 2.48206236231517553e-10, 6.12749025998292797e-08, 4.40212109023085101e-06,
    1.28826279961929280e-04, 1.83010313108049002e-03, 1.39978374471010220e-02, 6.15063720639768968e-02,
    1.61739333983999978e-01, 2.60793063449554885e-01, 2.60793063449554885e-01, 1.61739333983999978e-01,
    6.15063720639768968e-02, 1.39978374471010220e-02, 1.83010313108049002e-03, 1.28826279961929280e-04,
    4.40212109023085101e-06, 6.12749025998292797e-08, 2.48206236231517553e-10, 1.25780067243792340e-13};

template <typename T>
__device__ __forceinline__ T lk_out(double x);
template <>
__device__ __forceinline__ double lk_out<double>(double x) { return x; }
template <>
__device__ __forceinline__ float lk_out<float>(double x) {
  const double big = 3.4028234663852886e+38;
  return (float)(x > big ? big : (x < -big ? -big : x));
}

// (sigmoid(f), sigmoid(-f)) from e = exp(-|f|)
__device__ __forceinline__ void lk_sigmoids(double f, double* sp, double* sn, double* e_out) {
  const double e = exp(-fabs(f)), big = 1.0 / (1.0 + e), small = e * big;
  *sp = f >= 0.0 ? big : small;
  *sn = f >= 0.0 ? small : big;
  *e_out = e;
}

__device__ __forceinline__ void lk_site(int lik, double y, double mu, double v, double s2, double* l, double* lam, double* beta) {
  if (lik == HB_LIK_GAUSSIAN) {
    const double dy = y - mu;
    *l = -0.5 * log(6.283185307179586477 * s2) - (dy * dy + v) / (2.0 * s2);
    *lam = 1.0 / s2;
    *beta = y / s2;
  } else if (lik == HB_LIK_BERNOULLI) {
    const double sd = sqrt(2.0 * v);
    double sl = 0.0, sg = 0.0, sh = 0.0;
#pragma unroll 4
    for (int i = 0; i < LK_GH; ++i) {
      const double f = mu + sd * LK_X[i];
      double sp, sn, e;
      lk_sigmoids(f, &sp, &sn, &e);
      const double softplus = (f > 0.0 ? f : 0.0) + log1p(e);
      sl += LK_W[i] * (y * f - softplus);
      sg += LK_W[i] * (y * sn - (1.0 - y) * sp);   // y - sigmoid(f)
      sh += LK_W[i] * (sp * sn);
    }
    *l = sl;
    *lam = sh;
    *beta = sg + sh * mu;
  } else {
    const double e = exp(mu + 0.5 * v);
    *l = y * mu - e - lgamma(y + 1.0);
    *lam = e;
    *beta = (y - e) + e * mu;
  }
}

template <typename T>
__global__ void __launch_bounds__(LK_THREADS) lik_sites_kernel(int lik, const T* __restrict__ y, const T* __restrict__ mean,
                                                               const T* __restrict__ var, double mscale, double vscale,
                                                               double s2, T* __restrict__ lam, T* __restrict__ beta,
                                                               double* __restrict__ partial, long N) {
  __shared__ double red[16];
  const long stride = (long)gridDim.x * LK_THREADS;
  double s = 0.0;
  for (long j = (long)blockIdx.x * LK_THREADS + threadIdx.x; j < N; j += stride) {
    double l, la, be;
    lk_site(lik, (double)y[j], mscale * (double)mean[j], vscale * (double)var[j], s2, &l, &la, &be);
    lam[j] = lk_out<T>(la);
    beta[j] = lk_out<T>(be);
    s += l;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// one block: the partials in block order (thread t takes t, t + 256, ..), then the block's fixed tree
__global__ void __launch_bounds__(LK_THREADS) lik_sites_fold_kernel(const double* __restrict__ partial, long nb,
                                                                    double* __restrict__ out) {
  __shared__ double red[16];
  double s = 0.0;
  for (long k = threadIdx.x; k < nb; k += LK_THREADS) s += partial[k];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s;
}

template <typename T>
__global__ void __launch_bounds__(LK_THREADS) lik_predict_kernel(int lik, const T* __restrict__ mean, const T* __restrict__ var,
                                                                 double s2, T* __restrict__ ymean, T* __restrict__ yvar, long N) {
  const long stride = (long)gridDim.x * LK_THREADS;
  for (long j = (long)blockIdx.x * LK_THREADS + threadIdx.x; j < N; j += stride) {
    const double mu = (double)mean[j], v = (double)var[j];
    double om, ov;
    if (lik == HB_LIK_GAUSSIAN) {
      om = mu;
      ov = v + s2;
    } else if (lik == HB_LIK_BERNOULLI) {
      const double sd = sqrt(2.0 * v);
      double p = 0.0, q = 0.0;   // q = E sigmoid(-f) = 1 - p, summed on its own: p (1 - p) keeps its digits as p -> 1
#pragma unroll 4
      for (int i = 0; i < LK_GH; ++i) {
        double sp, sn, e;
        lk_sigmoids(mu + sd * LK_X[i], &sp, &sn, &e);
        p += LK_W[i] * sp;
        q += LK_W[i] * sn;
      }
      om = p;
      ov = p * q;
    } else {
      const double e = exp(mu + 0.5 * v);
      om = e;
      ov = e + expm1(v) * e * e;
    }
    ymean[j] = lk_out<T>(om);
    yvar[j] = lk_out<T>(ov);
  }
}

static inline long lk_blocks(long N) {
  const long nb = (N + LK_THREADS - 1) / LK_THREADS;
  return nb < 1 ? 1 : (nb > LK_MAX_BLOCKS ? LK_MAX_BLOCKS : nb);
}

static int lk_check(const char* who, int lik, long N, double param) {
  HB_REQUIRE(lik == HB_LIK_GAUSSIAN || lik == HB_LIK_BERNOULLI || lik == HB_LIK_POISSON, "%s: unknown likelihood id %d", who,
             lik);
  HB_REQUIRE(N >= 0, "%s: negative N (%ld)", who, N);
  HB_REQUIRE(lik != HB_LIK_GAUSSIAN || param > 0.0, "%s: the Gaussian likelihood needs a variance > 0 (got %g)", who, param);
  return 0;
}

extern "C" long hb_lik_sites_ws_elems(long N) { return N > 0 ? lk_blocks(N) : 1; }

template <typename T>
static int lik_sites(int lik, const T* y, const T* mean, const T* var, double mscale, double vscale, double param, T* lam,
                     T* beta, double* ell_sum, long N, double* ws, hipStream_t st) {
  if (lk_check("hb_lik_sites", lik, N, param)) return -1;
  HB_REQUIRE(ell_sum && ws, "hb_lik_sites: NULL output / workspace pointer");
  HB_REQUIRE(N == 0 || (y && mean && var && lam && beta), "hb_lik_sites: NULL pointer");
  HB_REQUIRE(vscale >= 0.0, "hb_lik_sites: vscale must not be negative (got %g)", vscale);
  const long nb = N > 0 ? lk_blocks(N) : 0;
  if (nb > 0) {
    hipLaunchKernelGGL((lik_sites_kernel<T>), dim3((unsigned)nb), dim3(LK_THREADS), 0, st, lik, y, mean, var, mscale, vscale,
                       param, lam, beta, ws, N);
    HB_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(lik_sites_fold_kernel, dim3(1), dim3(LK_THREADS), 0, st, ws, nb, ell_sum);
  HB_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int lik_predict(int lik, const T* mean, const T* var, double param, T* ymean, T* yvar, long N, hipStream_t st) {
  if (lk_check("hb_lik_predict", lik, N, param)) return -1;
  if (N == 0) return 0;
  HB_REQUIRE(mean && var && ymean && yvar, "hb_lik_predict: NULL pointer");
  hipLaunchKernelGGL((lik_predict_kernel<T>), dim3((unsigned)lk_blocks(N)), dim3(LK_THREADS), 0, st, lik, mean, var, param,
                     ymean, yvar, N);
  HB_LAUNCH_CHECK();
  return 0;
}

extern "C" int hb_lik_sites_f32(int lik, const float* y, const float* mean, const float* var, double mscale, double vscale,
                                double param, float* lam, float* beta, double* ell_sum, long N, double* ws, void* stream) {
  return lik_sites<float>(lik, y, mean, var, mscale, vscale, param, lam, beta, ell_sum, N, ws, (hipStream_t)stream);
}
extern "C" int hb_lik_sites_f64(int lik, const double* y, const double* mean, const double* var, double mscale, double vscale,
                                double param, double* lam, double* beta, double* ell_sum, long N, double* ws, void* stream) {
  return lik_sites<double>(lik, y, mean, var, mscale, vscale, param, lam, beta, ell_sum, N, ws, (hipStream_t)stream);
}
extern "C" int hb_lik_predict_f32(int lik, const float* mean, const float* var, double param, float* ymean, float* yvar, long N,
                                  void* stream) {
  return lik_predict<float>(lik, mean, var, param, ymean, yvar, N, (hipStream_t)stream);
}
extern "C" int hb_lik_predict_f64(int lik, const double* mean, const double* var, double param, double* ymean, double* yvar,
                                  long N, void* stream) {
  return lik_predict<double>(lik, mean, var, param, ymean, yvar, N, (hipStream_t)stream);
}
