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
// The likelihoods with a parameter of their own (HB_LIK_LAPLACE, _GAMMA, _NEGBINOMIAL, _BINOMIAL; formulas in the header)
// have kernels of their own below, chosen on the host by the id: the three branches above and their kernels stay as they
// were, machine code included.  With them: the derivative of sum_j l_j with respect to the parameter (hb_lik_param_grad_*)
// and the predictive log density log E p(y_j | f) of all seven (hb_lik_logdens_*).
// sum_j l_j: every block folds its threads' terms (a grid-stride loop, a fixed grid for a given N) into one partial, a
// second launch of one block adds the partials in block order.  No atomics: two runs give the same bits.
// HB_LIK_HETGAUSS (y ~ N(f, exp(g + c)), two latent functions) has entries of its own at the end of the file
// (hb_lik_hetgauss_*); the one-latent entries refuse its id as they refuse HB_LIK_SOFTMAX.
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

// ------------------------------------------------------------------ likelihoods with a parameter of their own
#define LK_SQRT_PI 1.77245385090551602730
#define LK_MAX_DIGAMMA_TRIPS 11

// psi(x) for x > 0 in double: the recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 10 (at most 11 steps: a tiny x gives
// x + 1 == 1, then 1 .. 9), then ln x - 1 / 2x - sum_n B_2n / (2n x^2n) through x^-14; the first term left out,
// 3617 / (8160 x^16), is below 5e-17 there.  NaN and +inf pass through.
__device__ __forceinline__ double lk_digamma(double x) {
  double r = 0.0;
  for (int t = 0; t < LK_MAX_DIGAMMA_TRIPS && x < 10.0; ++t) {
    r -= 1.0 / x;
    x += 1.0;
  }
  const double f = 1.0 / (x * x);
  return r + log(x) - 0.5 / x -
         f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132 - f * (691.0 / 32760 - f * (1.0 / 12)))))));
}

// Laplace moments under f ~ N(mu, v), d = mu - y: A = E|y - f|, er = erf(d / sqrt(2 v)), dens = N(y; mu, v)
__device__ __forceinline__ void lk_laplace_moments(double y, double mu, double v, double* A, double* er, double* dens) {
  const double d = mu - y;
  if (v > 0.0) {
    const double s = sqrt(2.0 * v), ex = exp(-(d * d) / (2.0 * v));
    const double e = erf(d / s);
    *er = e;
    *A = s * ex / LK_SQRT_PI + d * e;
    *dens = ex / (s * LK_SQRT_PI);
  } else {
    *er = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
    *A = fabs(d);
    *dens = 0.0;
  }
}

// l, g = E dlog p/df, lam = E -d2log p/df2 of the site and, with GRAD, dl = dl / dparam (HB_LIK_BINOMIAL: dl = 0)
template <bool GRAD>
__device__ __forceinline__ void lk_zoo_site(int lik, double y, double mu, double v, double p, double* l, double* g, double* lam,
                                            double* dl) {
  *dl = 0.0;
  if (lik == HB_LIK_LAPLACE) {
    double A, er, dens;
    lk_laplace_moments(y, mu, v, &A, &er, &dens);
    *l = -log(2.0 * p) - A / p;
    *g = -er / p;
    *lam = 2.0 * dens / p;
    if (GRAD) *dl = -1.0 / p + A / (p * p);
  } else if (lik == HB_LIK_GAMMA) {
    const double yE = y * exp(-mu + 0.5 * v), ly = log(y), lp = log(p);
    *l = p * lp - lgamma(p) + (p - 1.0) * ly - p * mu - p * yE;
    *g = -p + p * yE;
    *lam = p * yE;
    if (GRAD) *dl = lp + 1.0 - lk_digamma(p) + ly - mu - yE;
  } else {
    // the two 20-node likelihoods: log p = c + y t - n softplus(t) = c - y softplus(-t) - (n - y) softplus(t), t = f - shift.
    // l is summed in the second form: its terms share a sign, where y t and n softplus(t) cancel in the tails (y = n = 1000
    // at t = 37: both 3.7e4, their difference 1e-13)
    const bool nb = lik == HB_LIK_NEGBINOMIAL;
    const double shift = nb ? log(p) : 0.0, n = nb ? y + p : p, neg = nb ? p : p - y;   // neg = n - y weighs sigmoid(t) in g
    const double sd = sqrt(2.0 * v), m0 = mu - shift;
    double sl = 0.0, sg = 0.0, sh = 0.0, ssp = 0.0, ssg = 0.0;
#pragma unroll 4
    for (int i = 0; i < LK_GH; ++i) {
      const double t = m0 + sd * LK_X[i];
      double sp, sn, e;
      lk_sigmoids(t, &sp, &sn, &e);
      const double l1pe = log1p(e), softplus = (t > 0.0 ? t : 0.0) + l1pe, softminus = (t < 0.0 ? -t : 0.0) + l1pe;
      sl -= LK_W[i] * (y * softminus + neg * softplus);
      sg += LK_W[i] * (y * sn - neg * sp);
      sh += LK_W[i] * (sp * sn);
      if (GRAD) {
        ssp += LK_W[i] * softplus;
        ssg += LK_W[i] * sp;
      }
    }
    const double c = nb ? lgamma(y + p) - lgamma(p) - lgamma(y + 1.0) : lgamma(p + 1.0) - lgamma(y + 1.0) - lgamma(p - y + 1.0);
    *l = c + sl;
    *g = sg;
    *lam = n * sh;
    if (GRAD && nb) *dl = lk_digamma(y + p) - lk_digamma(p) - y / p - ssp + (n / p) * ssg;
  }
}

template <typename T>
__global__ void __launch_bounds__(LK_THREADS) lik_zoo_sites_kernel(int lik, const T* __restrict__ y, const T* __restrict__ mean,
                                                                   const T* __restrict__ var, double mscale, double vscale,
                                                                   double param, T* __restrict__ lam, T* __restrict__ beta,
                                                                   double* __restrict__ partial, long N) {
  __shared__ double red[16];
  const long stride = (long)gridDim.x * LK_THREADS;
  double s = 0.0;
  for (long j = (long)blockIdx.x * LK_THREADS + threadIdx.x; j < N; j += stride) {
    const double mu = mscale * (double)mean[j];
    double l, g, la, dl;
    lk_zoo_site<false>(lik, (double)y[j], mu, vscale * (double)var[j], param, &l, &g, &la, &dl);
    lam[j] = lk_out<T>(la);
    beta[j] = lk_out<T>(g + la * mu);
    s += l;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

template <typename T>
__global__ void __launch_bounds__(LK_THREADS) lik_zoo_predict_kernel(int lik, const T* __restrict__ mean,
                                                                     const T* __restrict__ var, double param,
                                                                     T* __restrict__ ymean, T* __restrict__ yvar, long N) {
  const long stride = (long)gridDim.x * LK_THREADS;
  for (long j = (long)blockIdx.x * LK_THREADS + threadIdx.x; j < N; j += stride) {
    const double mu = (double)mean[j], v = (double)var[j];
    double om, ov;
    if (lik == HB_LIK_LAPLACE) {
      om = mu;
      ov = v + 2.0 * param * param;
    } else if (lik == HB_LIK_BINOMIAL) {
      const double sd = sqrt(2.0 * v);
      double p = 0.0, a = 0.0, b = 0.0;
#pragma unroll 4
      for (int i = 0; i < LK_GH; ++i) {
        double sp, sn, e;
        lk_sigmoids(mu + sd * LK_X[i], &sp, &sn, &e);
        p += LK_W[i] * sp;
        a += LK_W[i] * (sp * sn);
      }
#pragma unroll 4
      for (int i = 0; i < LK_GH; ++i) {   // E (sigmoid - p)^2 once p is known: no E sigmoid^2 - p^2
        double sp, sn, e;
        lk_sigmoids(mu + sd * LK_X[i], &sp, &sn, &e);
        b += LK_W[i] * ((sp - p) * (sp - p));
      }
      om = param * p;
      ov = param * a + param * param * b;
    } else {
      const double e = exp(mu + 0.5 * v), over = expm1(v) + exp(v) / param;
      om = e;
      ov = lik == HB_LIK_GAMMA ? e * e * over : e + e * e * over;
    }
    ymean[j] = lk_out<T>(om);
    yvar[j] = lk_out<T>(ov);
  }
}

// partial[0 .. nb) the blocks' sums of l_j, partial[nb .. 2 nb) of dl_j / dparam
template <typename T>
__global__ void __launch_bounds__(LK_THREADS) lik_param_grad_kernel(int lik, const T* __restrict__ y, const T* __restrict__ mean,
                                                                    const T* __restrict__ var, double mscale, double vscale,
                                                                    double param, double* __restrict__ partial, long N) {
  __shared__ double red[16];
  const long stride = (long)gridDim.x * LK_THREADS;
  double s = 0.0, sd = 0.0;
  for (long j = (long)blockIdx.x * LK_THREADS + threadIdx.x; j < N; j += stride) {
    const double yj = (double)y[j], mu = mscale * (double)mean[j], v = vscale * (double)var[j];
    double l, g, la, dl;
    if (lik == HB_LIK_GAUSSIAN) {
      const double dy = yj - mu;
      lk_site(lik, yj, mu, v, param, &l, &la, &g);
      dl = -1.0 / (2.0 * param) + (dy * dy + v) / (2.0 * param * param);
    } else {
      lk_zoo_site<true>(lik, yj, mu, v, param, &l, &g, &la, &dl);
    }
    s += l;
    sd += dl;
  }
  s = block_sum(s, red);
  sd = block_sum(sd, red);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = s;
    partial[gridDim.x + blockIdx.x] = sd;
  }
}

// block r: row r of the partials [rows, nb] in block order, as lik_sites_fold_kernel folds its one row
__global__ void __launch_bounds__(LK_THREADS) lik_fold_rows_kernel(const double* __restrict__ partial, long nb,
                                                                   double* __restrict__ out) {
  __shared__ double red[16];
  const double* row = partial + (long)blockIdx.x * nb;
  double s = 0.0;
  for (long k = threadIdx.x; k < nb; k += LK_THREADS) s += row[k];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// log of e^(v / 2b^2) [e^(-d/b) erfc(z1) + e^(d/b) erfc(z2)] / 4b, d = y - mu, z1,2 = (v / b -+ d) / sqrt(2 v).  A term with
// z >= 0 is -d^2 / 2v + log erfcx(z) (z^2 cancels the exponent); z1 + z2 > 0, so at most one term takes the other route,
// where erfc is in (1, 2] and its exponent is negative.
__device__ __forceinline__ double lk_laplace_logdens(double y, double mu, double v, double b) {
  const double d = y - mu;
  if (!(v > 0.0)) return -log(2.0 * b) - fabs(d) / b;
  const double s = sqrt(2.0 * v), q = (d * d) / (2.0 * v), c = v / (2.0 * b * b);
  const double z1 = (v / b - d) / s, z2 = (v / b + d) / s;
  const double t1 = z1 >= 0.0 ? -q + log(erfcx(z1)) : c - d / b + log(erfc(z1));
  const double t2 = z2 >= 0.0 ? -q + log(erfcx(z2)) : c + d / b + log(erfc(z2));
  const double m = t1 > t2 ? t1 : t2;
  return -log(4.0 * b) + m + log(exp(t1 - m) + exp(t2 - m));
}

// log sum_i w_i p(y | f_i) for the five likelihoods the rule serves:
//   log p(y | f) = c - wn softplus(-t) - wp softplus(t) + a t - k exp(s t),  t = f - shift
// (the logit and negative binomial ones through the two softplus terms, which share a sign -- y t - n softplus(t) cancels
// in the tails; Poisson and Gamma through a and k).  Combined as c + top + log S, S = sum_i w_i exp(lp_i - top) <= 1.  Where
// S > 1/2 (the mass spread over the nodes: a result that can be near 0 and must keep its digits) log S is taken as
// log1p(sum_i w_i expm1(lp_i - top)), every term <= 0; where S is small (one far node carries it, S = its weight) that sum
// is 1 - (nearly 1) and log S is taken directly.
__device__ __forceinline__ double lk_quad_logdens(int lik, double y, double mu, double v, double p) {
  double c = 0.0, wn = 0.0, wp = 0.0, a = 0.0, k = 0.0, sgn = 1.0, shift = 0.0;
  if (lik == HB_LIK_BERNOULLI) {
    wn = y;
    wp = 1.0 - y;
  } else if (lik == HB_LIK_POISSON) {
    a = y;
    k = 1.0;
    c = -lgamma(y + 1.0);
  } else if (lik == HB_LIK_GAMMA) {
    a = -p;
    k = p * y;
    sgn = -1.0;
    c = p * log(p) - lgamma(p) + (p - 1.0) * log(y);
  } else if (lik == HB_LIK_NEGBINOMIAL) {
    wn = y;
    wp = p;
    shift = log(p);
    c = lgamma(y + p) - lgamma(p) - lgamma(y + 1.0);
  } else {
    wn = y;
    wp = p - y;
    c = lgamma(p + 1.0) - lgamma(y + 1.0) - lgamma(p - y + 1.0);
  }
  const bool logit = k == 0.0;
  const double sd = sqrt(2.0 * v), m0 = mu - shift;
  double lp[LK_GH], top = -INFINITY;
#pragma unroll
  for (int i = 0; i < LK_GH; ++i) {
    const double t = m0 + sd * LK_X[i];
    double val;
    if (logit) {
      const double l1pe = log1p(exp(-fabs(t)));
      val = -(wn * ((t < 0.0 ? -t : 0.0) + l1pe) + wp * ((t > 0.0 ? t : 0.0) + l1pe));
    } else {
      val = a * t - k * exp(sgn * t);
    }
    lp[i] = val;
    top = val > top ? val : top;
  }
  if (!(top > -INFINITY)) return top + lp[0];   // every node at -inf, or a NaN input: NaN is passed on, not turned into -inf
  double s = 0.0, s1 = 0.0;
#pragma unroll
  for (int i = 0; i < LK_GH; ++i) {
    const double d = lp[i] - top;
    s += LK_W[i] * exp(d);
    s1 += LK_W[i] * expm1(d);
  }
  return c + top + (s > 0.5 ? log1p(s1) : log(s));
}

template <typename T>
__global__ void __launch_bounds__(LK_THREADS) lik_logdens_kernel(int lik, const T* __restrict__ y, const T* __restrict__ mean,
                                                                 const T* __restrict__ var, double mscale, double vscale,
                                                                 double param, T* __restrict__ out, double* __restrict__ partial,
                                                                 long N) {
  __shared__ double red[16];
  const long stride = (long)gridDim.x * LK_THREADS;
  double s = 0.0;
  for (long j = (long)blockIdx.x * LK_THREADS + threadIdx.x; j < N; j += stride) {
    const double yj = (double)y[j], mu = mscale * (double)mean[j], v = vscale * (double)var[j];
    double ld;
    if (lik == HB_LIK_GAUSSIAN) {
      const double dy = yj - mu, tot = v + param;
      ld = -0.5 * log(6.283185307179586477 * tot) - (dy * dy) / (2.0 * tot);
    } else if (lik == HB_LIK_LAPLACE) {
      ld = lk_laplace_logdens(yj, mu, v, param);
    } else {
      ld = lk_quad_logdens(lik, yj, mu, v, param);
    }
    if (out) out[j] = lk_out<T>(ld);
    s += ld;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

static inline long lk_blocks(long N) {
  const long nb = (N + LK_THREADS - 1) / LK_THREADS;
  return nb < 1 ? 1 : (nb > LK_MAX_BLOCKS ? LK_MAX_BLOCKS : nb);
}

static inline bool lk_has_own_param(int lik) { return lik >= HB_LIK_LAPLACE && lik <= HB_LIK_BINOMIAL; }

static int lk_check(const char* who, int lik, long N, double param) {
  HB_REQUIRE(lik != HB_LIK_HETGAUSS, "%s: HB_LIK_HETGAUSS has two latent functions: use hb_lik_hetgauss_*", who);
  HB_REQUIRE(lik == HB_LIK_GAUSSIAN || lik == HB_LIK_BERNOULLI || lik == HB_LIK_POISSON || lk_has_own_param(lik),
             "%s: unknown likelihood id %d", who, lik);
  HB_REQUIRE(N >= 0, "%s: negative N (%ld)", who, N);
  HB_REQUIRE(lik != HB_LIK_GAUSSIAN || param > 0.0, "%s: the Gaussian likelihood needs a variance > 0 (got %g)", who, param);
  HB_REQUIRE(lik != HB_LIK_LAPLACE || param > 0.0, "%s: the Laplace likelihood needs a scale > 0 (got %g)", who, param);
  HB_REQUIRE(lik != HB_LIK_GAMMA || param > 0.0, "%s: the Gamma likelihood needs a shape > 0 (got %g)", who, param);
  HB_REQUIRE(lik != HB_LIK_NEGBINOMIAL || param > 0.0, "%s: the negative binomial likelihood needs a dispersion > 0 (got %g)",
             who, param);
  HB_REQUIRE(lik != HB_LIK_BINOMIAL || (param >= 1.0 && param == floor(param)),
             "%s: the binomial likelihood needs an integer total count >= 1 (got %g)", who, param);
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
    if (lk_has_own_param(lik))
      hipLaunchKernelGGL((lik_zoo_sites_kernel<T>), dim3((unsigned)nb), dim3(LK_THREADS), 0, st, lik, y, mean, var, mscale,
                         vscale, param, lam, beta, ws, N);
    else
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
  if (lk_has_own_param(lik))
    hipLaunchKernelGGL((lik_zoo_predict_kernel<T>), dim3((unsigned)lk_blocks(N)), dim3(LK_THREADS), 0, st, lik, mean, var,
                       param, ymean, yvar, N);
  else
    hipLaunchKernelGGL((lik_predict_kernel<T>), dim3((unsigned)lk_blocks(N)), dim3(LK_THREADS), 0, st, lik, mean, var, param,
                       ymean, yvar, N);
  HB_LAUNCH_CHECK();
  return 0;
}

extern "C" long hb_lik_param_grad_ws_elems(long N) { return N > 0 ? 2 * lk_blocks(N) : 1; }

template <typename T>
static int lik_param_grad(int lik, const T* y, const T* mean, const T* var, double mscale, double vscale, double param,
                          double* out, long N, double* ws, hipStream_t st) {
  if (lk_check("hb_lik_param_grad", lik, N, param)) return -1;
  HB_REQUIRE(lik == HB_LIK_GAUSSIAN || lik == HB_LIK_LAPLACE || lik == HB_LIK_GAMMA || lik == HB_LIK_NEGBINOMIAL,
             "hb_lik_param_grad: likelihood id %d has no continuous parameter", lik);
  HB_REQUIRE(out && ws, "hb_lik_param_grad: NULL output / workspace pointer");
  HB_REQUIRE(N == 0 || (y && mean && var), "hb_lik_param_grad: NULL pointer");
  HB_REQUIRE(vscale >= 0.0, "hb_lik_param_grad: vscale must not be negative (got %g)", vscale);
  const long nb = N > 0 ? lk_blocks(N) : 0;
  if (nb > 0) {
    hipLaunchKernelGGL((lik_param_grad_kernel<T>), dim3((unsigned)nb), dim3(LK_THREADS), 0, st, lik, y, mean, var, mscale,
                       vscale, param, ws, N);
    HB_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(lik_fold_rows_kernel, dim3(2), dim3(LK_THREADS), 0, st, ws, nb, out);
  HB_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int lik_logdens(int lik, const T* y, const T* mean, const T* var, double mscale, double vscale, double param, T* out,
                       double* sum, long N, double* ws, hipStream_t st) {
  if (lk_check("hb_lik_logdens", lik, N, param)) return -1;
  HB_REQUIRE(sum && ws, "hb_lik_logdens: NULL output / workspace pointer");
  HB_REQUIRE(N == 0 || (y && mean && var), "hb_lik_logdens: NULL pointer");
  HB_REQUIRE(vscale >= 0.0, "hb_lik_logdens: vscale must not be negative (got %g)", vscale);
  const long nb = N > 0 ? lk_blocks(N) : 0;
  if (nb > 0) {
    hipLaunchKernelGGL((lik_logdens_kernel<T>), dim3((unsigned)nb), dim3(LK_THREADS), 0, st, lik, y, mean, var, mscale, vscale,
                       param, out, ws, N);
    HB_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(lik_sites_fold_kernel, dim3(1), dim3(LK_THREADS), 0, st, ws, nb, sum);
  HB_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------ heteroscedastic Gaussian: y ~ N(f, exp(g + c))
// Closed forms throughout (the header has them).  e = exp(-mu_g - c + v_g / 2) overflows double only past an argument of
// 709; the outputs then saturate (lk_out) or are inf in double, as the Poisson moments do.
template <typename T>
__global__ void __launch_bounds__(LK_THREADS) lik_hetgauss_sites_kernel(const T* __restrict__ y, const T* __restrict__ mean,
                                                                        const T* __restrict__ var, long ld, double mscale,
                                                                        double vscale, double c, T* __restrict__ lam,
                                                                        T* __restrict__ beta, T* __restrict__ r,
                                                                        double* __restrict__ partial, long N) {
  __shared__ double red[16];
  const long stride = (long)gridDim.x * LK_THREADS;
  double s = 0.0;
  for (long j = (long)blockIdx.x * LK_THREADS + threadIdx.x; j < N; j += stride) {
    const double mf = mscale * (double)mean[j], vf = vscale * (double)var[j];
    const double mg = mscale * (double)mean[ld + j], vg = vscale * (double)var[ld + j];
    const double dy = (double)y[j] - mf, sq = dy * dy + vf, e = exp(-mg - c + 0.5 * vg), hse = 0.5 * (sq * e);
    const double rf = dy * e, rg = -0.5 + hse;
    lam[j] = lk_out<T>(e);
    lam[ld + j] = lk_out<T>(hse);
    beta[j] = lk_out<T>(rf + e * mf);
    beta[ld + j] = lk_out<T>(rg + hse * mg);
    if (r) {
      r[j] = lk_out<T>(rf);
      r[ld + j] = lk_out<T>(rg);
    }
    s += -0.91893853320467274178 - 0.5 * (mg + c) - hse;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

template <typename T>
__global__ void __launch_bounds__(LK_THREADS) lik_hetgauss_predict_kernel(const T* __restrict__ mean, const T* __restrict__ var,
                                                                          long ld, double c, T* __restrict__ ymean,
                                                                          T* __restrict__ yvar, long N) {
  const long stride = (long)gridDim.x * LK_THREADS;
  for (long j = (long)blockIdx.x * LK_THREADS + threadIdx.x; j < N; j += stride) {
    ymean[j] = lk_out<T>((double)mean[j]);
    yvar[j] = lk_out<T>((double)var[j] + exp((double)mean[ld + j] + c + 0.5 * (double)var[ld + j]));
  }
}

// log sum_i w_i N(y; mu_f, v_f + exp(mu_g + c + sqrt(2 v_g) x_i)), by log-sum-exp over the nodes
__device__ __forceinline__ double lk_hetgauss_logdens(double y, double mf, double vf, double mg, double vg, double c) {
  const double dy = y - mf, sd = sqrt(2.0 * vg), m0 = mg + c;
  double lp[LK_GH], top = -INFINITY;
#pragma unroll
  for (int i = 0; i < LK_GH; ++i) {
    const double tot = vf + exp(m0 + sd * LK_X[i]);
    const double val = -0.5 * log(6.283185307179586477 * tot) - (dy * dy) / (2.0 * tot);
    lp[i] = val;
    top = val > top ? val : top;
  }
  if (!(top > -INFINITY)) return top + lp[0];   // every node at -inf, or a NaN input: NaN is passed on
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < LK_GH; ++i) s += LK_W[i] * exp(lp[i] - top);
  return top + log(s);
}

template <typename T>
__global__ void __launch_bounds__(LK_THREADS) lik_hetgauss_logdens_kernel(const T* __restrict__ y, const T* __restrict__ mean,
                                                                          const T* __restrict__ var, long ld, double mscale,
                                                                          double vscale, double c, T* __restrict__ out,
                                                                          double* __restrict__ partial, long N) {
  __shared__ double red[16];
  const long stride = (long)gridDim.x * LK_THREADS;
  double s = 0.0;
  for (long j = (long)blockIdx.x * LK_THREADS + threadIdx.x; j < N; j += stride) {
    const double l = lk_hetgauss_logdens((double)y[j], mscale * (double)mean[j], vscale * (double)var[j],
                                         mscale * (double)mean[ld + j], vscale * (double)var[ld + j], c);
    if (out) out[j] = lk_out<T>(l);
    s += l;
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

static int lk_hetgauss_check(const char* who, long N, long ld, double c, double vscale) {
  HB_REQUIRE(N >= 0, "%s: negative N (%ld)", who, N);
  HB_REQUIRE(ld >= N, "%s: the rows must be at least N apart (ld=%ld, N=%ld)", who, ld, N);
  HB_REQUIRE(c == c && c - c == 0.0, "%s: the mean of the log variance must be finite (got %g)", who, c);
  HB_REQUIRE(vscale >= 0.0, "%s: vscale must not be negative (got %g)", who, vscale);
  return 0;
}

extern "C" long hb_lik_hetgauss_ws_elems(long N) { return N > 0 ? lk_blocks(N) : 1; }

template <typename T>
static int lik_hetgauss_sites(const T* y, const T* mean, const T* var, long ld, double mscale, double vscale, double c, T* lam,
                              T* beta, T* r, double* ell_sum, long N, double* ws, hipStream_t st) {
  if (lk_hetgauss_check("hb_lik_hetgauss_sites", N, ld, c, vscale)) return -1;
  HB_REQUIRE(ell_sum && ws, "hb_lik_hetgauss_sites: NULL output / workspace pointer");
  HB_REQUIRE(N == 0 || (y && mean && var && lam && beta), "hb_lik_hetgauss_sites: NULL pointer");
  const long nb = N > 0 ? lk_blocks(N) : 0;
  if (nb > 0) {
    hipLaunchKernelGGL((lik_hetgauss_sites_kernel<T>), dim3((unsigned)nb), dim3(LK_THREADS), 0, st, y, mean, var, ld, mscale,
                       vscale, c, lam, beta, r, ws, N);
    HB_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(lik_sites_fold_kernel, dim3(1), dim3(LK_THREADS), 0, st, ws, nb, ell_sum);
  HB_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int lik_hetgauss_predict(const T* mean, const T* var, long ld, double c, T* ymean, T* yvar, long N, hipStream_t st) {
  if (lk_hetgauss_check("hb_lik_hetgauss_predict", N, ld, c, 0.0)) return -1;
  if (N == 0) return 0;
  HB_REQUIRE(mean && var && ymean && yvar, "hb_lik_hetgauss_predict: NULL pointer");
  hipLaunchKernelGGL((lik_hetgauss_predict_kernel<T>), dim3((unsigned)lk_blocks(N)), dim3(LK_THREADS), 0, st, mean, var, ld, c,
                     ymean, yvar, N);
  HB_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int lik_hetgauss_logdens(const T* y, const T* mean, const T* var, long ld, double mscale, double vscale, double c, T* out,
                                double* sum, long N, double* ws, hipStream_t st) {
  if (lk_hetgauss_check("hb_lik_hetgauss_logdens", N, ld, c, vscale)) return -1;
  HB_REQUIRE(sum && ws, "hb_lik_hetgauss_logdens: NULL output / workspace pointer");
  HB_REQUIRE(N == 0 || (y && mean && var), "hb_lik_hetgauss_logdens: NULL pointer");
  const long nb = N > 0 ? lk_blocks(N) : 0;
  if (nb > 0) {
    hipLaunchKernelGGL((lik_hetgauss_logdens_kernel<T>), dim3((unsigned)nb), dim3(LK_THREADS), 0, st, y, mean, var, ld, mscale,
                       vscale, c, out, ws, N);
    HB_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(lik_sites_fold_kernel, dim3(1), dim3(LK_THREADS), 0, st, ws, nb, sum);
  HB_LAUNCH_CHECK();
  return 0;
}

extern "C" int hb_lik_hetgauss_sites_f32(const float* y, const float* mean, const float* var, long ld, double mscale,
                                         double vscale, double param, float* lam, float* beta, float* r, double* ell_sum,
                                         long N, double* ws, void* stream) {
  return lik_hetgauss_sites<float>(y, mean, var, ld, mscale, vscale, param, lam, beta, r, ell_sum, N, ws, (hipStream_t)stream);
}
extern "C" int hb_lik_hetgauss_sites_f64(const double* y, const double* mean, const double* var, long ld, double mscale,
                                         double vscale, double param, double* lam, double* beta, double* r, double* ell_sum,
                                         long N, double* ws, void* stream) {
  return lik_hetgauss_sites<double>(y, mean, var, ld, mscale, vscale, param, lam, beta, r, ell_sum, N, ws, (hipStream_t)stream);
}
extern "C" int hb_lik_hetgauss_predict_f32(const float* mean, const float* var, long ld, double param, float* ymean,
                                           float* yvar, long n, void* stream) {
  return lik_hetgauss_predict<float>(mean, var, ld, param, ymean, yvar, n, (hipStream_t)stream);
}
extern "C" int hb_lik_hetgauss_predict_f64(const double* mean, const double* var, long ld, double param, double* ymean,
                                           double* yvar, long n, void* stream) {
  return lik_hetgauss_predict<double>(mean, var, ld, param, ymean, yvar, n, (hipStream_t)stream);
}
extern "C" int hb_lik_hetgauss_logdens_f32(const float* y, const float* mean, const float* var, long ld, double mscale,
                                           double vscale, double param, float* out, double* sum, long N, double* ws,
                                           void* stream) {
  return lik_hetgauss_logdens<float>(y, mean, var, ld, mscale, vscale, param, out, sum, N, ws, (hipStream_t)stream);
}
extern "C" int hb_lik_hetgauss_logdens_f64(const double* y, const double* mean, const double* var, long ld, double mscale,
                                           double vscale, double param, double* out, double* sum, long N, double* ws,
                                           void* stream) {
  return lik_hetgauss_logdens<double>(y, mean, var, ld, mscale, vscale, param, out, sum, N, ws, (hipStream_t)stream);
}
extern "C" int hb_lik_param_grad_f32(int lik, const float* y, const float* mean, const float* var, double mscale, double vscale,
                                     double param, double* out, long N, double* ws, void* stream) {
  return lik_param_grad<float>(lik, y, mean, var, mscale, vscale, param, out, N, ws, (hipStream_t)stream);
}
extern "C" int hb_lik_param_grad_f64(int lik, const double* y, const double* mean, const double* var, double mscale,
                                     double vscale, double param, double* out, long N, double* ws, void* stream) {
  return lik_param_grad<double>(lik, y, mean, var, mscale, vscale, param, out, N, ws, (hipStream_t)stream);
}
extern "C" int hb_lik_logdens_f32(int lik, const float* y, const float* mean, const float* var, double mscale, double vscale,
                                  double param, float* out, double* sum, long N, double* ws, void* stream) {
  return lik_logdens<float>(lik, y, mean, var, mscale, vscale, param, out, sum, N, ws, (hipStream_t)stream);
}
extern "C" int hb_lik_logdens_f64(int lik, const double* y, const double* mean, const double* var, double mscale, double vscale,
                                  double param, double* out, double* sum, long N, double* ws, void* stream) {
  return lik_logdens<double>(lik, y, mean, var, mscale, vscale, param, out, sum, N, ws, (hipStream_t)stream);
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
