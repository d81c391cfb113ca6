// Sites and predictive of the softmax (multi-class) likelihood under C independent Gaussian marginals
// (hb_lik_softmax_sites_*, hb_lik_softmax_grad_*, hb_lik_softmax_predict_*, include/henbun_hip.h; SparseGP.natgrad_q,
// SparseGP.elbo_and_grad_multi, models.SVGPMulticlass).
//
// For point j with label y_j and f_c ~ N(mu_jc, v_jc), mu = mscale mean, v = vscale var, and S standard-normal nodes
// eps [S, C] shared by all points:
//     f_sc = mu_jc + sqrt(max(v_jc, 0)) eps_sc,   p_s = softmax_c(f_s)
//     l_j = mean_s log p_{s, y_j},   g_jc = mean_s ([c = y_j] - p_sc),   lam_jc = mean_s p_sc (1 - p_sc),
//     beta_jc = g_jc + lam_jc mu_jc;   predict: prob_jc = mean_s p_sc,   logdens_j = log mean_s p_{s, y_j}.
// lam is Price's form of -2 dE l / dv_c; it is never negative, so the conjugate update of q(u_c) stays positive definite.
//
// Layout: a group of CP lanes per point, CP the power of two >= C, so a wave takes 64 / CP points; lane c of the group
// owns class c -- its mu, sqrt(v) and running sums live in registers, nothing is indexed by a class number at run time.
// The maximum, the first lane that holds it and the sum over classes are xor-butterflies inside the group.  Padding lanes
// (c >= C) hold f = -inf and contribute exp(-inf) = 0.  Points past N are computed on clamped loads and masked at the
// store: every lane of a wave reaches every shuffle.
// One softmax: with mx = max_c f_c and `first` the lowest class that attains it, e_c = exp(f_c - mx) for c != first and
// rest = sum_{c != first} e_c, so the sum over classes is 1 + rest EXACTLY as formed:
//     p_first = 1 / (1 + rest),  1 - p_first = rest / (1 + rest);   p_c = e_c / (1 + rest),  1 - p_c by subtraction (p_c <= 1/2)
//     log p_c = (f_c - mx) - log1p(rest).
// No 1 - p where p is near 1: lam and g keep their relative digits when one class carries the mass.
// Arithmetic is double whatever the storage type; one rounding on output.  The nodes go through LDS in tiles of whole
// nodes (SM_TILE doubles); when all of them fit in one tile they are staged once per workgroup.
// sum_j l_j / sum_j logdens_j: every block folds its lanes' terms (a grid-stride loop over point tiles, a fixed grid for a
// given N and C) into one partial, a second launch of one block adds the partials in block order.  No atomics: two runs
// give the same bits.
#include "common.cuh"
#include "../../include/henbun_hip.h"

#define SM_THREADS 256
#define SM_MAX_BLOCKS 1024
#define SM_TILE 4096   // doubles of nodes per LDS tile (32 KB): 64 nodes at C = 64
#define SM_MAX_C 64
#define SM_MAX_S 1024

template <typename T>
__device__ __forceinline__ T sm_out(double x);
template <>
__device__ __forceinline__ double sm_out<double>(double x) { return x; }
template <>
__device__ __forceinline__ float sm_out<float>(double x) {
  const double big = 3.4028234663852886e+38;
  return (float)(x > big ? big : (x < -big ? -big : x));
}

template <int CP>
__device__ __forceinline__ double sm_group_max(double v) {
#pragma unroll
  for (int off = CP / 2; off > 0; off >>= 1) {
    const double o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}
template <int CP>
__device__ __forceinline__ double sm_group_sum(double v) {
#pragma unroll
  for (int off = CP / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
template <int CP>
__device__ __forceinline__ int sm_group_min(int v) {
#pragma unroll
  for (int off = CP / 2; off > 0; off >>= 1) {
    const int o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}

// one softmax over the group: p, q = 1 - p and lp = log p of this lane's class
template <int CP>
__device__ __forceinline__ void sm_softmax(double f, int c, double* p, double* q, double* lp) {
  const double mx = sm_group_max<CP>(f);
  const int first = sm_group_min<CP>(f == mx ? c : CP);
  const double d = f - mx;
  const double e = c == first ? 0.0 : exp(d);
  const double rest = sm_group_sum<CP>(e);
  const double inv = 1.0 / (1.0 + rest);
  if (c == first) {
    *p = inv;
    *q = rest * inv;
  } else {
    *p = e * inv;
    *q = 1.0 - e * inv;
  }
  *lp = d - log1p(rest);
}

// tile t of the nodes into LDS: whole nodes, `per` of them (the last tile: what is left)
__device__ __forceinline__ long sm_stage(const double* __restrict__ nodes, double* tile, long t, long per, long S, long C) {
  const long s0 = t * per, ns = S - s0 < per ? S - s0 : per;
  for (long i = threadIdx.x; i < ns * C; i += SM_THREADS) tile[i] = nodes[s0 * C + i];
  return ns;
}

template <typename T, int CP>
__global__ void __launch_bounds__(SM_THREADS) lik_softmax_sites_kernel(const T* __restrict__ y, const T* __restrict__ mean,
                                                                       const T* __restrict__ var, double mscale, double vscale,
                                                                       const double* __restrict__ nodes, long S,
                                                                       T* __restrict__ lam, T* __restrict__ beta,
                                                                       double* __restrict__ partial, long N, long C) {
  __shared__ double tile[SM_TILE];
  __shared__ double red[16];
  constexpr int PPB = SM_THREADS / CP;
  const int c = threadIdx.x % CP, g = threadIdx.x / CP;
  const bool cls = c < C;
  const long per = SM_TILE / C, ntiles = (S + per - 1) / per;
  const double invS = 1.0 / (double)S;
  long ns = 0;
  if (ntiles == 1) {
    ns = sm_stage(nodes, tile, 0, per, S, C);
    __syncthreads();
  }
  double lsum = 0.0;
  // the trip count depends on the block alone: every thread reaches every barrier and shuffle
  for (long base = (long)blockIdx.x * PPB; base < N; base += (long)gridDim.x * PPB) {
    const long j = base + g, jj = j < N ? j : N - 1;
    double mu = -INFINITY, sd = 0.0;
    int yj = -1;
    if (cls) {
      const double v = vscale * (double)var[c * N + jj];
      mu = mscale * (double)mean[c * N + jj];
      sd = sqrt(v > 0.0 ? v : 0.0);
      yj = (int)(double)y[jj];
    }
    const bool mine = c == yj;
    double gacc = 0.0, lacc = 0.0, ell = 0.0;
    for (long t = 0; t < ntiles; ++t) {
      if (ntiles > 1) {
        __syncthreads();
        ns = sm_stage(nodes, tile, t, per, S, C);
        __syncthreads();
      }
      for (long s = 0; s < ns; ++s) {
        const double f = cls ? mu + sd * tile[s * C + c] : -INFINITY;
        double p, q, lp;
        sm_softmax<CP>(f, c, &p, &q, &lp);
        gacc += mine ? q : -p;
        lacc += p * q;
        ell += mine ? lp : 0.0;
      }
    }
    if (cls && j < N) {
      const double la = lacc * invS, ga = gacc * invS;
      lam[c * N + j] = sm_out<T>(la);
      beta[c * N + j] = sm_out<T>(ga + la * mu);
      if (mine) lsum += ell * invS;
    }
  }
  lsum = block_sum(lsum, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = lsum;
}

// Weights of the hyper-parameter gradient at fixed q (hb_lik_softmax_grad_*): the sites kernel's walk, node tiles, softmax
// and lsum (the same terms added in the same order on the same grid: the same bits), with the reparameterised weight in
// place of Price's lam.  d_sc = [c = y] - p_sc is q on the label lane and -p elsewhere, as in g; with eps = nodes[s, c]
//     r[c, j] = mean_s d_sc,   w[c, j] = -mean_s(d_sc eps_sc) / sqrt(v_jc)   (v_jc > 0: -2 d l_j / d v_jc of the node sum)
//     w[c, j] = mean_s p_sc (1 - p_sc)                                        (v_jc <= 0: eps_sc does not reach f; Price's form)
// w and r are double whatever T, rows `ldo` apart.
template <typename T, int CP>
__global__ void __launch_bounds__(SM_THREADS) lik_softmax_grad_kernel(const T* __restrict__ y, const T* __restrict__ mean,
                                                                      const T* __restrict__ var, double mscale, double vscale,
                                                                      const double* __restrict__ nodes, long S,
                                                                      double* __restrict__ wout, double* __restrict__ rout,
                                                                      long ldo, double* __restrict__ partial, long N, long C) {
  __shared__ double tile[SM_TILE];
  __shared__ double red[16];
  constexpr int PPB = SM_THREADS / CP;
  const int c = threadIdx.x % CP, g = threadIdx.x / CP;
  const bool cls = c < C;
  const long per = SM_TILE / C, ntiles = (S + per - 1) / per;
  const double invS = 1.0 / (double)S;
  long ns = 0;
  if (ntiles == 1) {
    ns = sm_stage(nodes, tile, 0, per, S, C);
    __syncthreads();
  }
  double lsum = 0.0;
  for (long base = (long)blockIdx.x * PPB; base < N; base += (long)gridDim.x * PPB) {
    const long j = base + g, jj = j < N ? j : N - 1;
    double mu = -INFINITY, sd = 0.0;
    int yj = -1;
    if (cls) {
      const double v = vscale * (double)var[c * N + jj];
      mu = mscale * (double)mean[c * N + jj];
      sd = sqrt(v > 0.0 ? v : 0.0);
      yj = (int)(double)y[jj];
    }
    const bool mine = c == yj;
    double gacc = 0.0, lacc = 0.0, wacc = 0.0, ell = 0.0;
    for (long t = 0; t < ntiles; ++t) {
      if (ntiles > 1) {
        __syncthreads();
        ns = sm_stage(nodes, tile, t, per, S, C);
        __syncthreads();
      }
      for (long s = 0; s < ns; ++s) {
        const double eps = cls ? tile[s * C + c] : 0.0;
        const double f = cls ? mu + sd * tile[s * C + c] : -INFINITY;   // the sites kernel's expression: the same bits
        double p, q, lp;
        sm_softmax<CP>(f, c, &p, &q, &lp);
        const double dl = mine ? q : -p;
        gacc += dl;
        wacc = __builtin_fma(dl, eps, wacc);
        lacc += p * q;
        ell += mine ? lp : 0.0;
      }
    }
    if (cls && j < N) {
      rout[c * ldo + j] = gacc * invS;
      wout[c * ldo + j] = sd > 0.0 ? -(wacc * invS) / sd : lacc * invS;
      if (mine) lsum += ell * invS;
    }
  }
  lsum = block_sum(lsum, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = lsum;
}

// HAS_Y: the label lane, and no other, also carries log sum_s p_{s, y} as a running (top, acc) pair,
// acc = sum_s exp(lp_s - top), and sum_s (1 - p_{s, y})
template <typename T, int CP, bool HAS_Y>
__global__ void __launch_bounds__(SM_THREADS) lik_softmax_predict_kernel(const T* __restrict__ y, const T* __restrict__ mean,
                                                                         const T* __restrict__ var, double mscale, double vscale,
                                                                         const double* __restrict__ nodes, long S,
                                                                         T* __restrict__ prob, T* __restrict__ logdens,
                                                                         double* __restrict__ partial, long N, long C) {
  __shared__ double tile[SM_TILE];
  __shared__ double red[16];
  constexpr int PPB = SM_THREADS / CP;
  const int c = threadIdx.x % CP, g = threadIdx.x / CP;
  const bool cls = c < C;
  const long per = SM_TILE / C, ntiles = (S + per - 1) / per;
  const double invS = 1.0 / (double)S, logS = log((double)S);
  long ns = 0;
  if (ntiles == 1) {
    ns = sm_stage(nodes, tile, 0, per, S, C);
    __syncthreads();
  }
  double tsum = 0.0;
  for (long base = (long)blockIdx.x * PPB; base < N; base += (long)gridDim.x * PPB) {
    const long j = base + g, jj = j < N ? j : N - 1;
    double mu = -INFINITY, sd = 0.0;
    int yj = -1;
    if (cls) {
      const double v = vscale * (double)var[c * N + jj];
      mu = mscale * (double)mean[c * N + jj];
      sd = sqrt(v > 0.0 ? v : 0.0);
      if (HAS_Y) yj = (int)(double)y[jj];
    }
    const bool mine = c == yj;
    double pacc = 0.0, qacc = 0.0, top = -INFINITY, acc = 0.0;
    for (long t = 0; t < ntiles; ++t) {
      if (ntiles > 1) {
        __syncthreads();
        ns = sm_stage(nodes, tile, t, per, S, C);
        __syncthreads();
      }
      for (long s = 0; s < ns; ++s) {
        const double f = cls ? mu + sd * tile[s * C + c] : -INFINITY;
        double p, q, lp;
        sm_softmax<CP>(f, c, &p, &q, &lp);
        pacc += p;
        if (HAS_Y && mine) {   // the label lane alone (the shuffles are behind us: only the ALU diverges)
          qacc += q;
          if (lp > top) {
            acc = acc * exp(top - lp) + 1.0;
            top = lp;
          } else {
            acc += exp(lp - top);
          }
        }
      }
    }
    if (cls && j < N) {
      if (prob) prob[c * N + j] = sm_out<T>(pacc * invS);
      if (HAS_Y && mine) {
        // mean p above 1/2: log1p(-mean(1 - p)), which keeps its digits as the density goes to 1 (log of a number near 1
        // would not); else the log-sum-exp, which keeps them as it goes to 0
        const double ld = pacc * invS > 0.5 ? log1p(-(qacc * invS)) : top + log(acc) - logS;
        if (logdens) logdens[j] = sm_out<T>(ld);
        tsum += ld;
      }
    }
  }
  if (HAS_Y) {
    tsum = block_sum(tsum, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tsum;
  }
}

// one block: the partials in block order (thread t takes t, t + 256, ..), then the block's fixed tree
__global__ void __launch_bounds__(SM_THREADS) lik_softmax_fold_kernel(const double* __restrict__ partial, long nb,
                                                                      double* __restrict__ out) {
  __shared__ double red[16];
  double s = 0.0;
  for (long k = threadIdx.x; k < nb; k += SM_THREADS) s += partial[k];
  s = block_sum(s, red);
  if (threadIdx.x == 0) out[0] = s;
}

static inline int sm_group(long C) {
  int cp = 2;
  while (cp < C) cp <<= 1;
  return cp;
}
static inline long sm_blocks(long N, long C) {
  const long ppb = SM_THREADS / sm_group(C), nb = (N + ppb - 1) / ppb;
  return nb < 1 ? 1 : (nb > SM_MAX_BLOCKS ? SM_MAX_BLOCKS : nb);
}

extern "C" long hb_lik_softmax_ws_elems(long N, long C) {
  return N > 0 && C >= 2 && C <= SM_MAX_C ? sm_blocks(N, C) : 1;
}

static int sm_check(const char* who, long N, long C, long S, double vscale) {
  HB_REQUIRE(C >= 2 && C <= SM_MAX_C, "%s: 2 <= C <= %d classes expected (got %ld)", who, SM_MAX_C, C);
  HB_REQUIRE(S >= 1 && S <= SM_MAX_S, "%s: 1 <= S <= %d nodes expected (got %ld)", who, SM_MAX_S, S);
  HB_REQUIRE(N >= 0, "%s: negative N (%ld)", who, N);
  HB_REQUIRE(N * C < (1L << 40), "%s: N C = %ld too large", who, N * C);
  HB_REQUIRE(vscale >= 0.0, "%s: vscale must not be negative (got %g)", who, vscale);
  return 0;
}

#define SM_DISPATCH(CPV, LAUNCH) \
  switch (CPV) {                 \
    case 2: LAUNCH(2); break;    \
    case 4: LAUNCH(4); break;    \
    case 8: LAUNCH(8); break;    \
    case 16: LAUNCH(16); break;  \
    case 32: LAUNCH(32); break;  \
    default: LAUNCH(64); break;  \
  }

template <typename T>
static int lik_softmax_sites(const T* y, const T* mean, const T* var, double mscale, double vscale, const double* nodes, long S,
                             T* lam, T* beta, double* lsum, long N, long C, double* ws, hipStream_t st) {
  if (sm_check("hb_lik_softmax_sites", N, C, S, vscale)) return -1;
  HB_REQUIRE(lsum && ws, "hb_lik_softmax_sites: NULL output / workspace pointer");
  HB_REQUIRE(N == 0 || (y && mean && var && nodes && lam && beta), "hb_lik_softmax_sites: NULL pointer");
  const long nb = N > 0 ? sm_blocks(N, C) : 0;
  if (nb > 0) {
#define SM_LAUNCH_SITES(CP)                                                                                              \
  hipLaunchKernelGGL((lik_softmax_sites_kernel<T, CP>), dim3((unsigned)nb), dim3(SM_THREADS), 0, st, y, mean, var, mscale, \
                     vscale, nodes, S, lam, beta, ws, N, C)
    SM_DISPATCH(sm_group(C), SM_LAUNCH_SITES)
#undef SM_LAUNCH_SITES
    HB_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(lik_softmax_fold_kernel, dim3(1), dim3(SM_THREADS), 0, st, ws, nb, lsum);
  HB_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int lik_softmax_grad(const T* y, const T* mean, const T* var, double mscale, double vscale, const double* nodes, long S,
                            double* w, double* r, long ldo, double* lsum, long N, long C, double* ws, hipStream_t st) {
  if (sm_check("hb_lik_softmax_grad", N, C, S, vscale)) return -1;
  HB_REQUIRE(lsum && ws, "hb_lik_softmax_grad: NULL output / workspace pointer");
  HB_REQUIRE(ldo >= N, "hb_lik_softmax_grad: the output rows must be at least N apart (ldo=%ld, N=%ld)", ldo, N);
  HB_REQUIRE(N == 0 || (y && mean && var && nodes && w && r), "hb_lik_softmax_grad: NULL pointer");
  const long nb = N > 0 ? sm_blocks(N, C) : 0;
  if (nb > 0) {
#define SM_LAUNCH_GRAD(CP)                                                                                              \
  hipLaunchKernelGGL((lik_softmax_grad_kernel<T, CP>), dim3((unsigned)nb), dim3(SM_THREADS), 0, st, y, mean, var, mscale, \
                     vscale, nodes, S, w, r, ldo, ws, N, C)
    SM_DISPATCH(sm_group(C), SM_LAUNCH_GRAD)
#undef SM_LAUNCH_GRAD
    HB_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(lik_softmax_fold_kernel, dim3(1), dim3(SM_THREADS), 0, st, ws, nb, lsum);
  HB_LAUNCH_CHECK();
  return 0;
}

template <typename T>
static int lik_softmax_predict(const T* y, const T* mean, const T* var, double mscale, double vscale, const double* nodes,
                               long S, T* prob, T* logdens, double* total, long N, long C, double* ws, hipStream_t st) {
  if (sm_check("hb_lik_softmax_predict", N, C, S, vscale)) return -1;
  HB_REQUIRE(y || (!logdens && !total), "hb_lik_softmax_predict: logdens and total need the labels y");
  HB_REQUIRE(prob || logdens || total, "hb_lik_softmax_predict: no output asked for");
  const bool has_y = y && (logdens || total);
  HB_REQUIRE(!has_y || ws, "hb_lik_softmax_predict: logdens and total need a workspace (the blocks' partial sums)");
  HB_REQUIRE(N == 0 || (mean && var && nodes), "hb_lik_softmax_predict: NULL pointer");
  const long nb = N > 0 ? sm_blocks(N, C) : 0;
  if (nb > 0) {
#define SM_LAUNCH_PREDICT(CP)                                                                                                \
  if (has_y)                                                                                                                 \
    hipLaunchKernelGGL((lik_softmax_predict_kernel<T, CP, true>), dim3((unsigned)nb), dim3(SM_THREADS), 0, st, y, mean, var, \
                       mscale, vscale, nodes, S, prob, logdens, ws, N, C);                                                   \
  else                                                                                                                       \
    hipLaunchKernelGGL((lik_softmax_predict_kernel<T, CP, false>), dim3((unsigned)nb), dim3(SM_THREADS), 0, st, y, mean, var, \
                       mscale, vscale, nodes, S, prob, logdens, ws, N, C)
    SM_DISPATCH(sm_group(C), SM_LAUNCH_PREDICT)
#undef SM_LAUNCH_PREDICT
    HB_LAUNCH_CHECK();
  }
  if (total) {
    hipLaunchKernelGGL(lik_softmax_fold_kernel, dim3(1), dim3(SM_THREADS), 0, st, ws, nb, total);
    HB_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int hb_lik_softmax_sites_f32(const float* y, const float* mean, const float* var, double mscale, double vscale,
                                        const double* nodes, long S, float* lam, float* beta, double* lsum, long N, long C,
                                        double* ws, void* stream) {
  return lik_softmax_sites<float>(y, mean, var, mscale, vscale, nodes, S, lam, beta, lsum, N, C, ws, (hipStream_t)stream);
}
extern "C" int hb_lik_softmax_sites_f64(const double* y, const double* mean, const double* var, double mscale, double vscale,
                                        const double* nodes, long S, double* lam, double* beta, double* lsum, long N, long C,
                                        double* ws, void* stream) {
  return lik_softmax_sites<double>(y, mean, var, mscale, vscale, nodes, S, lam, beta, lsum, N, C, ws, (hipStream_t)stream);
}
extern "C" int hb_lik_softmax_grad_f32(const float* y, const float* mean, const float* var, double mscale, double vscale,
                                       const double* nodes, long S, double* w, double* r, long ldo, double* lsum, long N, long C,
                                       double* ws, void* stream) {
  return lik_softmax_grad<float>(y, mean, var, mscale, vscale, nodes, S, w, r, ldo, lsum, N, C, ws, (hipStream_t)stream);
}
extern "C" int hb_lik_softmax_grad_f64(const double* y, const double* mean, const double* var, double mscale, double vscale,
                                       const double* nodes, long S, double* w, double* r, long ldo, double* lsum, long N, long C,
                                       double* ws, void* stream) {
  return lik_softmax_grad<double>(y, mean, var, mscale, vscale, nodes, S, w, r, ldo, lsum, N, C, ws, (hipStream_t)stream);
}
extern "C" int hb_lik_softmax_predict_f32(const float* y, const float* mean, const float* var, double mscale, double vscale,
                                          const double* nodes, long S, float* prob, float* logdens, double* total, long n, long C,
                                          double* ws, void* stream) {
  return lik_softmax_predict<float>(y, mean, var, mscale, vscale, nodes, S, prob, logdens, total, n, C, ws, (hipStream_t)stream);
}
extern "C" int hb_lik_softmax_predict_f64(const double* y, const double* mean, const double* var, double mscale, double vscale,
                                          const double* nodes, long S, double* prob, double* logdens, double* total, long n,
                                          long C, double* ws, void* stream) {
  return lik_softmax_predict<double>(y, mean, var, mscale, vscale, nodes, S, prob, logdens, total, n, C, ws,
                                     (hipStream_t)stream);
}
