// Bodies of the SMALL kernels of the step -- the flat-buffer Adam update, the one-workgroup Gaussian likelihood head, the
// sparse-GP finishing pass, the lengthscale-gradient fold -- written once, as device functions of a (first thread,
// thread count) pair, and used twice:
//   * by their ahead-of-time kernels (adam.hip, elementwise.hip, sgp.hip, gram.hip), which pass their own grid;
//   * by run-time generated SERIAL CHAIN kernels (csrc/jit.hip, hb_chain_*): several dependent small launches of a plan
//     (sparse-GP finish -> likelihood head -> its elementwise cluster;  lengthscale fold -> gradient cluster -> Adam)
//     become ONE workgroup of 1024 threads that runs them back to back with a barrier in between -- a kernel boundary
//     inside the captured step costs ~4.5 us, more than any of these bodies takes.
// The Adam update and the two folds come in two parts -- a LOAD part that only requests the operands of a thread and a
// COMPUTE-AND-STORE part that takes them -- and as the composition of the two under the old name: the ahead-of-time kernels
// call the composition, a chain calls the load parts of all its jobs before the first job runs (csrc/jit.hip,
// chain_source_hoist).  Same arithmetic in the same order either way.  The one-workgroup likelihood head and the sparse-GP
// finishing pass are NOT split: their operands are what the job in front of them wrote, so inside a chain they load after
// their barrier as before (the head only gained the LDS slots for its three sums).
// Part of the hiprtc prelude: keep this file self-contained (needs ew_math.cuh and rng_core.cuh before it; no #include).
#ifndef HB_CHAIN_BODIES_CUH
#define HB_CHAIN_BODIES_CUH

// Floating-point contraction OFF in this file (as in ew_math.cuh / ew_apply.cuh): the same body must return the same
// bits from its ahead-of-time kernel and from a run-time generated chain, whatever each compiler would have fused.
#pragma clang fp contract(off)

// A zero the compiler cannot see through, in a vector register: a load of ONE address by all threads indexed with it stays
// a vector load.  As a scalar load it would be waited for where it is issued (scalar loads return out of order, so the
// compiler waits for all of them at the first use of any), one round trip after the other in a phase whose point is to
// have every request in flight at once.
__device__ __forceinline__ long hb_opaque_zero() {
  int z = 0;
  asm volatile("" : "+v"(z));
  return (long)z;
}

// ---------------------------------------------------------------------------------------------------------------- Adam
// Failure containment (reference behaviour: tf.cholesky raises inside session.run BEFORE apply_gradients, so the
// parameters stay at the last good step).  Calls are asynchronous here, so the update itself looks at this step's
// factorisation status words (`info[n_info]`, LAPACK convention, written earlier in the same stream / graph), at
// the all-reduced failure flag of the other ranks (`dpflag`, nullable) and at the sticky record `fail[2]`
// (nullable): if any is non-zero the launch is a no-op -- theta, m, v and the step counter keep their values --
// and `fail` records the first failing step {t+1, first non-zero status seen}.  Every later step is then a no-op
// too, until the host clears `fail`.
// The check in two parts, so that a serial chain can issue the loads long before it needs the answer: hb_adam_status_load
// only REQUESTS the step counter, the sticky record, the rank flag and this thread's first status word;
// hb_adam_status_blocked evaluates them (and walks the status words past the first blockDim.x, if any).
// (The load part has no branch: a load under a condition is waited for at the end of its block.  Where a pointer is NULL
// or there is no status word, the step counter's address is loaded instead and the value ignored by the second part.)
template <typename T>
struct HbAdamStatus {
  long tnow, fail0;
  T dpf;
  int w0;
};
template <typename T>
__device__ __forceinline__ void hb_adam_status_load(const long* t, const int* info, long n_info, const T* dpflag, const long* fail,
                                                    HbAdamStatus<T>& s) {
  const long z = hb_opaque_zero();
  const long* fp = fail != nullptr ? fail : t;
  const T* dp = dpflag != nullptr ? dpflag : reinterpret_cast<const T*>(t);
  const int* ip = n_info > 0 ? info + ((long)threadIdx.x < n_info ? (long)threadIdx.x : n_info - 1) : reinterpret_cast<const int*>(t);
  s.tnow = t[z];
  s.fail0 = fp[z];
  s.dpf = dp[z];
  s.w0 = ip[z];
}
template <typename T>
__device__ __forceinline__ int hb_adam_status_blocked(const HbAdamStatus<T>& s, const long* t, const int* info, long n_info,
                                                      const T* dpflag, long* fail, bool record) {
  int bad = 0, what = 0;
  if (fail != nullptr && s.fail0 != 0) bad = 1;
  if (dpflag != nullptr && s.dpf != (T)0) { bad = 1; what = -1; }
  if ((long)threadIdx.x < n_info && s.w0 != 0) { bad = 1; what = s.w0; }
  for (long i = (long)threadIdx.x + blockDim.x; i < n_info; i += blockDim.x) {
    const int w = info[i];
    if (w != 0) { bad = 1; what = w; }
  }
  const int any = __syncthreads_or(bad);
  if (any && record && fail != nullptr) {
    // one writer: the lowest thread that saw a status word (or thread 0 for the flag-only case)
    __shared__ int who;
    if (threadIdx.x == 0) who = blockDim.x;
    __syncthreads();
    if (what != 0) atomicMin(&who, (int)threadIdx.x);
    __syncthreads();
    const int writer = who == (int)blockDim.x ? 0 : who;
    if ((int)threadIdx.x == writer && fail[0] == 0) {
      fail[1] = (long)what;
      fail[0] = t[0] + 1;
    }
  }
  return any;
}
template <typename T>
__device__ __forceinline__ int adam_step_blocked(const long* t, const int* info, long n_info, const T* dpflag,
                                                 long* fail, bool record) {
  HbAdamStatus<T> s;
  hb_adam_status_load<T>(t, info, n_info, dpflag, fail, s);
  return hb_adam_status_blocked<T>(s, t, info, n_info, dpflag, fail, record);
}

// The first D elements of a thread (i0, i0 + stride, ...), requested before anything is used: theta, m, v
// (hb_adam_load_tmv) and the gradient (hb_adam_load_g; a chain may take it from an LDS window instead).
template <typename T, int D>
struct HbAdamOps {
  T g[D], m[D], v[D], th[D];
};
template <typename T, int D>
__device__ __forceinline__ void hb_adam_load_tmv(const T* theta, const T* m, const T* v, long n, long i0, long stride,
                                                 HbAdamOps<T, D>& o) {
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const long i = i0 + k * stride, ic = i < n ? i : (n > 0 ? n - 1 : 0);
    o.m[k] = m[ic], o.v[k] = v[ic], o.th[k] = theta[ic];
  }
}
template <typename T, int D>
__device__ __forceinline__ void hb_adam_load_g(const T* g, long n, long i0, long stride, HbAdamOps<T, D>& o) {
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const long i = i0 + k * stride, ic = i < n ? i : (n > 0 ? n - 1 : 0);
    o.g[k] = g[ic];
  }
}
// the bias-corrected step size of step tnow + 1
template <typename T>
__device__ __forceinline__ T hb_adam_lr(double lr, double b1, double b2, long tnow) {
  const double tt = (double)(tnow + 1);
  return (T)(lr * sqrt(1.0 - pow(b2, tt)) / (1.0 - pow(b1, tt)));
}
struct HbNoMirror {
  template <typename T>
  __device__ __forceinline__ void operator()(const T*, T) const {}
};

// The update proper, from operands that are already loaded (the compute-and-store part): the first D elements of the
// thread from `o`, any further ones from memory.  `on_theta(address, value)` sees every parameter stored (a serial chain
// mirrors them into the LDS window of a later job; HbNoMirror otherwise).
template <typename T, int D, typename F>
__device__ __forceinline__ void hb_adam_body(T* __restrict__ theta, const T* __restrict__ g, T* __restrict__ m, T* __restrict__ v,
                                             long n, T lr_t, double b1, double b2, double eps, double gscale, long i0, long stride,
                                             const HbAdamOps<T, D>& o, F on_theta) {
  const T c1 = (T)b1, c2 = (T)b2, d1 = (T)(1.0 - b1), d2 = (T)(1.0 - b2), e = (T)eps, gs = (T)gscale;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const long i = i0 + k * stride;
    if (i < n) {
      const T gi = o.g[k] * gs;
      const T mi = c1 * o.m[k] + d1 * gi;
      const T vi = c2 * o.v[k] + d2 * gi * gi;
      m[i] = mi;
      v[i] = vi;
      const T ti = o.th[k] - lr_t * mi / (hb_sqrt(vi) + e);
      theta[i] = ti;
      on_theta(theta + i, ti);
    }
  }
  for (long i = i0 + D * stride; i < n; i += stride) {
    const T gi = g[i] * gs;
    const T mi = c1 * m[i] + d1 * gi;
    const T vi = c2 * v[i] + d2 * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const T ti = theta[i] - lr_t * mi / (hb_sqrt(vi) + e);
    theta[i] = ti;
    on_theta(theta + i, ti);
  }
}
// the single workgroup that owns a whole update advances the step counter itself (it read `tnow` from t[0] in this launch)
__device__ __forceinline__ void hb_adam_tick(long* t, long tnow) {
  if (threadIdx.x == 0) t[0] = tnow + 1;
}

// i0 / stride: this thread's first element and the thread count of the whole launch; `record`: this workgroup writes the
// failure record; `owner`: this workgroup is the only one of the launch (it may advance the step counter itself)
template <typename T>
__device__ __forceinline__ void hb_adam_body(T* __restrict__ theta, const T* __restrict__ g, T* __restrict__ m, T* __restrict__ v,
                                             long n, double lr, double b1, double b2, double eps, double gscale, long* t,
                                             int tick, const int* info, long n_info, const T* dpflag, long* fail, long i0,
                                             long stride, bool record, bool owner) {
  // The first batch of operands (8 elements per thread: a 2048-parameter model in one go) and the step counter are
  // requested BEFORE the status check: the check, the counter and the update were three dependent memory round
  // trips in a kernel whose arithmetic is a few hundred cycles.
  constexpr int U = 8;
  HbAdamOps<T, U> o;
  hb_adam_load_g<T, U>(g, n, i0, stride, o);
  hb_adam_load_tmv<T, U>(theta, m, v, n, i0, stride, o);
  HbAdamStatus<T> s;
  hb_adam_status_load<T>(t, info, n_info, dpflag, fail, s);
  if (hb_adam_status_blocked<T>(s, t, info, n_info, dpflag, fail, record)) return;
  const T lr_t = hb_adam_lr<T>(lr, b1, b2, s.tnow);
  hb_adam_body<T>(theta, g, m, v, n, lr_t, b1, b2, eps, gscale, i0, stride, o, HbNoMirror());
  if (owner && tick) {
    // a single block owns the whole update: it advances the step counter itself (every thread has read
    // t[0] by the barrier), saving the separate tick launch
    __syncthreads();
    hb_adam_tick(t, s.tnow);
  }
}

// Large parameter sets (several workgroups): 16 bytes per lane and array, every operand of a thread requested before the
// first is used.  theta, g, m, v 16-byte aligned; the n % (16 / sizeof(T)) trailing elements are updated one by one by the
// first threads of the launch.  One status check per workgroup.
template <typename T>
__device__ __forceinline__ void hb_adam_body_vec(T* __restrict__ theta, const T* __restrict__ g, T* __restrict__ m, T* __restrict__ v,
                                                 long n, double lr, double b1, double b2, double eps, double gscale, long* t,
                                                 const int* info, long n_info, const T* dpflag, long* fail, long i0, long stride,
                                                 bool record) {
  constexpr int VEC = 16 / (int)sizeof(T), U = 2;
  typedef T VT __attribute__((ext_vector_type(VEC)));
  const long nv = n / VEC;
  VT g0[U], m0[U], v0[U], th0[U];
#pragma unroll
  for (int k = 0; k < U; ++k) {
    const long i = i0 + k * stride, ic = i < nv ? i : (nv > 0 ? nv - 1 : 0);
    g0[k] = reinterpret_cast<const VT*>(g)[ic], m0[k] = reinterpret_cast<const VT*>(m)[ic];
    v0[k] = reinterpret_cast<const VT*>(v)[ic], th0[k] = reinterpret_cast<const VT*>(theta)[ic];
  }
  const long tnow = t[0];
  if (adam_step_blocked<T>(t, info, n_info, dpflag, fail, record)) return;
  const T lr_t = hb_adam_lr<T>(lr, b1, b2, tnow);
  const T c1 = (T)b1, c2 = (T)b2, d1 = (T)(1.0 - b1), d2 = (T)(1.0 - b2), e = (T)eps, gs = (T)gscale;
  auto upd = [&](VT gv, VT mv, VT vv, VT tv, long i) {
    VT mo, vo, to;
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
      const T gi = gv[q] * gs;
      const T mi = c1 * mv[q] + d1 * gi;
      const T vi = c2 * vv[q] + d2 * gi * gi;
      mo[q] = mi, vo[q] = vi, to[q] = tv[q] - lr_t * mi / (hb_sqrt(vi) + e);
    }
    reinterpret_cast<VT*>(m)[i] = mo;
    reinterpret_cast<VT*>(v)[i] = vo;
    reinterpret_cast<VT*>(theta)[i] = to;
  };
#pragma unroll
  for (int k = 0; k < U; ++k) {
    const long i = i0 + k * stride;
    if (i < nv) upd(g0[k], m0[k], v0[k], th0[k], i);
  }
  for (long i = i0 + U * stride; i < nv; i += stride)
    upd(reinterpret_cast<const VT*>(g)[i], reinterpret_cast<const VT*>(m)[i], reinterpret_cast<const VT*>(v)[i],
        reinterpret_cast<const VT*>(theta)[i], i);
  const long it = nv * VEC + i0;
  if (it < n) {
    const T gi = g[it] * gs;
    const T mi = c1 * m[it] + d1 * gi;
    const T vi = c2 * v[it] + d2 * gi * gi;
    m[it] = mi;
    v[it] = vi;
    theta[it] -= lr_t * mi / (hb_sqrt(vi) + e);
  }
}

// ------------------------------------------------------------------------------------- Gaussian likelihood head (one WG)
// sum_j log N(x_j | f_j * scale, var) with its gradients, n <= 16 * blockDim.x: every load of a thread is in flight before
// the first use.  blockDim.x = 1024.  fbar (nullable): also scale * (post * dmu_j), the gradient of post * ll w.r.t. f.
template <typename T>
__device__ __forceinline__ void hb_gauss_ll_single_body(const T* __restrict__ x, const T* __restrict__ f, const T* __restrict__ scale,
                                                        const T* __restrict__ var, long n, T* __restrict__ dmu, T* __restrict__ ll,
                                                        T* __restrict__ dscale, T* __restrict__ dvar, T* smem,
                                                        T* __restrict__ fbar = nullptr, T post = T(0), T* mir = nullptr) {
  constexpr int PER = 16;
  const T s = scale ? scale[0] : T(1), v = var[0];
  const T iv = T(1) / v, lc = T(-0.91893853320467274178) - T(0.5) * hb_log(v);
  T xv[PER], fv[PER];
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const long j = q * 1024 + threadIdx.x;
    const long jc = j < n ? j : n - 1;
    xv[q] = x[jc];
    fv[q] = f[jc];
  }
  T all = T(0), asc = T(0), avr = T(0);
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const long j = q * 1024 + threadIdx.x;
    const T dlt = xv[q] - fv[q] * s;
    const T g = dlt * iv;
    if (j < n) {
      dmu[j] = g;
      if (fbar) fbar[j] = s * (post * g);   // the gradient handed to the producer of f: scale * (upstream * dmu), same order as the graph's ops
      all += lc - T(0.5) * dlt * g;
      asc += g * fv[q];
      avr += T(-0.5) * iv + T(0.5) * g * g;
    }
  }
  all = block_sum(all, smem);
  asc = block_sum(asc, smem);
  avr = block_sum(avr, smem);
  if (threadIdx.x == 0) {
    ll[0] = all;
    dscale[0] = asc;
    dvar[0] = avr;
    if (mir) mir[0] = all, mir[1] = asc, mir[2] = avr;   // serial chain: the hand-off slots of a later job (LDS)
  }
}

// One point of the head (the operations of hb_gauss_ll_single_body's loop, for callers outside this file: contraction
// is off HERE, so the forward strip kernel of csrc/sgp.hip gets the head's bits from it)
template <typename T>
__device__ __forceinline__ void hb_gauss_point(T xv, T fv, T s, T iv, T lc, T& g, T& all, T& asc, T& avr) {
  const T dlt = xv - fv * s;
  g = dlt * iv;
  all += lc - T(0.5) * dlt * g;
  asc += g * fv;
  avr += T(-0.5) * iv + T(0.5) * g * g;
}

// Fold of the per-unit partial sums (ll, dscale, dvar) that a multi-workgroup head leaves as partial[3][nb] -- the
// partial-sum kernel of hb_gauss_ll, or the forward strip kernel of hb_sgp_fwd_gauss, one unit per strip.  One workgroup.
// Load part: the first D units of the thread (threadIdx.x, + blockDim.x, ...), three sums each; compute part: the fold of
// those and of any further units, in the order of the plain loop.  mir (nullable): three LDS slots that also get the sums.
template <typename T, int D>
__device__ __forceinline__ void hb_gauss_fold_load(const T* __restrict__ partial, long nb, T (&h)[3 * D]) {
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const long i = (long)threadIdx.x + (long)k * blockDim.x, ic = i < nb ? i : nb - 1;
    h[3 * k] = partial[ic], h[3 * k + 1] = partial[nb + ic], h[3 * k + 2] = partial[2 * nb + ic];
  }
}
template <typename T, int D>
__device__ __forceinline__ void hb_gauss_fold_body(const T (&h)[3 * D], const T* __restrict__ partial, long nb, T* __restrict__ ll,
                                                   T* __restrict__ dscale, T* __restrict__ dvar, T* smem, T* mir = nullptr) {
  T a0 = T(0), a1 = T(0), a2 = T(0);
#pragma unroll
  for (int k = 0; k < D; ++k) {
    if ((long)threadIdx.x + (long)k * blockDim.x < nb) {
      a0 += h[3 * k];
      a1 += h[3 * k + 1];
      a2 += h[3 * k + 2];
    }
  }
  for (long i = (long)threadIdx.x + (long)D * blockDim.x; i < nb; i += blockDim.x) {
    a0 += partial[i];
    a1 += partial[nb + i];
    a2 += partial[2 * nb + i];
  }
  a0 = block_sum(a0, smem);
  a1 = block_sum(a1, smem);
  a2 = block_sum(a2, smem);
  if (threadIdx.x == 0) {
    ll[0] = a0;
    dscale[0] = a1;
    dvar[0] = a2;
    if (mir) mir[0] = a0, mir[1] = a1, mir[2] = a2;
  }
}
template <typename T>
__device__ __forceinline__ void hb_gauss_fold_body(const T* __restrict__ partial, long nb, T* __restrict__ ll, T* __restrict__ dscale,
                                                   T* __restrict__ dvar, T* smem, T* mir = nullptr) {
  T h[3];
  hb_gauss_fold_load<T, 1>(partial, nb, h);
  hb_gauss_fold_body<T, 1>(h, partial, nb, ll, dscale, dvar, smem, mir);
}

// -------------------------------------------------------------------------------------------- sparse-GP finishing pass
// f, v (and the residual noise) from the column partials of the forward contraction: v = 1 - sum A^2, f = u A + sqrt|v| eps.
// The noise is drawn here (same per-lane streams and pair order as the stand-alone fill) or taken from eps_in.
template <typename T>
__device__ __forceinline__ void sgp_finish_one(const T* __restrict__ part, int gy, long idx, T epsv, T* __restrict__ f,
                                               T* __restrict__ v, T* __restrict__ eps_out, long n, long P, int diagonal) {
  const long e = idx / n, j = idx - e * n;
  const T* pp = part + e * gy * 5 * n + j;
  T s = T(0);
  for (int y = 0; y < gy; ++y) s += pp[(long)y * 5 * n];
  const T vv = T(1) - s;
  v[idx] = vv;
  if (eps_out) eps_out[idx] = epsv;
  const T scale = diagonal ? hb_sqrt(hb_abs(vv)) * epsv : T(0);
  for (long p = 0; p < P; ++p) {
    T mean = T(0);
    for (int y = 0; y < gy; ++y) mean += pp[((long)y * 5 + 1 + p) * n];
    f[(e * P + p) * n + j] = mean + scale;
  }
}

// t0 / nthreads: this thread's index in, and the size of, the whole launch.  With an RNG, thread t serves the lanes
// t, t + nthreads, ... (a launch of >= min(nlanes, npairs) threads gives one lane per thread, as the stand-alone kernel does).
template <typename T>
__device__ __forceinline__ void hb_sgp_finish_body(const T* __restrict__ part, int gy, const T* __restrict__ eps_in, uint64_t* rng,
                                                   long nlanes, T* __restrict__ eps_out, T* __restrict__ f, T* __restrict__ v,
                                                   long total, long n, long P, int diagonal, long t0, long nthreads) {
  const long npairs = (total + 1) / 2;
  if (rng) {
    const long nact = nlanes < npairs ? nlanes : npairs;
    for (long t = t0; t < nact; t += nthreads) {
      HbRng g = rng_load(rng, nlanes, t);
      for (long p = t; p < npairs; p += nlanes) {
        T z0, z1;
        g.normal2(z0, z1);
        sgp_finish_one<T>(part, gy, 2 * p, z0, f, v, eps_out, n, P, diagonal);
        if (2 * p + 1 < total) sgp_finish_one<T>(part, gy, 2 * p + 1, z1, f, v, eps_out, n, P, diagonal);
      }
      rng_store(rng, nlanes, t, g);
    }
  } else {
    for (long idx = t0; idx < total; idx += nthreads)
      sgp_finish_one<T>(part, gy, idx, eps_in ? eps_in[idx] : T(0), f, v, (eps_out != eps_in) ? eps_out : nullptr, n, P, diagonal);
  }
}

// ---------------------------------------------------------------------------------- lengthscale-gradient fold (gram_bwd)
// ellbar[c] = sum_r partial[r, c (or all columns when dl == 1)] for one (column c, batch entry): one workgroup
// Load part (the thread's first D partials) and compute part (their fold, then any further ones, in the order of the
// plain loop).  mir (nullable): an LDS slot that also gets the sum.
template <typename T, int D>
__device__ __forceinline__ void hb_gram_ell_load(const T* __restrict__ partial, long rows, long d, long dl, long c, T (&h)[D]) {
  const long cnt = dl == 1 ? rows * d : rows;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const long t = (long)threadIdx.x + (long)k * blockDim.x, tc = t < cnt ? t : cnt - 1;
    h[k] = dl == 1 ? partial[tc] : partial[tc * d + c];
  }
}
template <typename T, int D>
__device__ __forceinline__ void hb_gram_ell_body(const T (&h)[D], const T* __restrict__ partial, long rows, long d, long dl, long c,
                                                 T* __restrict__ ellbar, T* smem, T* mir = nullptr) {
  const long cnt = dl == 1 ? rows * d : rows;
  T acc = T(0);
#pragma unroll
  for (int k = 0; k < D; ++k)
    if ((long)threadIdx.x + (long)k * blockDim.x < cnt) acc += h[k];
  if (dl == 1) {
#pragma unroll 4
    for (long t = (long)threadIdx.x + (long)D * blockDim.x; t < cnt; t += blockDim.x) acc += partial[t];
  } else {
#pragma unroll 4
    for (long r = (long)threadIdx.x + (long)D * blockDim.x; r < cnt; r += blockDim.x) acc += partial[r * d + c];
  }
  acc = block_sum(acc, smem);
  if (threadIdx.x == 0) {
    ellbar[c] = acc;
    if (mir) mir[0] = acc;
  }
}
template <typename T>
__device__ __forceinline__ void hb_gram_ell_body(const T* __restrict__ partial, long rows, long d, long dl, long c,
                                                 T* __restrict__ ellbar, T* smem, T* mir = nullptr) {
  T h[1];
  hb_gram_ell_load<T, 1>(partial, rows, d, dl, c, h);
  hb_gram_ell_body<T, 1>(h, partial, rows, d, dl, c, ellbar, smem, mir);
}

// --------------------------------------------------------------- fold of a Gram VJP's tile partials (hb_gram_tiles_fold)
// part[B][tiles][tiles][32][2 d] is what the tiles-mode product (csrc/linalg.hip, matmul_wgk_kernel<.., TILES>) leaves: for
// every 32 x 32 tile of Kbar, per row, d point-gradient shares and then d lengthscale shares.  Output o of the fold,
// o = (b M + row) 2 d + q, is the sum of the tiles_n shares of its row in ascending tile order: q < d goes to
// Xbar[(b M + row) d + q], q >= d into the lengthscale sum (column q - d, or the one column when dl == 1), which is then
// folded over the rows and the batch into ellbar[dl].  One workgroup; thread t owns the outputs t, t + blockDim.x, ...
// Load part: the shares of the thread's first S outputs (S * TN values); compute part: their sums, any further output from
// memory in the order of the plain loop, the stores and the block sums.  on_xbar(address, value) sees every Xbar stored (a
// serial chain mirrors them into the LDS window of a later job); mir (nullable): an LDS slot that also gets ellbar[0].
#define HB_GRAM_TILES_MAXD 4
// (32-bit index arithmetic: outs and the partials are bounded by HB_CHAIN_TILES_MAX_N where the fold is launched)
__device__ __forceinline__ long hb_gram_tiles_addr(long o, long tiles_n, long d) {
  const unsigned w = 64u * (unsigned)d, g = (unsigned)o / w;   // g = b tiles_m + ti; o - g w = r 2 d + q
  return (long)(g * (unsigned)tiles_n * w + ((unsigned)o - g * w));
}
template <typename T, int S, int TN>
__device__ __forceinline__ void hb_gram_tiles_load(const T* __restrict__ part, long outs, long d, T (&h)[S * TN > 0 ? S * TN : 1]) {
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const long o = (long)threadIdx.x + (long)s * blockDim.x, oc = o < outs ? o : outs - 1;
    const T* p = part + hb_gram_tiles_addr(oc, TN, d);
#pragma unroll
    for (int t = 0; t < TN; ++t) h[s * TN + t] = p[(long)t * 64 * d];
  }
}
template <typename T, int S, int TN, typename F>
__device__ __forceinline__ void hb_gram_tiles_body(const T (&h)[S * TN > 0 ? S * TN : 1], const T* __restrict__ part, long outs, long tiles_n, long d,
                                                   long dl, T* __restrict__ Xbar, T* __restrict__ ellbar, T* smem, F on_xbar,
                                                   T* mir = nullptr) {
  T lp[HB_GRAM_TILES_MAXD];
#pragma unroll
  for (int k = 0; k < HB_GRAM_TILES_MAXD; ++k) lp[k] = T(0);
  auto put = [&](long o, T v) {
    const long row = (long)((unsigned)o / (2u * (unsigned)d)), q = o - row * 2 * d;
    if (q < d) {
      Xbar[row * d + q] = v;
      on_xbar(Xbar + row * d + q, v);
    } else {
      const long c = dl == 1 ? 0 : q - d;
#pragma unroll
      for (int k = 0; k < HB_GRAM_TILES_MAXD; ++k)
        if (c == k) lp[k] += v;
    }
  };
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const long o = (long)threadIdx.x + (long)s * blockDim.x;
    T acc = T(0);
#pragma unroll
    for (int t = 0; t < TN; ++t) acc += h[s * TN + t];
    if (o < outs) put(o, acc);
  }
  for (long o = (long)threadIdx.x + (long)S * blockDim.x; o < outs; o += blockDim.x) {
    const T* p = part + hb_gram_tiles_addr(o, tiles_n, d);
    T acc = T(0);
    for (long t = 0; t < tiles_n; ++t) acc += p[t * 64 * d];
    put(o, acc);
  }
#pragma unroll
  for (int k = 0; k < HB_GRAM_TILES_MAXD; ++k) {
    if (k < dl) {   // (uniform)
      const T e = block_sum(lp[k], smem);
      if (threadIdx.x == 0) {
        ellbar[k] = e;
        if (mir && k == 0) mir[0] = e;
      }
    }
  }
}
// the composition: nothing preloaded, every output from memory
template <typename T, typename F>
__device__ __forceinline__ void hb_gram_tiles_body(const T* __restrict__ part, long outs, long tiles_n, long d, long dl,
                                                   T* __restrict__ Xbar, T* __restrict__ ellbar, T* smem, F on_xbar) {
  const T h[1] = {T(0)};
  hb_gram_tiles_body<T, 0, 1, F>(h, part, outs, tiles_n, d, dl, Xbar, ellbar, smem, on_xbar);
}

// ------------------------------------------------------------------------- serial chains: LDS windows (csrc/jit.hip)
// A window holds the n elements from `base` on that a later job of the chain reads: filled from memory in the load phase
// (hb_chain_win_load requests, hb_chain_win_store writes the LDS copy), then every store of an earlier job that falls
// inside [base, base + n) is repeated into it (hb_chain_mirror), so the consumer reads what a load after the barrier
// would have returned.  One workgroup of blockDim.x threads.
template <typename T, int D>
__device__ __forceinline__ void hb_chain_win_load(const T* base, long n, T (&h)[D]) {
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const long i = (long)threadIdx.x + (long)k * blockDim.x;
    h[k] = base[i < n ? i : hb_opaque_zero()];
  }
}
template <typename T, int D>
__device__ __forceinline__ void hb_chain_win_store(T* win, long n, const T (&h)[D]) {
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const long i = (long)threadIdx.x + (long)k * blockDim.x;
    if (i < n) win[i] = h[k];
  }
}
template <typename T>
__device__ __forceinline__ void hb_chain_mirror(const T* p, T v, const T* base, long n, T* win) {
  const long ob = (long)p - (long)base;
  if (ob >= 0 && ob < n * (long)sizeof(T)) win[ob / (long)sizeof(T)] = v;
}
// the barrier between the window fill and the first job
__device__ __forceinline__ void hb_chain_sync() { __syncthreads(); }

#pragma clang fp contract(fast)
#endif  // HB_CHAIN_BODIES_CUH
