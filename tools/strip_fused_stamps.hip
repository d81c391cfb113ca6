// Diagnostic build of the backward strip kernel and of the fused forward + Kbar strip kernel with in-kernel phase stamps
// for every workgroup and wave (not part of the product), at the cfg-2 shape (M = 512, n = 8192, d = 1, P = 1):
//   hipcc -O3 --offload-arch=gfx950 tools/strip_fused_stamps.hip -o tools/_bin/strip_fused_stamps
// Kbar kernel: 0 entry, 1 after the Abar build's barrier, 2 after the tile loop, 3 end.
// Fused kernel: 0 entry, 1 K block synthesised, 2 forward loop done, 3 epilogue done (the phase boundary), 4 Abar in LDS,
//               5 Kbar loop done, 6 end.
#include <hip/hip_runtime.h>
#define NSTAMP 8
__device__ long long hb_stamps[256 * 8 * NSTAMP];
__device__ long long hb_wall[256 * 2];
#define HB_STAMP_AT(i, last)                                                                                      \
  do {                                                                                                            \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 256) {                                                            \
      hb_stamps[(blockIdx.x * 8 + (threadIdx.x >> 6)) * NSTAMP + (i)] = clock64();                                \
      if (threadIdx.x == 0 && ((i) == 0 || (i) == (last))) hb_wall[blockIdx.x * 2 + ((i) == (last))] = wall_clock64(); \
    }                                                                                                             \
  } while (0)
#define HB_KSTAMP(i) HB_STAMP_AT(i, 3)
#define HB_FSTAMP(i) HB_STAMP_AT(i, 6)
#include "../henbun_amd/csrc/runtime.hip"
#include "../henbun_amd/csrc/elementwise.hip"
#include "../henbun_amd/csrc/gram.hip"
#include "../henbun_amd/csrc/linalg.hip"
#include "../henbun_amd/csrc/sgp.hip"
// (the serial-chain recorder lives in csrc/jit.hip, which this diagnostic build leaves out: nothing is ever recording)
bool hb_chain_recording() { return false; }
int hb_chain_push(const HbChainJob&, hipStream_t) { return 0; }
int hb_chain_flush(hipStream_t) { return 0; }
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static const int M = 512, n = 8192;
static float *x, *z, *ell, *W, *Wf, *u, *eps, *Af, *Abf, *f, *v, *ws, *bws, *y, *var, *dmu, *fbar, *hpart, *Phi, *ubar, *zbar, *ellbar;

static int fwd() {
  return hb_sgp_fwd_gauss_f32(0, 1, x, 0, z, ell, 1, W, Wf, 0, u, eps, nullptr, 0, eps, nullptr, Af, f, v, 1, n, M, 1, 1, ws, y, nullptr, var,
                              2.5, dmu, fbar, hpart, n / 32, 0);
}
static int kbar() {   // the strip kernel of hb_sgp_bwd_phi_f32 alone
  SgpBwdArgs<float> a = sgp_bwd_args<float>(W, u, nullptr, fbar, eps, v, nullptr, n, M, 1, 1, 1);
  const HbWfragLayout lay = hb_wfrag_layout(1, M, false);
  a.x = x; a.sx = 0; a.z = z; a.ell = ell; a.dl = 1;
  a.WTf = Wf + lay.wt; a.plane3 = lay.plane;
  a.part = bws + sgp_ws(1, n, M, 1, 1).shared;
  a.Af = Af; a.Kf = Abf; a.Abf = Abf;
  return sgp_bwd_strip_launch(a, 1, n / 32, 0);
}
static int fused() {
  return hb_sgp_fwd_gauss_kbar_f32(0, 1, x, 0, z, ell, 1, W, Wf, 0, u, eps, nullptr, 0, eps, nullptr, Af, f, v, 1, n, M, 1, 1, ws, y, nullptr,
                                   var, 2.5, dmu, fbar, hpart, n / 32, Abf, bws, 0);
}

template <typename F>
static float back_to_back(F run, const char* what) {
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  for (int i = 0; i < 5; ++i)
    if (run()) { printf("%s: %s\n", what, hb_last_error_string()); exit(1); }
  (void)hipEventRecord(e0);
  for (int i = 0; i < 50; ++i) run();
  (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
  float ms;
  (void)hipEventElapsedTime(&ms, e0, e1);
  printf("%-28s %.2f us per launch (50 back-to-back stream launches)\n", what, ms * 1e3 / 50);
  return ms * 1e3f / 50;
}

static void report(const char* what, int last, const char* const* names) {
  std::vector<long long> st(256 * 8 * NSTAMP), rt(512);
  (void)hipMemcpyFromSymbol(st.data(), HIP_SYMBOL(hb_stamps), st.size() * 8);
  (void)hipMemcpyFromSymbol(rt.data(), HIP_SYMBOL(hb_wall), rt.size() * 8);
  long long t0 = rt[0], t1 = rt[1];
  std::vector<double> durs;
  for (int b = 0; b < 256; ++b) {
    t0 = std::min(t0, rt[2 * b]); t1 = std::max(t1, rt[2 * b + 1]);
    durs.push_back((rt[2 * b + 1] - rt[2 * b]) / 100.0);
  }
  std::sort(durs.begin(), durs.end());
  printf("%s, last launch: first workgroup start -> last workgroup end %.2f us; workgroup durations min %.2f median %.2f max %.2f us (100 MHz wall clock)\n",
         what, (t1 - t0) / 100.0, durs[0], durs[128], durs[255]);
  for (int p = 0; p < last; ++p) {
    std::vector<long long> c;
    for (int i = 0; i < 256 * 8; ++i) c.push_back(st[i * NSTAMP + p + 1] - st[i * NSTAMP + p]);
    std::sort(c.begin(), c.end());
    printf("  %-34s cycles over 2048 waves: min %6lld  median %6lld  p90 %6lld  max %6lld\n", names[p], c[0], c[1024], c[1843], c[2047]);
  }
}

int main() {
  float *K, *L, *cws;
  int* info;
  const long wse = hb_cholesky_inverse_ws_elems(1, M, 4);
  const long sws = hb_sgp_ws_elems(1, n, M, 1, 1);
  (void)hipMalloc(&K, M * M * 4); (void)hipMalloc(&L, M * M * 4); (void)hipMalloc(&W, M * M * 4); (void)hipMalloc(&cws, wse * 4);
  (void)hipMemset(cws, 0, wse * 4);
  (void)hipMalloc(&Wf, 2 * M * M * 4); (void)hipMalloc(&info, 4);
  (void)hipMalloc(&z, M * 4); (void)hipMalloc(&x, n * 4); (void)hipMalloc(&ell, 4); (void)hipMalloc(&u, M * 4); (void)hipMalloc(&eps, n * 4);
  (void)hipMalloc(&Af, (size_t)M * n * 4); (void)hipMalloc(&Abf, (size_t)M * n * 4); (void)hipMalloc(&f, n * 4); (void)hipMalloc(&v, n * 4);
  (void)hipMalloc(&ws, sws * 4); (void)hipMalloc(&bws, sws * 4);
  (void)hipMalloc(&y, n * 4); (void)hipMalloc(&var, 4); (void)hipMalloc(&dmu, n * 4); (void)hipMalloc(&fbar, n * 4); (void)hipMalloc(&hpart, 3 * (n / 32) * 4);
  (void)hipMalloc(&Phi, M * M * 4); (void)hipMalloc(&ubar, M * 4); (void)hipMalloc(&zbar, M * 4); (void)hipMalloc(&ellbar, 4);
  std::vector<float> hz(M), hx(n), hu(M), he(n), hy(n);
  for (int i = 0; i < M; ++i) hz[i] = i * 0.5f, hu[i] = 0.01f * ((i * 37) % 101 - 50);
  for (int i = 0; i < n; ++i) hx[i] = (i % 997) * 0.25f, he[i] = 0.02f * ((i * 53) % 97 - 48), hy[i] = 0.01f * ((i * 29) % 89 - 44);
  float one = 1.f, hv = 0.4f;
  (void)hipMemcpy(z, hz.data(), M * 4, hipMemcpyHostToDevice); (void)hipMemcpy(x, hx.data(), n * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(u, hu.data(), M * 4, hipMemcpyHostToDevice); (void)hipMemcpy(eps, he.data(), n * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(y, hy.data(), n * 4, hipMemcpyHostToDevice);
  (void)hipMemcpy(ell, &one, 4, hipMemcpyHostToDevice); (void)hipMemcpy(var, &hv, 4, hipMemcpyHostToDevice);
  if (hb_gram_fwd_f32(0, z, 0, z, 0, ell, 0, 1, K, 1, M, M, 1, 1e-3, 0)) { printf("gram: %s\n", hb_last_error_string()); return 1; }
  if (hb_cholesky_inverse_f32(K, L, W, 1, M, info, cws, Wf, 0, 0)) { printf("chol: %s\n", hb_last_error_string()); return 1; }
  static const char* const kn[] = {"staging + Abar build (prologue)", "tile loop", "lengthscale fold"};
  static const char* const fn[] = {"K block synthesis", "forward loop", "forward epilogue", "Abar from registers (hand-over)", "Kbar loop", "lengthscale fold"};
  const float tf = back_to_back(fwd, "forward (head inside)");
  const float tk = back_to_back(kbar, "Kbar strip kernel");
  report("Kbar strip kernel", 3, kn);
  const float tu = back_to_back(fused, "fused forward + Kbar");
  report("fused kernel", 6, fn);
  printf("forward + Kbar as two launches %.2f us, fused %.2f us: %.2f us less\n", tf + tk, tu, tf + tk - tu);
  return 0;
}
