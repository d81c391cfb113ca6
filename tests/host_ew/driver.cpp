// Host build of the elementwise op table (csrc/ew_math.cuh, csrc/ew_apply.cuh through shim.h).
//   driver digamma [points_f32.bin points_f64.bin]
//       walks hb_digamma over every sign and exponent of float and of double (four mantissas each: 0, 1, the middle,
//       all ones -- zeros, subnormals, infinities and NaNs included), the negative integers and their neighbours and
//       the points of the given files; counts the trips of the recurrence per call through HB_DIGAMMA_TRIP and checks
//       the contract on the special values.  A call that passes TRIP_ABORT trips is abandoned and reported as unbounded.
//       Exit status 1 when any call needed more than HB_DIGAMMA_MAX_TRIPS trips or broke the contract.
//       Built against a csrc whose hb_digamma has no HB_DIGAMMA_TRIP hook (build.sh OUT CSRC_DIR with an older tree),
//       trips cannot be counted: every call then runs under a timer of CALL_LIMIT_MS, a call that has not returned by
//       then is abandoned and reported, and the exit status is 1 when there was one.
//   driver apply f32|f64 OP P0 P1 NIN N in.bin out.bin
//       out[k][i] = ew_apply(OP, in[0][i], .., in[NIN-1][i]) for the op's outputs k (3 for HB_EW_GAUSS_LOGPDF_GRAD).
#include "shim.h"
#include "../../include/henbun_hip.h"
#include <csetjmp>
#include <csignal>
#include <sys/time.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static long g_trips = 0;
static sigjmp_buf g_abort;
#define TRIP_ABORT 100000L
#define HB_DIGAMMA_TRIP()                              \
  do {                                                 \
    if (++g_trips > TRIP_ABORT) siglongjmp(g_abort, 1); \
  } while (0)
#include "ew_math.cuh"
#include "ew_apply.cuh"
#ifdef HB_DIGAMMA_MAX_TRIPS
#define HOOKED 1
static void arm(bool) {}
#else
// a tree from before the bound: no hook, so a timer per call instead of a trip count
#define HOOKED 0
#define HB_DIGAMMA_MAX_TRIPS 6
#define CALL_LIMIT_MS 10
static void on_alarm(int) { siglongjmp(g_abort, 1); }
static void arm(bool on) {
  std::signal(SIGALRM, on_alarm);
  itimerval t = {{0, 0}, {0, on ? CALL_LIMIT_MS * 1000 : 0}};
  setitimer(ITIMER_REAL, &t, nullptr);
}
#endif

template <typename T>
struct Walk {
  long calls = 0, over = 0, unbounded = 0, max_trips = 0, contract = 0;
  T worst = T(0);
  // volatile: the value must survive the longjmp
  T run(T x, bool* finished) {
    volatile T res = T(0);
    g_trips = 0;
    ++calls;
    if (sigsetjmp(g_abort, 1) == 0) {
      arm(true);
      res = hb_digamma<T>(x);
      arm(false);
      *finished = true;
    } else {
      *finished = false;
      ++unbounded;
    }
    if (g_trips > HB_DIGAMMA_MAX_TRIPS) {
      if (g_trips > max_trips) worst = x;
      ++over;
    }
    if (g_trips > max_trips) max_trips = g_trips;
    return res;
  }
  void expect(bool ok, const char* what, T x) {
    if (!ok) {
      ++contract;
      std::printf("  contract: %s at x = %.17g\n", what, (double)x);
    }
  }
};

template <typename T, typename U>
static int walk(const char* name, int ebits, int mbits, const char* points) {
  Walk<T> w;
  bool fin;
  const U mants[4] = {U(0), U(1), U(1) << (mbits - 1), (U(1) << mbits) - 1};
  for (int s = 0; s < 2; ++s)
    for (U e = 0; e < (U(1) << ebits); ++e)
      for (int m = 0; m < 4; ++m) {
        const U bits = (U(s) << (ebits + mbits)) | (e << mbits) | mants[m];
        T x;
        std::memcpy(&x, &bits, sizeof(T));
        const T r = w.run(x, &fin);
        if (!fin) continue;
        if (x != x) w.expect(r != r, "NaN -> NaN", x);
        else if (x > T(0) && std::isinf(x)) w.expect(std::isinf(r) && r > T(0), "+inf -> +inf", x);
        else if (x > T(0)) w.expect(r == r, "x > 0 -> a number (-inf where -1/x overflows)", x);
        else if (x == T(0) && !std::signbit(x)) w.expect(std::isinf(r) && r < T(0), "+0 -> -inf", x);
        else if (x < T(0) && (std::isinf(x) || x == std::floor(x))) w.expect(!std::isfinite(r), "pole or -inf -> non-finite", x);
      }
  for (int k = 1; k <= 40; ++k) {
    const T x = T(-k);
    T r = w.run(x, &fin);
    if (fin) w.expect(!std::isfinite(r), "negative integer -> non-finite", x);
    r = w.run(std::nextafter(x, T(0)), &fin);
    if (fin) w.expect(std::isfinite(r), "neighbour of a negative integer -> finite", x);
    r = w.run(std::nextafter(x, T(-1e30)), &fin);
    if (fin) w.expect(std::isfinite(r), "neighbour of a negative integer -> finite", x);
    r = w.run(x + T(0.5), &fin);
    if (fin) w.expect(std::isfinite(r), "negative half-integer -> finite", x);
  }
  if (points) {
    std::FILE* f = std::fopen(points, "rb");
    if (!f) {
      std::printf("cannot open %s\n", points);
      return 2;
    }
    T x;
    while (std::fread(&x, sizeof(T), 1, f) == 1) w.run(x, &fin);
    std::fclose(f);
  }
#if HOOKED
  std::printf("%s: %ld calls, max trips %ld, over the bound of %d: %ld (abandoned after %ld trips: %ld), contract failures %ld",
              name, w.calls, w.max_trips, (int)HB_DIGAMMA_MAX_TRIPS, w.over, TRIP_ABORT, w.unbounded, w.contract);
  if (w.over) std::printf(", worst x = %.9g", (double)w.worst);
#else
  std::printf("%s: %ld calls, no trip hook in this tree; not returned within %d ms and abandoned: %ld, contract failures %ld",
              name, w.calls, (int)CALL_LIMIT_MS, w.unbounded, w.contract);
#endif
  std::printf("\n");
  return (w.over || w.unbounded || w.contract) ? 1 : 0;
}

template <typename T>
static int apply(int op, const double* p, int nin, long n, const char* in_path, const char* out_path) {
  std::vector<T> in((size_t)nin * n), out;
  std::FILE* f = std::fopen(in_path, "rb");
  if (!f || std::fread(in.data(), sizeof(T), in.size(), f) != in.size()) return 2;
  std::fclose(f);
  const int nout = op == HB_EW_GAUSS_LOGPDF_GRAD ? 3 : 1;
  out.resize((size_t)nout * n);
  for (long i = 0; i < n; ++i) {
    T v[4] = {T(0), T(0), T(0), T(0)}, o[3] = {T(0), T(0), T(0)};
    for (int k = 0; k < nin; ++k) v[k] = in[(size_t)k * n + i];
    g_trips = 0;
    if (sigsetjmp(g_abort, 1) != 0) return 3;
    ew_apply<T>(op, v[0], v[1], v[2], v[3], p, o[0], o[1], o[2]);
    for (int k = 0; k < nout; ++k) out[(size_t)k * n + i] = o[k];
  }
  f = std::fopen(out_path, "wb");
  if (!f || std::fwrite(out.data(), sizeof(T), out.size(), f) != out.size()) return 2;
  std::fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::string(argv[1]) == "digamma") {
    const int a = walk<float, uint32_t>("float", 8, 23, argc >= 4 ? argv[2] : nullptr);
    const int b = walk<double, uint64_t>("double", 11, 52, argc >= 4 ? argv[3] : nullptr);
    if (a == 0 && b == 0) std::printf("digamma: every call within the bound\n");
    return a | b;
  }
  if (argc == 10 && std::string(argv[1]) == "apply") {
    const double p[4] = {std::atof(argv[4]), std::atof(argv[5]), 0.0, 0.0};
    const int op = std::atoi(argv[3]), nin = std::atoi(argv[6]);
    const long n = std::atol(argv[7]);
    if (std::string(argv[2]) == "f32") return apply<float>(op, p, nin, n, argv[8], argv[9]);
    return apply<double>(op, p, nin, n, argv[8], argv[9]);
  }
  std::fprintf(stderr, "usage: driver digamma [f32.bin f64.bin] | driver apply f32|f64 OP P0 P1 NIN N in.bin out.bin\n");
  return 2;
}
