// Host build of the noise generator (csrc/rng_core.cuh, csrc/rng_seed.cuh through shim.h).
//   driver CMDS OUT
// reads one command per line of CMDS and writes one line per result to OUT; every number is a 64-bit (or, for floats, a
// 32-bit) pattern in hexadecimal.
//   next S0 S1 K        K steps of HbRng::next from the state: K lines  "r s0 s1"
//   seed SEED STREAM T  hb_rng_seed_lane:                              "s0 s1"
//   uni S0 S1           HbRng::uniform():                              "bits(double) s0 s1"
//   unipos S0 S1        HbRng::uniform_pos():                          "bits(double) s0 s1"
//   n32 S0 S1           HbRng::normal2(float&, float&):                "bits(u1) bits(u2) bits(z0) bits(z1) s0 s1"
//                       (u1, u2: what normal2 handed to the log and to the cos / sin stand-ins)
//   n64 S0 S1           HbRng::normal2(double&, double&):              "bits(z0) bits(z1) s0 s1"
//   ldst NLANES T       rng_load / next / rng_store of lane T in an array holding 1 .. 2 NLANES:  the 2 NLANES words after
#include "shim.h"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>
#include "rng_core.cuh"
#include "rng_seed.cuh"

static uint64_t bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return b;
}
static uint32_t bits(float v) {
  uint32_t b;
  std::memcpy(&b, &v, 4);
  return b;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: driver CMDS OUT\n");
    return 2;
  }
  std::FILE* in = std::fopen(argv[1], "r");
  std::FILE* out = std::fopen(argv[2], "w");
  if (!in || !out) return 2;
  char cmd[16];
  uint64_t a, b, c;
  while (std::fscanf(in, "%15s", cmd) == 1) {
    const bool three = !std::strcmp(cmd, "next") || !std::strcmp(cmd, "seed");
    if (std::fscanf(in, "%" SCNx64 " %" SCNx64, &a, &b) != 2) return 3;
    if (three && std::fscanf(in, "%" SCNx64, &c) != 1) return 3;
    HbRng g;
    g.s0 = a, g.s1 = b;
    if (!std::strcmp(cmd, "next")) {
      for (uint64_t k = 0; k < c; ++k) {
        const uint64_t r = g.next();
        std::fprintf(out, "%" PRIx64 " %" PRIx64 " %" PRIx64 "\n", r, g.s0, g.s1);
      }
    } else if (!std::strcmp(cmd, "seed")) {
      uint64_t s0, s1;
      hb_rng_seed_lane(a, b, c, s0, s1);
      std::fprintf(out, "%" PRIx64 " %" PRIx64 "\n", s0, s1);
    } else if (!std::strcmp(cmd, "uni") || !std::strcmp(cmd, "unipos")) {
      const double u = cmd[3] ? g.uniform_pos() : g.uniform();
      std::fprintf(out, "%" PRIx64 " %" PRIx64 " %" PRIx64 "\n", bits(u), g.s0, g.s1);
    } else if (!std::strcmp(cmd, "n32")) {
      float z0, z1;
      g.normal2(z0, z1);
      if (g_cos_arg != g_sin_arg && !(g_cos_arg != g_cos_arg)) return 4;   // one angle feeds both
      std::fprintf(out, "%x %x %x %x %" PRIx64 " %" PRIx64 "\n", bits(g_log_arg), bits(g_cos_arg), bits(z0), bits(z1), g.s0, g.s1);
    } else if (!std::strcmp(cmd, "n64")) {
      double z0, z1;
      g.normal2(z0, z1);
      std::fprintf(out, "%" PRIx64 " %" PRIx64 " %" PRIx64 " %" PRIx64 "\n", bits(z0), bits(z1), g.s0, g.s1);
    } else if (!std::strcmp(cmd, "ldst")) {
      const long nlanes = (long)a, t = (long)b;
      std::vector<uint64_t> st(2 * nlanes);
      for (long i = 0; i < 2 * nlanes; ++i) st[i] = (uint64_t)(i + 1);
      HbRng h = rng_load(st.data(), nlanes, t);
      h.next();
      rng_store(st.data(), nlanes, t, h);
      for (long i = 0; i < 2 * nlanes; ++i) std::fprintf(out, "%" PRIx64 "%c", st[i], i + 1 < 2 * nlanes ? ' ' : '\n');
    } else {
      return 5;
    }
  }
  std::fclose(in);
  return std::fclose(out) == 0 ? 0 : 2;
}
