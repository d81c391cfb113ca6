// Seeding of the per-lane xoroshiro128+ states (hb_rng_init, rng.hip): splitmix64 and the (seed, stream, lane) -> (s0, s1)
// map.  Self-contained (no #include, plain integer arithmetic) so that a host build can take it as ordinary C++ next to
// rng_core.cuh (tests/host_rng).
#ifndef HB_RNG_SEED_CUH
#define HB_RNG_SEED_CUH

__host__ __device__ static inline uint64_t hb_splitmix64(uint64_t& x) {
  uint64_t z = (x += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// State of lane t of stream `stream_id` under `seed`: distinct lanes and streams start splitmix64 from distinct points,
// one step decorrelates them, and the next two outputs are the state (never all zero: xoroshiro's fixed point).
__host__ __device__ static inline void hb_rng_seed_lane(uint64_t seed, uint64_t stream_id, uint64_t t, uint64_t& s0, uint64_t& s1) {
  uint64_t x = seed ^ (stream_id * 0xD1342543DE82EF95ull) ^ (t * 0x9E3779B97F4A7C15ull);
  x = hb_splitmix64(x) ^ t;
  s0 = hb_splitmix64(x);
  s1 = hb_splitmix64(x);
  if (s0 == 0 && s1 == 0) s1 = 0x9E3779B97F4A7C15ull;
}

#endif  // HB_RNG_SEED_CUH
