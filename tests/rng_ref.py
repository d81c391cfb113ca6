"""Exact host model of the per-lane noise generator (csrc/rng_core.cuh, csrc/rng.hip) and of the way every kernel that
draws noise assigns generator lanes to outputs.  Written from the algorithm's description -- splitmix64 seeding,
xoroshiro128+ with the constants 24 / 16 / 37, Box-Muller -- over numpy uint64 with wrap-around arithmetic.

A state is ONE uint64 array of 2 * nlanes words, s0 of every lane and then s1 of every lane: the layout of the device
array, so `Rng.state` read back (int64 viewed as uint64) compares with it word for word.

The stream layout all draw sites share: pair p of an output of n values is elements 2p and 2p + 1, and it is draw
number p // nlanes of lane p % nlanes.  A lane that owns no pair is not touched.  fp64 pairs take two generator steps
(radius, then angle), fp32 pairs one (upper 32 bits radius, lower 32 bits angle).
"""
import numpy as np

U64 = np.uint64
MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
STREAM_MUL = 0xD1342543DE82EF95
TWO_M53 = 2.0 ** -53
TWO_M32_F32 = np.float32(2.0 ** -32)
# largest |z| an fp32 pair can hold: u1 >= 2^-32, so r <= sqrt(64 ln 2)
F32_MAX_ABS = float(np.sqrt(64.0 * np.log(2.0)))


def _u(a):
    return np.asarray(a, dtype=U64)


def _rotl(x, k):
    return (x << U64(k)) | (x >> U64(64 - k))


def splitmix64(x):
    """One step: returns (advanced x, output).  x: uint64 array."""
    with np.errstate(over="ignore"):
        x = x + U64(GOLDEN)
        z = x.copy()
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return x, z ^ (z >> U64(31))


def init_state(seed, stream_id, nlanes):
    """The state hb_rng_init leaves: lane t starts splitmix64 from seed ^ stream*C1 ^ t*C2, takes one step and mixes t in
    again, and the next two outputs are s0, s1 (never both zero)."""
    t = np.arange(nlanes, dtype=U64)
    with np.errstate(over="ignore"):
        x = U64(int(seed) & MASK) ^ U64((int(stream_id) * STREAM_MUL) & MASK) ^ (t * U64(GOLDEN))
    x, z = splitmix64(x)
    x = z ^ t
    x, a = splitmix64(x)
    x, b = splitmix64(x)
    b = np.where((a == 0) & (b == 0), U64(GOLDEN), b)
    return np.concatenate([a, b])


def next_(s0, s1):
    """xoroshiro128+: returns (output, new s0, new s1); arrays or scalars of uint64."""
    s0, s1 = _u(s0), _u(s1)
    with np.errstate(over="ignore"):
        r = s0 + s1
    b = s1 ^ s0
    return r, _rotl(s0, 24) ^ b ^ (b << U64(16)), _rotl(b, 37)


def next_int(s0, s1):
    """The same step over Python ints (the anchor of the CPU tests is checked against both)."""
    r = (s0 + s1) & MASK
    b = s0 ^ s1
    rot = lambda x, k: ((x << k) | (x >> (64 - k))) & MASK
    return r, rot(s0, 24) ^ b ^ ((b << 16) & MASK), rot(b, 37)


# ---------------------------------------------------------------------------------------------------- variates
def uniform_pos(x):
    """(0, 1] from one output: ((x >> 11) + 1) 2^-53 (exact in float64)."""
    return ((_u(x) >> U64(11)).astype(np.float64) + 1.0) * TWO_M53


def uniform(x):
    """[0, 1) from one output: (x >> 11) 2^-53."""
    return (_u(x) >> U64(11)).astype(np.float64) * TWO_M53


def _sincos_rev(u):
    """sin and cos of u revolutions (u in [0, 1], float64), accurate to an ulp of the result also next to their zeros:
    the angle is reduced exactly to an eighth of a turn around the nearest multiple of a quarter turn first."""
    u = np.asarray(u, dtype=np.float64)
    k = np.rint(4.0 * u)
    r = u - k / 4.0                          # exact: |r| <= 1/8, a difference of neighbours in the same binade or below
    s, c = np.sin(2.0 * np.pi * r), np.cos(2.0 * np.pi * r)
    q = k.astype(np.int64) & 3
    sn = np.choose(q, [s, c, -s, -c])
    cs = np.choose(q, [c, -s, -c, s])
    return sn, cs


def normal_f64(xa, xb):
    """The fp64 pair from two consecutive outputs: radius from the first, angle from the second."""
    u1, u2 = uniform_pos(xa), uniform(xb)
    r = np.sqrt(-2.0 * np.log(u1))
    sn, cs = _sincos_rev(u2)
    return r * cs, r * sn


def f32_uniforms(x):
    """u1 in (0, 1] and u2 in [0, 1] of an fp32 pair, in float32 exactly as the kernel forms them: the 32-bit half
    converted to float32 (round to nearest even), `+ 1.0f` for u1, times 2^-32.  u1 = 1 at hi = 0xFFFFFFFF (2^32 + 1 rounds to
    2^32) and u2 = 1 at lo = 0xFFFFFFFF are part of the contract."""
    x = _u(x)
    hi = (x >> U64(32)).astype(np.uint32)
    lo = (x & U64(0xFFFFFFFF)).astype(np.uint32)
    u1 = (hi.astype(np.float32) + np.float32(1.0)) * TWO_M32_F32
    u2 = lo.astype(np.float32) * TWO_M32_F32
    return u1, u2


def normal_f32(x):
    """The fp32 pair from ONE output, evaluated in float64 from the float32 u1, u2: what the hardware log2 / sqrt / sin /
    cos approximate."""
    u1, u2 = f32_uniforms(x)
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    sn, cs = _sincos_rev(u2.astype(np.float64))
    return r * cs, r * sn


# ---------------------------------------------------------------------------------------------------- streams
def _split(state, nlanes):
    state = _u(state)
    assert state.shape == (2 * nlanes,), (state.shape, nlanes)
    return state[:nlanes].copy(), state[nlanes:].copy()


def draws(state, nlanes, counts_steps):
    """Advance lane t by counts_steps[t] steps.  Returns (out, new state): out[k, t] is output number k of lane t (0 where
    the lane takes fewer steps)."""
    s0, s1 = _split(state, nlanes)
    counts = np.asarray(counts_steps, dtype=np.int64)
    assert counts.shape == (nlanes,)
    kmax = int(counts.max()) if nlanes else 0
    out = np.zeros((kmax, nlanes), dtype=U64)
    for k in range(kmax):
        live = counts > k
        r, a, b = next_(s0[live], s1[live])
        out[k, live] = r
        s0[live], s1[live] = a, b
    return out, np.concatenate([s0, s1])


def pair_counts(nlanes, npairs):
    """How many of the pairs 0 .. npairs-1 fall on each lane (pair p on lane p % nlanes)."""
    t = np.arange(nlanes, dtype=np.int64)
    return np.maximum(0, (npairs - t + nlanes - 1) // nlanes)


def fill(state, nlanes, n, dtype):
    """n normals as every fill / fused sampler draws them.  dtype 'f32' or 'f64'.  Returns (values as float64 [n], new state,
    the raw outputs used: [npairs] for f32, [npairs, 2] for f64)."""
    npairs = (n + 1) // 2
    per = 2 if dtype == "f64" else 1
    counts = pair_counts(nlanes, npairs)
    out, new = draws(state, nlanes, counts * per)
    p = np.arange(npairs, dtype=np.int64)
    lane, k = p % nlanes, p // nlanes
    if dtype == "f64":
        xa, xb = out[2 * k, lane], out[2 * k + 1, lane]
        z0, z1 = normal_f64(xa, xb)
        raw = np.stack([xa, xb], axis=1)
    else:
        raw = out[k, lane]
        z0, z1 = normal_f32(raw)
    vals = np.empty(2 * npairs, dtype=np.float64)
    vals[0::2], vals[1::2] = z0, z1
    return vals[:n], new, raw


def mulhi64(x, m):
    return (int(x) * int(m)) >> 64


def randint(state, nlanes, n, lo, hi):
    """n integers in [lo, hi): value i is draw number i // nlanes of lane i % nlanes, lo + floor(x (hi - lo) / 2^64)."""
    counts = pair_counts(nlanes, n)
    out, new = draws(state, nlanes, counts)
    i = np.arange(n, dtype=np.int64)
    xs = out[i // nlanes, i % nlanes]
    vals = np.array([lo + mulhi64(x, hi - lo) for x in xs], dtype=np.int64).reshape(n)
    return vals, new


# ---------------------------------------------------------------------------------------------------- per-site maps
def gather_draw(state, nlanes, n, lo, hi):
    """MultiGather.launch_draw (gather_draw_body): output row r takes ONE step of lane r; needs n <= nlanes."""
    assert n <= nlanes
    counts = (np.arange(nlanes) < n).astype(np.int64)
    out, new = draws(state, nlanes, counts)
    return np.array([lo + mulhi64(x, hi - lo) for x in out[0, :n]], dtype=np.int64).reshape(n), new


def sgp_in_strip(state, nlanes, total):
    """The finishing pass inside the sparse-GP strip kernel (fp32, total = E n even): the pair of the flat indices
    idx = e n + j and idx + 1 takes ONE step of lane idx >> 1; needs nlanes >= total / 2."""
    assert total % 2 == 0 and nlanes >= total // 2
    counts = (np.arange(nlanes) < total // 2).astype(np.int64)
    out, new = draws(state, nlanes, counts)
    z0, z1 = normal_f32(out[0, :total // 2])
    vals = np.empty(total, dtype=np.float64)
    vals[0::2], vals[1::2] = z0, z1
    return vals, new, out[0, :total // 2]


ENC_L = 16


def encoder(state, nlanes, rows):
    """The fused encoder (mlp.hip, fp32): lane 2 row + half takes four steps; normal number k = 2 step + (0: cos, 1: sin) of
    that lane is latent column 4 half + (k & 3) + 8 (k >> 2) of the row.  Needs nlanes >= 2 rows."""
    assert nlanes >= 2 * rows
    counts = 4 * (np.arange(nlanes) < 2 * rows).astype(np.int64)
    out, new = draws(state, nlanes, counts)
    u = np.empty((rows, ENC_L), dtype=np.float64)
    raw = np.empty((rows, 2, 4), dtype=U64)
    for half in range(2):
        lanes = 2 * np.arange(rows) + half
        for step in range(4):
            x = out[step, lanes]
            raw[:, half, step] = x
            z = normal_f32(x)
            for which in range(2):
                k = 2 * step + which
                u[:, 4 * half + (k & 3) + 8 * (k >> 2)] = z[which]
    return u, new, raw


# ---------------------------------------------------------------------------------------------------- crafted states
def state_for_output(x, s1=0x0123456789ABCDEF):
    """(s0, s1) of one lane whose NEXT output is x: s0 = x - s1 (mod 2^64)."""
    return (int(x) - int(s1)) & MASK, int(s1) & MASK


def state_before(s0, s1):
    """The state one step BEFORE (s0, s1): the transition is a bijection (s1' = rotl(b, 37), s0' = rotl(s0, 24) ^ b ^ (b << 16)
    with b = s0 ^ s1).  With state_for_output it gives a lane whose SECOND output is a chosen value."""
    rotr = lambda x, k: ((x >> k) | (x << (64 - k))) & MASK
    b = rotr(int(s1), 37)
    a = rotr(int(s0) ^ b ^ ((b << 16) & MASK), 24)
    return a, a ^ b


def state_for_second_output(x, s1=0x0123456789ABCDEF):
    return state_before(*state_for_output(x, s1))


def i64(state):
    """The state as the int64 words `Rng.state` holds."""
    return _u(state).view(np.int64)
