"""The noise generator without a GPU: csrc/rng_core.cuh and csrc/rng_seed.cuh compiled for the host (tests/host_rng)
against the exact model of tests/rng_ref.py -- integer streams, seeding and the uniforms bit for bit, the fp64 normals to
a few ulp -- and the properties of the model itself that the device tests (test_rng_contract_gpu.py) rely on."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import rng_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = R.MASK
ANCHOR = (1, 2)
WIDE = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (123, 0, 65535), (5, 3, 299), (M, M, M), (0x8000000000000000, 0x7FFFFFFFFFFFFFFF, 1 << 40),
        (0xDEADBEEFCAFEF00D, 0xFFFFFFFF00000001, 0xFFFFFFFF)]
F32_HI = [0, 0xFFFFFFFF]
F32_LO = [0, 1 << 30, 1 << 31, 0xFFFFFFFF]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("host_rng") / "driver"
    r = subprocess.run(["bash", os.path.join(ROOT, "tests", "host_rng", "build.sh"), str(out)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return str(out)


def run(driver, tmp_path, cmds):
    """cmds: tuples (name, int, ...).  Returns the output lines as lists of ints."""
    fin, fout = str(tmp_path / "cmds.txt"), str(tmp_path / "out.txt")
    with open(fin, "w") as f:
        for c in cmds:
            f.write(c[0] + " " + " ".join("%x" % v for v in c[1:]) + "\n")
    r = subprocess.run([driver, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    with open(fout) as f:
        return [[int(w, 16) for w in line.split()] for line in f]


def f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def model_lane(seed, stream, t):
    """State of lane t alone from the model (init_state builds lanes 0 .. nlanes-1; a wide t is rebuilt by hand)."""
    if t < 70000:
        st = R.init_state(seed, stream, t + 1)
        return int(st[t]), int(st[2 * t + 1])
    x = (seed ^ (stream * R.STREAM_MUL) ^ (t * R.GOLDEN)) & M
    sm = lambda v: tuple(int(w[0]) for w in R.splitmix64(np.array([v], dtype=np.uint64)))
    x, z = sm(x)
    x, a = sm(z ^ t)
    x, b = sm(x)
    return (a, b if (a or b) else R.GOLDEN)


# ------------------------------------------------------------------------------------------------------ the model itself
def test_model_anchor_worked_by_hand():
    """xoroshiro128+ 24 / 16 / 37 from state (1, 2): output 3; b = 3; s0 = rotl(1, 24) ^ 3 ^ (3 << 16) = 0x1030003;
    s1 = rotl(3, 37) = 0x6000000000 -- in both forms of the model."""
    assert R.next_int(1, 2) == (3, 0x1030003, 0x6000000000)
    r, a, b = R.next_(np.uint64(1), np.uint64(2))
    assert (int(r), int(a), int(b)) == (3, 0x1030003, 0x6000000000)
    # wrap-around and the rotations' high bits
    for s0, s1 in ((M, M), (1 << 63, 1 << 63), (0xDEADBEEFCAFEF00D, 0x0123456789ABCDEF)):
        r, a, b = R.next_(np.uint64(s0), np.uint64(s1))
        assert (int(r), int(a), int(b)) == R.next_int(s0, s1)
    assert R.next_int(M, M)[0] == M - 1 and R.next_int(1 << 63, 1 << 63) == (0, 1 << 23, 0)


def test_model_seeding_gives_distinct_nonzero_states():
    """hb_rng_init: no two of the 65536 lanes x stream ids 0..3 share (s0, s1) and none is the all-zero fixed point."""
    for seed in (0, 123):
        st = [R.init_state(seed, s, 65536) for s in range(4)]
        s0 = np.concatenate([a[:65536] for a in st])
        s1 = np.concatenate([a[65536:] for a in st])
        assert not np.any((s0 == 0) & (s1 == 0))
        pairs = np.stack([s0, s1], axis=1)
        assert np.unique(pairs, axis=0).shape[0] == 4 * 65536
        # neither word alone collides either (a 64-bit birthday collision among 2^18 values has probability 2^-29)
        assert np.unique(s0).size == s0.size and np.unique(s1).size == s1.size


def test_model_stream_layout():
    """Pair p is draw p // nlanes of lane p % nlanes; lanes without a pair keep their state; a second call continues; the
    per-site maps agree with the shared layout where they overlap."""
    nl = 7
    st = R.init_state(3, 1, nl)
    for dt, per in (("f32", 1), ("f64", 2)):
        for n in (1, 2, 3, 2 * nl - 1, 2 * nl, 2 * nl + 1, 5 * nl + 3):
            vals, new, raw = R.fill(st, nl, n, dt)
            npairs = (n + 1) // 2
            for t in range(nl):
                s0, s1 = int(st[t]), int(st[nl + t])
                cnt = len(range(t, npairs, nl))
                for k in range(cnt):
                    for q in range(per):
                        r, s0, s1 = R.next_int(s0, s1)
                        assert r == int(raw.reshape(npairs, per)[t + k * nl, q])
                assert (int(new[t]), int(new[nl + t])) == (s0, s1)
            # two calls of n1 + n2 values, n1 even and a whole number of rounds: the same values as one call
            if n > 2 * nl:
                v1, mid, _ = R.fill(st, nl, 2 * nl, dt)
                v2, end, _ = R.fill(mid, nl, n - 2 * nl, dt)
                assert np.array_equal(np.concatenate([v1, v2]), vals) and np.array_equal(end, new)
    vals, new, _ = R.sgp_in_strip(st, nl, 2 * nl)
    v2, n2, _ = R.fill(st, nl, 2 * nl, "f32")
    assert np.array_equal(vals, v2) and np.array_equal(new, n2)
    iv, new = R.gather_draw(st, nl, nl, -5, 1000)
    i2, n2 = R.randint(st, nl, nl, -5, 1000)
    assert np.array_equal(iv, i2) and np.array_equal(new, n2)
    i3, n3 = R.randint(st, nl, 3 * nl + 2, 0, 1 << 40)
    assert i3.min() >= 0 and i3.max() < (1 << 40) and np.array_equal(R.randint(n2, nl, 2 * nl + 2, 0, 1 << 40)[0], i3[nl:])
    u, new, raw = R.encoder(R.init_state(3, 1, 8), 8, 3)
    assert np.array_equal(new[6:8], R.init_state(3, 1, 8)[6:8])             # lanes >= 2 rows untouched
    z = R.normal_f32(raw[1, 1, 2])                                           # row 1, half 1, step 2 -> normals 4, 5 -> columns 12, 13
    assert u[1, 12] == z[0] and u[1, 13] == z[1]
    z = R.normal_f32(raw[2, 0, 1])                                           # row 2, half 0, step 1 -> normals 2, 3 -> columns 2, 3
    assert u[2, 2] == z[0] and u[2, 3] == z[1]


def test_model_uniform_ranges_and_extremes():
    lo, hi = np.uint64(0), np.uint64(M)
    assert R.uniform(lo) == 0.0 and R.uniform(hi) == 1.0 - 2.0 ** -53 < 1.0
    assert R.uniform_pos(lo) == 2.0 ** -53 > 0.0 and R.uniform_pos(hi) == 1.0
    for h in F32_HI:
        for l in F32_LO:
            u1, u2 = R.f32_uniforms(np.uint64((h << 32) | l))
            assert u1.dtype == np.float32 and 0.0 < u1 <= 1.0 and 0.0 <= u2 <= 1.0
            assert u1 == (np.float32(2.0 ** -32) if h == 0 else np.float32(1.0))    # 2^32 + 1 rounds to 2^32
            assert u2 == np.float32(l / 2.0 ** 32)                                      # (0xFFFFFFFF rounds to 2^32: u2 = 1)
            z0, z1 = R.normal_f32(np.uint64((h << 32) | l))
            assert np.isfinite(z0) and np.isfinite(z1) and max(abs(z0), abs(z1)) <= R.F32_MAX_ABS < 6.67
    z0, z1 = R.normal_f64(lo, lo)
    assert z1 == 0.0 and abs(z0 - np.sqrt(2 * 53 * np.log(2.0))) < 1e-14
    z0, z1 = R.normal_f64(hi, hi)
    assert z0 == 0.0 and z1 == 0.0


# ------------------------------------------------------------------------------------------------------ the host build
def test_integer_stream_of_the_host_build(driver, tmp_path):
    """HbRng::next from the anchor and from seeded states: bit-identical to the model over 64 steps."""
    starts = [ANCHOR, (M, M), (1 << 63, 1)] + [model_lane(*w) for w in WIDE]
    out = run(driver, tmp_path, [("next", s0, s1, 64) for s0, s1 in starts])
    assert out[0] == [3, 0x1030003, 0x6000000000]
    assert len(out) == 64 * len(starts)
    for i, (s0, s1) in enumerate(starts):
        for k in range(64):
            r, s0, s1 = R.next_int(s0, s1)
            assert out[64 * i + k] == [r, s0, s1], (i, k)


def test_seeding_of_the_host_build(driver, tmp_path):
    """hb_rng_seed_lane (what rng_init_kernel stores) for (seed, stream, t) including all-zero and 64-bit-wide values."""
    out = run(driver, tmp_path, [("seed",) + w for w in WIDE])
    for w, got in zip(WIDE, out):
        assert tuple(got) == model_lane(*w), w
    lanes = list(range(0, 300, 7))
    out = run(driver, tmp_path, [("seed", 123, 2, t) for t in lanes])
    st = R.init_state(123, 2, 300)
    assert [tuple(o) for o in out] == [(int(st[t]), int(st[300 + t])) for t in lanes]


def test_state_load_and_store_of_the_host_build(driver, tmp_path):
    """rng_load / rng_store: s0 of every lane, then s1 of every lane; one lane's step touches its two words only."""
    for nl, t in ((1, 0), (5, 0), (5, 3), (5, 4)):
        (out,) = run(driver, tmp_path, [("ldst", nl, t)])
        want = list(range(1, 2 * nl + 1))
        _, want[t], want[nl + t] = R.next_int(t + 1, nl + t + 1)
        assert out == want


def test_uniforms_of_the_host_build(driver, tmp_path):
    """uniform() in [0, 1) and uniform_pos() in (0, 1] at the extreme outputs x = 0 and x = 2^64 - 1 and along a stream:
    the model's bits."""
    xs = [0, M, 1 << 11, (1 << 11) - 1, M - (1 << 11)] + [R.next_int(*model_lane(9, 1, t))[0] for t in range(20)]
    cmds = []
    for x in xs:
        s0, s1 = R.state_for_output(x)
        cmds += [("uni", s0, s1), ("unipos", s0, s1)]
    out = run(driver, tmp_path, cmds)
    for i, x in enumerate(xs):
        s0, s1 = R.state_for_output(x)
        after = list(R.next_int(s0, s1)[1:])
        u, up = f64(out[2 * i][0]), f64(out[2 * i + 1][0])
        assert out[2 * i][1:] == after and out[2 * i + 1][1:] == after            # exactly one step each
        assert u == float(R.uniform(np.uint64(x))) and up == float(R.uniform_pos(np.uint64(x))), hex(x)
        assert 0.0 <= u < 1.0 and 0.0 < up <= 1.0
    assert f64(out[0][0]) == 0.0 and f64(out[3][0]) == 1.0


def test_fp32_pair_of_the_host_build(driver, tmp_path):
    """normal2(float): ONE step; the u1 handed to the log and the u2 handed to cos / sin are the model's float32 bits --
    hi in {0, 0xFFFFFFFF} x lo in {0, 2^30, 2^31, 0xFFFFFFFF}, and values whose conversion to float32 rounds (more than
    24 significant bits) both ways."""
    halves = [(h, l) for h in F32_HI for l in F32_LO]
    halves += [(0x01000001, 0x01000001), (0x01000003, 0x01000003), (0xFFFFFF7F, 0xFFFFFF80), (0xFFFFFF80, 0xFFFFFF7F), (0x00FFFFFF, 0x7FFFFFC0),
               (0x80000040, 0x800000C0), (12345, 0xC0000000)]
    halves += [(x >> 32, x & 0xFFFFFFFF) for x in (R.next_int(*model_lane(4, 0, t))[0] for t in range(40))]
    cmds = [("n32",) + R.state_for_output((h << 32) | l) for h, l in halves]
    out = run(driver, tmp_path, cmds)
    for (h, l), c, got in zip(halves, cmds, out):
        x = np.uint64((h << 32) | l)
        u1, u2 = R.f32_uniforms(x)
        assert got[0] == int(u1.view(np.uint32)) and got[1] == int(u2.view(np.uint32)), (hex(h), hex(l))
        assert got[4:] == list(R.next_int(c[1], c[2])[1:])
        z0, z1 = R.normal_f32(x)
        g0, g1 = float(f32(got[2])), float(f32(got[3]))
        assert np.isfinite(g0) and np.isfinite(g1) and max(abs(g0), abs(g1)) <= 6.67
        # the host stand-ins are libm calls rounded to float32: a few float32 ulp of the radius (<= 6.66)
        assert abs(g0 - z0) <= 4e-6 and abs(g1 - z1) <= 4e-6, (hex(h), hex(l), g0, z0, g1, z1)


def test_fp64_pair_of_the_host_build(driver, tmp_path):
    """normal2(double): TWO steps, radius from the first and angle from the second; within 8 ulp of the model (u1, u2 and
    2 u2 are exact; log, the product, sqrt, sin / cos and the final product round once each: under 5 ulp in all), at
    x >> 11 in {0, 2^53 - 1} and along a stream."""
    # the radius' output at its extremes (and just inside), then the angle's: zero, all ones, the quarter turns and their
    # neighbours, where sin or cos pass through zero
    starts = [R.state_for_output(xa, s1=s) for xa in (0, M, 1 << 11, M - (1 << 11), 12345 << 11) for s in (1, 0xFEDCBA9876543210)]
    starts += [R.state_for_second_output(xb) for xb in (0, M, 1 << 62, 1 << 63, 3 << 62, (1 << 63) + (1 << 11), (1 << 62) - (1 << 11),
                                                        (3 << 62) + (1 << 11), (1 << 63) - (1 << 11), 1 << 11)]
    starts += [model_lane(11, 2, t) for t in range(60)]
    out = run(driver, tmp_path, [("n64", s0, s1) for s0, s1 in starts])
    eps = 2.0 ** -52
    for (s0, s1), got in zip(starts, out):
        xa, a0, a1 = R.next_int(s0, s1)
        xb, b0, b1 = R.next_int(a0, a1)
        assert got[2:] == [b0, b1]
        z0, z1 = R.normal_f64(np.uint64(xa), np.uint64(xb))
        g0, g1 = f64(got[0]), f64(got[1])
        assert np.isfinite(g0) and np.isfinite(g1)
        assert abs(g0 - z0) <= 8 * eps * abs(z0) and abs(g1 - z1) <= 8 * eps * abs(z1), (hex(xa), hex(xb), g0, z0, g1, z1)
