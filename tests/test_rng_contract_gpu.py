"""The noise generator and EVERY kernel that draws from it against the exact host model of tests/rng_ref.py.

rng.hip states the contract -- "a draw of n values is a pure function of (state, n) whatever the launch geometry", and the
fused samplers "follow the same assignment" -- and this file checks it independently of the device: values against the
model, the generator state afterwards bit for bit (lanes that drew nothing included), and a second call that continues
the stream.  Small lane counts (64, and 300: no multiple of 256) put several pairs on one lane.

Draw sites covered (a new one must be added here):
  rng.hip            rng_init_kernel, rng_normal_kernel<float|double>, rng_randint_kernel
  variational.hip    diag_fwd_kernel -> diag_fwd_body (side_jobs.cuh; dense, rows=, defer=True side job),
                     rng_fill_kernel (three-launch full-rank sampler), fullrank_fwd_one_kernel (one launch)
  side_jobs.cuh      gather_draw_body (MultiGather.launch_draw, direct and as a side job)
  sgp.hip            sgp_rng_fill_kernel (P > 4), sgp_finish_part_kernel -> hb_sgp_finish_body (chain_bodies.cuh;
                     stand-alone and inside a serial chain), the in-strip finishing pass (alone and riding in the
                     persistent factorisation's launch)
  mlp.hip            mlp2_fwd_kernel (one lane per (row, half), four steps)

Tolerances.  States, integer streams and randint are exact.  fp32 normals run v_log_f32 / v_sin_f32 / v_cos_f32; their
largest deviation from the float64 model measured over the stand-alone fill (400001 values and the crafted extremes,
profiles/rng_contract.txt) is 5.438e-7, fp64 8.882e-16; the bounds are 8 times that: 4.35e-6 and 7.1e-15 (caps: 1e-4,
1e-12).  A variate from the
wrong lane, pair or step is off by O(1).  Fused fp32 sites are also compared with the stand-alone device fill BIT FOR BIT.
"""
import numpy as np
import pytest
import torch

import rng_ref as R

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f64": torch.float64}
MEASURED = {"f32": 5.438e-7, "f64": 8.882e-16}            # profiles/rng_contract.txt
TOL = {"f32": min(8 * MEASURED["f32"], 1e-4), "f64": min(8 * MEASURED["f64"], 1e-12)}
M64 = R.MASK
F32_HI = [0, 0xFFFFFFFF]
F32_LO = [0, 1 << 30, 1 << 31, 0xFFFFFFFF]


@pytest.fixture(scope="module")
def H():
    from henbun_amd import hip_ops

    assert torch.cuda.is_available()
    return hip_ops


def words(g):
    """The generator state as the model holds it."""
    torch.cuda.synchronize()
    return g.state.cpu().numpy().view(np.uint64).copy()


def put(g, st):
    g.state.copy_(torch.from_numpy(R.i64(st).copy()).to(g.state.device))


def fresh(H, nlanes, seed=11, stream=3):
    g, st = H.Rng(seed, stream, nlanes), R.init_state(seed, stream, nlanes)
    return g, st


def same_state(g, st, msg):
    got = words(g)
    nl = st.size // 2
    bad = np.nonzero((got[:nl] != st[:nl]) | (got[nl:] != st[nl:]))[0]
    assert bad.size == 0, "%s: %d of %d lanes differ from the model, first %s" % (msg, bad.size, nl, bad[:8].tolist())


def close(got, want, p, msg):
    got = got.detach().cpu().double().numpy().reshape(-1)
    assert got.shape == want.shape, (msg, got.shape, want.shape)
    assert np.all(np.isfinite(got)), msg
    err = np.abs(got - want)
    assert err.max() <= TOL[p], "%s: max |device - model| %.3e at %d (bound %.1e)" % (msg, err.max(), int(err.argmax()), TOL[p])


def nan_buf(shape, dt):
    return torch.full(shape, float("nan"), dtype=dt, device="cuda")


def ns_for(nl):
    return [1, 2, 3, 2 * nl - 1, 2 * nl, 2 * nl + 1, 5 * nl + 3]


# ===================================================================================================== stand-alone generator
@pytest.mark.parametrize("nlanes", [1, 64, 300, 65536])
def test_rng_init_kernel_state_equals_the_model(H, nlanes):
    for seed, stream in ((0, 0), (123, 1), (M64, M64), (0xDEADBEEFCAFEF00D, 3)):
        g = H.Rng(seed, stream, nlanes)
        same_state(g, R.init_state(seed, stream, nlanes), "init seed %x stream %x" % (seed, stream))
    g.reseed(5, 2)
    same_state(g, R.init_state(5, 2, nlanes), "reseed")


@pytest.mark.parametrize("p", ["f32", "f64"])
@pytest.mark.parametrize("nlanes", [64, 300])
def test_rng_normal_kernel_values_state_and_continuation(H, p, nlanes):
    """rng_normal_kernel: values, the state afterwards (every drawing lane advanced by its number of pairs, twice that in
    fp64, the others untouched) and a second call that continues; nothing written past n."""
    for n in ns_for(nlanes):
        g, st = fresh(H, nlanes)
        for call in range(2):
            buf = nan_buf((n + 3,), DT[p])
            g.normal(None, out=buf[:n])
            want, st, _ = R.fill(st, nlanes, n, p)
            close(buf[:n], want, p, "normal %s nlanes %d n %d call %d" % (p, nlanes, n, call))
            assert bool(torch.isnan(buf[n:]).all()), (n, "wrote past the end")
            same_state(g, st, "normal %s nlanes %d n %d call %d" % (p, nlanes, n, call))
    g, st = fresh(H, nlanes)
    assert g.normal((0,), DT[p]).numel() == 0
    same_state(g, st, "n = 0 draws nothing")


@pytest.mark.parametrize("nlanes", [64, 300])
def test_rng_randint_kernel_values_state_and_continuation(H, nlanes):
    """rng_randint_kernel: lo + mulhi64(next, hi - lo), value i from lane i % nlanes; exact integers; a range of 1, a
    negative lo and a range above 2^32."""
    for lo, hi in ((0, 1), (7, 8), (10, 20), (-5, (1 << 40) + 3), (0, (1 << 62) + 12345)):
        for n in (1, 2, 3, nlanes - 1, nlanes, nlanes + 1, 5 * nlanes + 3):
            g, st = fresh(H, nlanes, seed=n, stream=1)
            for call in range(2):
                buf = torch.full((n + 3,), -77, dtype=torch.int64, device="cuda")
                g.randint(n, lo, hi, out=buf[:n])
                want, st = R.randint(st, nlanes, n, lo, hi)
                got = buf.cpu().numpy()
                assert np.array_equal(got[:n], want) and np.all(got[n:] == -77), (lo, hi, n, call)
                assert got[:n].min() >= lo and got[:n].max() < hi
                same_state(g, st, "randint [%d,%d) nlanes %d n %d call %d" % (lo, hi, nlanes, n, call))
    with pytest.raises(Exception, match="empty range"):
        g.randint(4, 3, 3)


def crafted_f32_state(nlanes, st):
    """Lanes 0.. take the outputs hi x lo of the extremes (u1 in {2^-32, 1}, u2 in {0, 1/4, 1/2, 1})."""
    st = st.copy()
    xs = [(h << 32) | l for h in F32_HI for l in F32_LO]
    for t, x in enumerate(xs):
        st[t], st[nlanes + t] = R.state_for_output(x, s1=0x9E3779B97F4A7C15 * (t + 1))
    return st, xs


def crafted_f64_state(nlanes, st):
    """x >> 11 in {0, 2^53 - 1} as the radius' output (first) and as the angle's (second), and the quarter turns."""
    st = st.copy()
    firsts = [0, M64, (1 << 11) - 1, M64 - ((1 << 11) - 1)]
    seconds = [0, M64, 1 << 62, 1 << 63, 3 << 62, (1 << 63) + (1 << 11)]
    t = 0
    for x in firsts:
        st[t], st[nlanes + t] = R.state_for_output(x)
        t += 1
    for x in seconds:
        st[t], st[nlanes + t] = R.state_for_second_output(x)
        t += 1
    return st, t


def test_rng_normal_kernel_crafted_extremes(H):
    """s0 + s1 at its extremes: every result finite and the model's; fp32 stays within |z| <= 6.67."""
    nl = 64
    g, st = fresh(H, nl)
    st, xs = crafted_f32_state(nl, st)
    put(g, st)
    out = g.normal((2 * nl,), torch.float32)
    want, st2, raw = R.fill(st, nl, 2 * nl, "f32")
    assert [int(x) for x in raw[:len(xs)]] == xs
    close(out, want, "f32", "crafted f32")
    assert float(out.abs().max()) <= 6.67
    assert abs(float(out[0]) - R.F32_MAX_ABS) <= TOL["f32"] and float(out[1]) == 0.0      # hi = 0, lo = 0: the largest radius, angle 0
    assert float(out[2 * 4]) == 0.0 and float(out[2 * 4 + 1]) == 0.0                        # hi = 0xFFFFFFFF: u1 = 1, radius 0
    same_state(g, st2, "crafted f32")
    g, st = fresh(H, nl)
    st, cnt = crafted_f64_state(nl, st)
    put(g, st)
    out = g.normal((2 * nl,), torch.float64)
    want, st2, raw = R.fill(st, nl, 2 * nl, "f64")
    assert int(raw[0, 0]) == 0 and int(raw[1, 0]) == M64 and int(raw[4, 1]) == 0 and int(raw[5, 1]) == M64
    close(out, want, "f64", "crafted f64")
    assert float(out.abs().max()) <= 8.58          # sqrt(2 * 53 ln 2) = 8.5716
    same_state(g, st2, "crafted f64")


def test_measured_deviation_of_the_normals_from_the_model(H):
    """The figures the bounds rest on (profiles/rng_contract.txt): the stand-alone fill over 400001 fp32 / 100001 fp64
    values, several pairs per lane, and the crafted extremes."""
    worst = {}
    for p, n in (("f32", 400001), ("f64", 100001)):
        g, st = fresh(H, 65536, seed=2024, stream=0)
        out = g.normal((n,), DT[p])
        want, st, _ = R.fill(st, 65536, n, p)
        same_state(g, st, "measure " + p)
        worst[p] = float(np.abs(out.cpu().double().numpy() - want).max())
        g, st = fresh(H, 64)
        st = crafted_f32_state(64, st)[0] if p == "f32" else crafted_f64_state(64, st)[0]
        put(g, st)
        out = g.normal((128,), DT[p])
        worst[p + "_crafted"] = float(np.abs(out.cpu().double().numpy() - R.fill(st, 64, 128, p)[0]).max())
        print("rng contract: max |device - model| %s fill %.3e, crafted extremes %.3e (bound %.2e)"
              % (p, worst[p], worst[p + "_crafted"], TOL[p]))
    for p in ("f32", "f64"):
        assert max(worst[p], worst[p + "_crafted"]) <= TOL[p], worst


# ===================================================================================================== diagonal sampler
def _diag_layout(n):
    """(nrows, L) with nrows * L == n, L the largest divisor of n up to 50."""
    L = max(k for k in range(1, 51) if n % k == 0)
    return n // L, L


@pytest.mark.parametrize("p,form", [("f32", "dense"), ("f32", "rows"), ("f32", "defer"), ("f64", "dense"), ("f64", "rows")])
@pytest.mark.parametrize("nlanes", [64, 300, 65536])
def test_diag_fwd_body_draws_the_model_stream(H, p, form, nlanes):
    """diag_sample_kl_fwd(rng=): diag_fwd_kernel / the HB_SIDE_DIAG_FWD side job -> diag_fwd_body.  dense, the rows=
    column-block form, and defer=True (an fp32 form: a one-workgroup call is recorded as a side job, flushed here; larger
    calls launch at once).  nlanes = 65536 is the case of lanes far above n."""
    dt = DT[p]
    ns = [1, 7] if nlanes == 65536 else [1, 7, 2 * nlanes + 1, 5 * nlanes + 3]
    rs = np.random.RandomState(nlanes)
    try:
        for n in ns:
            g, st = fresh(H, nlanes, seed=n)
            g2, _ = fresh(H, nlanes, seed=n)
            nrows, L = _diag_layout(n)
            enc = torch.as_tensor(0.3 * rs.randn(nrows, 2 * L), dtype=dt).cuda()
            flat = enc.reshape(-1)
            mu_c, s_c = enc[:, :L].contiguous().reshape(-1), enc[:, L:].contiguous().reshape(-1)
            for call in range(2):
                out = (nan_buf((n,), dt), nan_buf((1,), dt), nan_buf((n,), dt))
                tag = "diag %s %s nlanes %d n %d call %d" % (p, form, nlanes, n, call)
                if form == "rows":
                    x, kl, u = H.diag_sample_kl_fwd(flat[0:], flat[L:], rng=g, out=out, rows=(nrows, L, 2 * L, 2 * L))
                else:
                    x, kl, u = H.diag_sample_kl_fwd(mu_c, s_c, rng=g, out=out, defer=(form == "defer"))
                if form == "defer":
                    H.side_flush()
                    assert H.side_pending() == 0
                want, st, _ = R.fill(st, nlanes, n, p)
                close(u, want, p, tag)
                same_state(g, st, tag)
                if p == "f32":
                    assert torch.equal(u, g2.normal((n,), dt)), tag + ": not the bits of the stand-alone fill"
                ud = u.double()
                xw = mu_c.double() + torch.exp(s_c.double()) * ud
                assert float((x.double() - xw).abs().max()) <= (1e-5 if p == "f32" else 1e-13) * max(1.0, float(xw.abs().max())), tag
                klw = -0.5 * float((2 * s_c.double() + ud * ud - xw * xw).sum())
                assert abs(float(kl) - klw) <= (1e-4 if p == "f32" else 1e-11) * max(1.0, abs(klw), float(n) ** 0.5), tag
    finally:
        H.side_discard()


def test_diag_fwd_lane_count_at_and_past_its_bound(H):
    """The launcher takes one thread per lane in at most 2048 workgroups: 524288 lanes are served, one more is refused
    (before anything is launched)."""
    nl = 2048 * 256
    mu, s = torch.zeros(7, device="cuda"), torch.zeros(7, device="cuda")
    g, st = fresh(H, nl)
    x, kl, u = H.diag_sample_kl_fwd(mu, s, rng=g)
    want, st, _ = R.fill(st, nl, 7, "f32")
    close(u, want, "f32", "diag at the lane bound")
    same_state(g, st, "diag at the lane bound")
    g, st = fresh(H, nl + 1)
    with pytest.raises(Exception, match="rng_lanes too large"):
        H.diag_sample_kl_fwd(mu, s, rng=g)
    same_state(g, st, "refused call")


# ===================================================================================================== full-rank sampler
def _fullrank_case(H, p, rows, size, packed, nlanes, three, S=None, check_x=True):
    dt = DT[p]
    rs = np.random.RandomState(rows * size)
    mu = torch.as_tensor(0.3 * rs.randn(rows, size), dtype=dt).cuda()
    if S is None:
        Sh = np.tril(0.05 * rs.randn(rows, size, size)) + np.eye(size)
        il = np.tril_indices(size)
        S = torch.as_tensor(Sh[:, il[0], il[1]] if packed else Sh, dtype=dt).cuda().contiguous()
        Sd = torch.as_tensor(Sh, dtype=torch.float64).cuda()
    n = rows * size
    H.debug_set("fullrank_three_launches", int(three))
    try:
        one = H._lib.lib().raw("hb_fullrank_one_launch_shape")(rows, size)
        g, st = fresh(H, nlanes, seed=size)
        g2, _ = fresh(H, nlanes, seed=size)
        for call in range(2):
            out = (nan_buf((rows, size), dt), nan_buf((1,), dt), nan_buf((rows, size), dt))
            tag = "fullrank %s (%d,%d) packed %d nlanes %d three %d call %d" % (p, rows, size, packed, nlanes, three, call)
            x, kl, u = H.fullrank_sample_kl_fwd(mu, S, rng=g, out=out, packed=packed)
            want, st, _ = R.fill(st, nlanes, n, p)
            close(u, want, p, tag)
            same_state(g, st, tag)
            if p == "f32":
                assert torch.equal(u.reshape(-1), g2.normal((n,), dt)), tag + ": not the bits of the stand-alone fill"
            if check_x:
                xw = mu.double() + torch.einsum("rkj,rj->rk", Sd, u.double())
                assert float((x.double() - xw).abs().max()) <= (2e-5 if p == "f32" else 1e-12) * max(1.0, float(xw.abs().max())), tag
            assert bool(torch.isfinite(kl).all()), tag
    finally:
        H.debug_clear()
    return one


@pytest.mark.parametrize("p", ["f32", "f64"])
@pytest.mark.parametrize("rows,size", [(1, 1), (3, 5), (8, 65)])
@pytest.mark.parametrize("nlanes", [64, 65536])
def test_fullrank_samplers_draw_the_model_stream(H, p, rows, size, nlanes):
    """fullrank_sample_kl_fwd(rng=): fullrank_fwd_one_kernel (one launch: every workgroup draws all of u, the last one
    stores the states) and rng_fill_kernel (three launches), dense and packed.  Blocks of up to 64 dimensions take the
    three-launch form by themselves."""
    for packed in (False, True):
        for three in (0, 1):
            one = _fullrank_case(H, p, rows, size, packed, nlanes, three)
            assert one == (1 if (size > 64 and not three) else 0), (rows, size, three, one)


def test_fullrank_one_launch_at_and_past_its_size_bound(H):
    """rows * size = 8192 values (4096 pairs: sixteen lanes per thread of the one-launch form) and one shape past it, which
    takes the three-launch form."""
    for rows, size, want_one in ((8, 1024, 1), (9, 911, 0)):
        S = torch.full((rows, size * (size + 1) // 2), 0.01, device="cuda")
        assert _fullrank_case(H, "f32", rows, size, True, 65536, 0, S=S, check_x=False) == want_one
    S = torch.full((8, 1024 * 1025 // 2), 0.01, device="cuda")
    assert _fullrank_case(H, "f32", 8, 1024, True, 300, 0, S=S, check_x=False) == 1


# ===================================================================================================== sparse GP
def _sgp_setup(H, p, E, n, M, P, frag):
    dt = DT[p]
    rs = np.random.RandomState(E * 1000 + n + M)
    lead = (E,) if E > 1 else ()
    z = torch.as_tensor(np.sort(rs.uniform(0, M / 2.0, lead + (M, 1)), axis=-2), dtype=dt).cuda()
    x = torch.as_tensor(rs.uniform(0, M / 2.0, (n, 1)), dtype=dt).cuda()
    ell = torch.ones(lead + (1,), dtype=dt, device="cuda")
    u = torch.as_tensor(rs.randn(*(lead + (P, M))), dtype=dt).cuda()
    K = torch.exp(-0.5 * (z - z.transpose(-1, -2)) ** 2) + 1e-3 * torch.eye(M, device="cuda", dtype=dt)
    fr = torch.empty(2 * E * M * M, dtype=dt, device="cuda") if frag else None
    L, W, info = H.cholesky_inverse(K.contiguous(), frag=fr)
    torch.cuda.synchronize()
    assert info.tolist() == [0] * E
    return dict(x=x, z=z, ell=ell, u=u, W=W, frag=fr, K=K.contiguous(), E=E, n=n, M=M, P=P, lead=lead, dt=dt)


def _sgp_outs(c):
    E, n, M, P, lead, dt = c["E"], c["n"], c["M"], c["P"], c["lead"], c["dt"]
    return (nan_buf(lead + (P, n), dt), nan_buf(lead + (M, n), dt), nan_buf(lead + (n,), dt), nan_buf(lead + (n,), dt))


def _sgp_check(H, p, c, nlanes, model, run, tag):
    """Two calls of `run(g, out)` drawing the residual noise; eps against `model`, states, continuation; fp32 bits against
    the stand-alone fill; f against the same call with that noise injected."""
    total = c["E"] * c["n"]
    g, st = fresh(H, nlanes, seed=total)
    g2, _ = fresh(H, nlanes, seed=total)
    for call in range(2):
        out = _sgp_outs(c)
        run(g, out)
        f, A, v, eps = out
        want, st, _ = model(st, nlanes, total)
        t = "%s call %d" % (tag, call)
        close(eps, want, p, t)
        same_state(g, st, t)
        if p == "f32":
            assert torch.equal(eps.reshape(-1), g2.normal((total,), c["dt"])), t + ": not the bits of the stand-alone fill"
        ref = H.sgp_fwd(c["x"], c["z"], c["ell"], c["W"], c["u"], eps_in=eps.clone())
        assert bool(torch.isfinite(f).all()), t
        # (another kernel form may sum in another order: fp32 rounding of W K with entries of W up to +-30; other noise: O(0.1))
        assert float((f - ref[0]).abs().max()) <= (1e-3 if p == "f32" else 1e-9) * max(1.0, float(ref[0].abs().max())), t


def _fill_model(dtype):
    return lambda st, nl, total: R.fill(st, nl, total, dtype)


@pytest.mark.parametrize("p", ["f32", "f64"])
def test_sgp_rng_fill_kernel_draws_the_model_stream(H, p):
    """sgp_fwd(rng=) with P > 4 column means: sgp_rng_fill_kernel, then the contraction and sgp_finish_kernel.  E = 2, so
    idx = e n + j crosses experts; 16 lanes, so a lane holds several pairs."""
    c = _sgp_setup(H, p, 2, 37, 32, 5, frag=False)
    assert not H.sgp_strip_path(2, 37, 32, 1, 5)
    run = lambda g, out: H.sgp_fwd(c["x"], c["z"], c["ell"], c["W"], c["u"], rng=g, out=out)
    _sgp_check(H, p, c, 16, _fill_model(p), run, "sgp fill " + p)


@pytest.mark.parametrize("p", ["f32", "f64"])
@pytest.mark.parametrize("nlanes", [16, 300])
def test_sgp_finish_part_kernel_draws_the_model_stream(H, p, nlanes):
    """sgp_fwd(rng=) in the tiled form: sgp_finish_part_kernel -> hb_sgp_finish_body, a launch of its own."""
    c = _sgp_setup(H, p, 2, 37, 30, 1, frag=False)
    assert not H.sgp_strip_path(2, 37, 30, 1, 1)
    assert H.sgp_head_units(c["x"], c["z"], c["u"], H.PREC_NATIVE, False, True, None) == 0
    run = lambda g, out: H.sgp_fwd(c["x"], c["z"], c["ell"], c["W"], c["u"], rng=g, out=out)
    _sgp_check(H, p, c, nlanes, _fill_model(p), run, "sgp finish %s nlanes %d" % (p, nlanes))


@pytest.mark.parametrize("p", ["f32", "f64"])
def test_hb_sgp_finish_body_inside_a_serial_chain_draws_the_model_stream(H, p):
    """The same finishing pass recorded as the first job of a serial chain (chain_begin / chain_end): ONE workgroup of 1024
    threads serves all lanes.  E n = 74 <= 512, the chain's admission limit; 16 lanes."""
    if not H.ewise_jit_enabled():
        pytest.skip("hiprtc is not loadable in this process")
    c = _sgp_setup(H, p, 2, 37, 30, 1, frag=False)

    def run(g, out):
        H.chain_begin()
        try:
            H.sgp_fwd(c["x"], c["z"], c["ell"], c["W"], c["u"], rng=g, out=out)
            src = H.chain_source()
            H.chain_end()
        finally:
            H.chain_discard()
        assert "hb_sgp_finish_body" in src

    _sgp_check(H, p, c, 16, _fill_model(p), run, "sgp chain " + p)


def test_sgp_in_strip_finish_draws_the_model_stream(H):
    """sgp_fwd(rng=, wfrag=) in column-strip form with one column mean (fp32 only): the finishing pass inside the strip
    kernel, lane idx >> 1, one step.  E = 2, n = 64: 64 pairs on 64 lanes is the bound (one lane per pair); with 63 lanes
    the call falls back to the stand-alone pass, where lane 0 takes two pairs -- the same stream."""
    c = _sgp_setup(H, "f32", 2, 64, 64, 1, frag=True)
    assert H.sgp_strip_path(2, 64, 64, 1, 1)
    run = lambda g, out: H.sgp_fwd(c["x"], c["z"], c["ell"], c["W"], c["u"], rng=g, out=out, wfrag=c["frag"])
    for nlanes, fused in ((64, True), (300, True), (63, False)):
        probe = H.Rng(1, 0, nlanes)
        assert (H.sgp_head_units(c["x"], c["z"], c["u"], H.PREC_NATIVE, True, True, probe) > 0) == fused, nlanes
        model = (lambda st, nl, total: R.sgp_in_strip(st, nl, total)) if fused else _fill_model("f32")
        _sgp_check(H, "f32", c, nlanes, model, run, "sgp in-strip nlanes %d" % nlanes)
    # odd n: a pair would straddle two experts -- not fused, the stand-alone pass draws the shared layout
    c = _sgp_setup(H, "f32", 2, 33, 64, 1, frag=True)
    assert H.sgp_head_units(c["x"], c["z"], c["u"], H.PREC_NATIVE, True, True, H.Rng(1, 0, 64)) == 0
    run = lambda g, out: H.sgp_fwd(c["x"], c["z"], c["ell"], c["W"], c["u"], rng=g, out=out, wfrag=c["frag"])
    _sgp_check(H, "f32", c, 16, _fill_model("f32"), run, "sgp strip, odd n")


def test_sgp_in_strip_finish_riding_in_the_factorisation_draws_the_model_stream(H):
    """The recorded forward (sgp_rider_begin) launched inside the persistent factorisation's grid: the same in-strip
    finishing pass.  32 pairs on 32 lanes is the bound; with 31 lanes the call cannot ride."""
    c = _sgp_setup(H, "f32", 1, 64, 64, 1, frag=True)
    assert H.cholesky_persistent_shape(1, 64, torch.float32)
    assert not H.sgp_rider_supported(c["x"], c["z"], c["u"], H.PREC_NATIVE, True, True, H.Rng(1, 0, 31))
    L, W = torch.empty_like(c["K"]), torch.empty_like(c["K"])
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    afrag = nan_buf((H.sgp_frag_elems(1, 64, 64, H.PREC_NATIVE),), torch.float32)

    def run(g, out):
        assert H.sgp_rider_supported(c["x"], c["z"], c["u"], H.PREC_NATIVE, True, True, g)
        H.sgp_rider_begin()
        try:
            H.sgp_fwd(c["x"], c["z"], c["ell"], W, c["u"], rng=g, out=out, wfrag=c["frag"], a_frag=afrag, skip_a=True)
            assert H.sgp_rider_pending() == 1
            H.cholesky_inverse(c["K"], out=L, inv=W, info=info, frag=c["frag"])
            assert H.sgp_rider_pending() == 0
        finally:
            H.sgp_rider_flush()
        torch.cuda.synchronize()
        assert info.tolist() == [0]

    for nlanes in (32, 300):
        _sgp_check(H, "f32", c, nlanes, lambda st, nl, total: R.sgp_in_strip(st, nl, total), run, "sgp rider nlanes %d" % nlanes)


# ===================================================================================================== encoder
def test_mlp2_fwd_kernel_draws_the_model_stream(H):
    """mlp2_sample_fwd(rng=) at its smallest shape (32 rows, 32 inputs, 256 hidden units): lane 2 row + half, four steps,
    the eight normals laid out as the kernel writes u.  64 lanes is the bound; lanes from 2 rows on stay untouched; 63
    lanes are refused."""
    n, din, hid = 32, 32, 256
    rs = np.random.RandomState(0)
    d32 = lambda a: torch.as_tensor(a, dtype=torch.float32).cuda().contiguous()
    Y, W0, B0 = d32(rs.randn(n, din)), d32(rs.randn(din, hid) / np.sqrt(din)), d32(0.1 * rs.randn(1, hid))
    W1, B1 = d32(rs.randn(hid, 32) / np.sqrt(hid)), d32(0.1 * rs.randn(1, 32))
    for nlanes in (64, 300):
        assert H.mlp2_sample_supported(n, din, hid, 32, nlanes, False)
        g, st = fresh(H, nlanes)
        g2, _ = fresh(H, nlanes)
        fill = g2.normal((8 * nlanes,), torch.float32).cpu().numpy()      # lane t: pairs t, t + nlanes, ... (four steps)
        for call in range(2):
            x, kl, u, o = H.mlp2_sample_fwd(Y, W0, B0, W1, B1, "sigmoid", rng=g)
            want, st, _ = R.encoder(st, nlanes, n)
            tag = "encoder nlanes %d call %d" % (nlanes, call)
            close(u, want.reshape(-1), "f32", tag)
            same_state(g, st, tag)
            if call == 0:
                uh = u.cpu().numpy()
                for half in range(2):
                    for k in range(8):
                        col = 4 * half + (k & 3) + 8 * (k >> 2)
                        lanes = 2 * np.arange(n) + half
                        assert np.array_equal(uh[:, col], fill[2 * (lanes + (k >> 1) * nlanes) + (k & 1)]), (tag, half, k)
            xw = o[:, :16].double() + torch.exp(o[:, 16:].double()) * u.double()
            assert float((x.double() - xw).abs().max()) <= 1e-5 * max(1.0, float(xw.abs().max())), tag
    assert not H.mlp2_sample_supported(n, din, hid, 32, 63, False)
    g, st = fresh(H, 63)
    with pytest.raises(Exception, match="unsupported shape"):
        H.mlp2_sample_fwd(Y, W0, B0, W1, B1, "sigmoid", rng=g)
    same_state(g, st, "refused call")


# ===================================================================================================== minibatch draw
@pytest.mark.parametrize("p", ["f32", "f64"])
@pytest.mark.parametrize("defer", [False, True])
def test_gather_draw_body_draws_the_model_stream(H, p, defer):
    """MultiGather.launch_draw: gather_draw_body, row r takes one step of lane r (direct launch, and recorded as a side
    job and flushed: fp32 only, fp64 launches at once).  n = nlanes is the bound; one more row is refused."""
    dt = DT[p]
    nl, N, lo, hi = 300, 500, 3, 403
    rs = np.random.RandomState(4)
    srcs = [torch.as_tensor(rs.randn(N, w), dtype=dt).cuda() for w in (1, 5, 8)]
    perm = torch.as_tensor(rs.permutation(N)).cuda()
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    try:
        for n in (1, 100, nl):
            g, st = fresh(H, nl, seed=n)
            idx = torch.full((n,), -1, dtype=torch.int64, device="cuda")
            outs = [nan_buf((n, s.shape[1]), dt) for s in srcs]
            mg = H.MultiGather(srcs, outs, idx, perm, err)
            for call in range(2):
                mg.launch_draw(g, lo, hi, defer=defer)
                H.side_flush()
                want, st = R.gather_draw(st, nl, n, lo, hi)
                tag = "gather draw %s n %d call %d" % (p, n, call)
                assert np.array_equal(idx.cpu().numpy(), want), tag
                same_state(g, st, tag)
                rows = perm.cpu().numpy()[want]
                for s, o in zip(srcs, outs):
                    assert np.array_equal(o.cpu().numpy(), s.cpu().numpy()[rows]), tag
            assert err.item() == 0
        g, st = fresh(H, nl)
        idx = torch.zeros(nl + 1, dtype=torch.int64, device="cuda")
        outs = [nan_buf((nl + 1, s.shape[1]), dt) for s in srcs]
        with pytest.raises(Exception, match="RNG lanes"):
            H.MultiGather(srcs, outs, idx, perm, err).launch_draw(g, lo, hi, defer=defer)
        same_state(g, st, "refused call")
    finally:
        H.side_discard()
