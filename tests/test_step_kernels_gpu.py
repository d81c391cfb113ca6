"""The kernels of the optimiser step and of the amortised / full-rank posteriors against the float64 references of
tests/step_ref.py, at the smallest shapes that reach each of their paths (tests/test_step_kernels_cpu.py asserts that they
still do): the fused encoder (csrc/mlp.hip: all twelve instantiations, ragged row chunks, the finish kernel's 16-partial
round with a tail, the forward's grid-stride second trip, saturated and kink-free inputs), the full-rank sampler
(csrc/variational.hip: thread / wave / one-launch forms at their limits, the packed backward entry by entry, NaN above the
diagonal of a dense S), one Adam step from a non-zero state with non-default hyper-parameters on each of its three code
paths, and the middle-axis reductions on both sides of their split thresholds.

The reference is evaluated on the inputs as the device holds them (rounded to fp32 for the fp32 kernels).  float64 kernels
are held to 1e-12 of the natural scale of each result (1e-13 for the float64 sums of hb_reduce); every fp32 bound goes
through parity.observe with the range observed on MI355X beside it."""
import numpy as np
import pytest
import torch

import step_ref as SR
from parity import observe, tile_err

pytestmark = pytest.mark.gpu
DT = {"f32": torch.float32, "f64": torch.float64}
NPDT = {"f32": np.float32, "f64": np.float64}
NAN = float("nan")


@pytest.fixture(scope="module")
def H():
    from henbun_amd import hip_ops

    assert torch.cuda.is_available()
    return hip_ops


def dev(a, dt):
    return torch.as_tensor(np.asarray(a), dtype=dt).cuda().contiguous()


def host(t):
    return t.detach().cpu().double().numpy()


def rnd(a, p):
    """`a` as the device will hold it, in float64."""
    return np.asarray(a, dtype=NPDT[p]).astype(np.float64)


def emax(got, ref, scale):
    """max |got - ref| / scale, elementwise; the comparison itself must be finite."""
    got, ref, scale = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(scale, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.all(np.isfinite(got)), "non-finite result"
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - ref) / np.maximum(scale, 1e-300)))


# ====================================================================================================== fused encoder
ENC_ALL = [(din, hid, act) for din in (32, 64) for hid in (128, 256) for act in ("sigmoid", "relu", "tanh")]


def _enc_inputs(n, din, hid, act, seed, sat=False):
    rng = np.random.RandomState(seed)
    if act == "relu":
        # dyadic: every pre-activation is a multiple of 2^-9 below 2^8 -- exact in fp32 in any summation order -- and an ODD
        # multiple, so at least 2^-9 away from the kink
        y = rng.randint(-32, 33, (n, din)) / 16.0
        w0 = rng.randint(-16, 17, (din, hid)) / 16.0
        b0 = (2 * rng.randint(-24, 24, hid) + 1) / 512.0
        w1 = 0.25 * rng.randn(hid, 2 * SR.L) / np.sqrt(hid)
    else:
        y = rng.randn(n, din)
        w0, b0 = rng.randn(din, hid) / np.sqrt(din), 0.1 * rng.randn(hid)
        w1 = rng.randn(hid, 2 * SR.L) / np.sqrt(hid)
        if sat:
            y *= 40.0 / np.abs(y @ w0 + b0).max()
    b1 = 0.1 * rng.randn(2 * SR.L)
    u = rng.randn(n, SR.L)
    xbar = rng.randn(n, SR.L) / np.sqrt(n)
    return [rnd(a, "f32") for a in (y, w0, b0, w1, b1, u, xbar)]


# fp32 bounds of the encoder's assertion sites, each at most 10x the largest error observed there on MI355X (o, x: against
# the scale of the sums behind them; kl: against max(|kl|, n L); gradients: worst 32 x 32 tile)
ENC_BOUND = {"o": 2e-6,      # observed 1.2e-7 .. 3.1e-7 over the 25 regular cases
             "x": 2e-6,      # observed 7.2e-8 .. 2.6e-7
             "kl": 2e-6,     # observed 4.7e-10 .. 2.8e-7
             "dw0": 2e-6,    # observed 9.3e-8 .. 2.5e-7
             "db0": 1e-6,    # observed 4.3e-8 .. 1.2e-7
             "dw1": 1.5e-6,  # observed 4.4e-8 .. 1.8e-7
             "db1": 9e-7}    # observed 2.0e-8 .. 9.6e-8
ENC_BOUND_SAT = {"o": 1.5e-6,    # observed 1.7e-7, 1.8e-7 (sigmoid, tanh)
                 "x": 1.5e-6,    # observed 1.2e-7, 1.6e-7
                 "kl": 5e-7,     # observed 5.4e-9, 5.9e-8
                 "dw0": 6e-6,    # observed 4.7e-7, 7.9e-7
                 "db0": 5e-6,    # observed 1.9e-7, 5.3e-7
                 "dw1": 2e-6,    # observed 8.2e-8, 2.0e-7
                 "db1": 7e-7}    # observed 5.8e-8, 7.9e-8
ENC_BOUND_HALVES = {"xbar_only/dw0": 1.9e-6, "xbar_only/db0": 2e-6, "xbar_only/dw1": 1.6e-6, "xbar_only/db1": 1.5e-6,
                    # observed 1.98e-7, 2.33e-7, 1.66e-7, 1.55e-7
                    "klbar_only/dw0": 1.2e-6, "klbar_only/db0": 8e-7, "klbar_only/dw1": 8e-7, "klbar_only/db1": 4.5e-7,
                    # observed 1.25e-7, 8.6e-8, 8.9e-8, 4.7e-8
                    "halves_add_up/dw0": 1.5e-6, "halves_add_up/db0": 8e-7, "halves_add_up/dw1": 1.2e-6, "halves_add_up/db1": 5e-7}
                    # observed 1.60e-7, 9.0e-8, 1.22e-7, 5.7e-8


def _enc_check(H, n, din, hid, act, sat=False, in_kernel=False, backward=True):
    """One forward (and backward) of the fused encoder against step_ref; returns what the callers look at further."""
    y, w0, b0, w1, b1, u, xbar = _enc_inputs(n, din, hid, act, 1000 * din + hid + n, sat)
    d32 = lambda a: dev(a, torch.float32)
    Y, W0, B0, W1, B1 = d32(y), d32(w0), d32(b0), d32(w1), d32(b1)
    ws = lambda: torch.full((H.mlp2_sample_ws_elems(n, din, hid),), NAN, dtype=torch.float32, device="cuda")
    if in_kernel:
        assert H.mlp2_sample_supported(n, din, hid, 32, 65536, False)
        x, kl, uo, o = H.mlp2_sample_fwd(Y, W0, B0, W1, B1, act, rng=H.Rng(5, stream_id=3), ws=ws())
        x2, kl2, uo2, _ = H.mlp2_sample_fwd(Y, W0, B0, W1, B1, act, rng=H.Rng(5, stream_id=3), ws=ws())
        assert torch.equal(uo, uo2) and torch.equal(x, x2) and torch.equal(kl, kl2)       # a pure function of the state
        u = host(uo)
        assert abs(u.mean()) < 5.0 / np.sqrt(u.size) and abs(u.std() - 1.0) < 5.0 / np.sqrt(u.size)
    else:
        U = d32(u)
        x, kl, uo, o = H.mlp2_sample_fwd(Y, W0, B0, W1, B1, act, u_in=U, ws=ws())
        assert torch.equal(uo, U)
    f = SR.encoder_fwd(y, w0, b0, w1, b1, act, u)
    if act == "relu":
        assert np.array_equal(f["pre"] * 512, np.round(f["pre"] * 512)) and np.abs(f["pre"]).max() < 2.0 ** 15
        assert np.abs(f["pre"]).min() >= 2.0 ** -9
    if sat:
        assert 39.0 <= np.abs(f["pre"]).max() <= 41.0 and np.mean(np.abs(f["pre"]) > 15.0) > 0.05
    tag = "step_enc%s[%d,%d,%d,%s%s]/" % ("_sat" if sat else "", n, din, hid, act, ",rng" if in_kernel else "")
    bound = ENC_BOUND_SAT if sat else ENC_BOUND
    s = f["o"][:, SR.L:]
    # x = mu + exp(s) u carries o's error: its scale is that of the sums behind mu and s
    x_scale = f["o_scale"][:, :SR.L] + np.exp(s) * np.abs(u) * (1.0 + f["o_scale"][:, SR.L:])
    observe(tag + "o", emax(host(o), f["o"], f["o_scale"]), bound["o"])
    observe(tag + "x", emax(host(x), f["x"], x_scale), bound["x"])
    observe(tag + "kl", abs(kl.item() - f["kl"]) / max(abs(f["kl"]), n * SR.L), bound["kl"])
    if not backward:
        return None
    klbar = np.array([-0.75])
    XB, KB = d32(xbar), d32(klbar)
    args = (Y, W0, B0, W1, act, o, uo, x)
    grads = H.mlp2_sample_bwd(*args, XB, KB, ws=ws())
    # the reference takes the operands the entry takes: the device's own s, u and x
    so, xo = host(o)[:, SR.L:], host(x)
    ref = SR.encoder_vjp(y, w0, b0, w1, act, so, u, xo, xbar, klbar)
    for got, want, name in zip(grads, ref, ("dw0", "db0", "dw1", "db1")):
        assert torch.isfinite(got).all(), name
        observe(tag + name, tile_err(host(got), want), bound[name])
    return dict(args=args, XB=XB, KB=KB, ws=ws, ops=(y, w0, b0, w1, act, so, u, xo, xbar, klbar), grads=grads, tag=tag)


@pytest.mark.parametrize("din,hid,act", ENC_ALL)
def test_encoder_every_instantiation_with_two_tiles_on_one_wave(H, din, hid, act):
    """n = 160: five row tiles in one chunk; wave 0 walks tiles 0 and 4 (the second requested one tile ahead), waves 1-3 one."""
    _enc_check(H, 160, din, hid, act)


@pytest.mark.parametrize("din,hid", [(32, 128), (64, 256)])
@pytest.mark.parametrize("n", [32, 96, 800, 2176, 2208])
def test_encoder_row_count_edges(H, n, din, hid):
    """n = 32 / 96: three / one idle waves.  n = 800: chunk 5 of 6 is empty.  n = 2208: 17 chunks (the finish kernel's
    16-partial round, then a one-partial tail), chunks 14-16 empty -- the tail partial is a zero one there, so n = 2176
    (17 chunks of 4 tiles, all full) is what makes the partial added by the tail count."""
    _enc_check(H, n, din, hid, "sigmoid")


def test_encoder_forward_grid_stride_second_trip(H):
    """n = 131104: 4097 tiles on the capped grid of 1024 workgroups x 4 waves: wave 0 of workgroup 0 takes a second trip (tile
    4096) on operands requested during the first."""
    assert SR.mlp2_fwd_trips(131104) == (1024, 2)
    _enc_check(H, 131104, 32, 128, "tanh", backward=False)


def test_encoder_in_kernel_noise(H):
    _enc_check(H, 800, 32, 128, "sigmoid", in_kernel=True)


@pytest.mark.parametrize("act", ["sigmoid", "tanh"])
def test_encoder_saturated_activations(H, act):
    """Pre-activations out to +-40: sigmoid / tanh and their derivatives through the output (h (1 - h), 1 - h^2: exactly 0 in
    fp32 for most units) stay finite and within the bound."""
    _enc_check(H, 160, 64, 128, act, sat=True)


def test_encoder_null_adjoints_give_each_half_of_the_gradient(H):
    c = _enc_check(H, 800, 32, 128, "tanh")
    y, w0, b0, w1, act, so, u, xo, xbar, klbar = c["ops"]
    only_x = H.mlp2_sample_bwd(*c["args"], c["XB"], None, ws=c["ws"]())
    only_kl = H.mlp2_sample_bwd(*c["args"], None, c["KB"], ws=c["ws"]())
    ref_x = SR.encoder_vjp(y, w0, b0, w1, act, so, u, xo, xbar, None)
    ref_kl = SR.encoder_vjp(y, w0, b0, w1, act, so, u, xo, None, klbar)
    for i, name in enumerate(("dw0", "db0", "dw1", "db1")):
        B = ENC_BOUND_HALVES
        observe(c["tag"] + "xbar_only/" + name, tile_err(host(only_x[i]), ref_x[i]), B["xbar_only/" + name])
        observe(c["tag"] + "klbar_only/" + name, tile_err(host(only_kl[i]), ref_kl[i]), B["klbar_only/" + name])
        # linear in (xbar, klbar), up to fp32 summation order
        observe(c["tag"] + "halves_add_up/" + name, tile_err(host(only_x[i]) + host(only_kl[i]), host(c["grads"][i])),
                B["halves_add_up/" + name])


# ================================================================================================== full-rank sampler
def _fr_inputs(rows, size, p, seed):
    rng = np.random.RandomState(seed)
    mu, u = 0.3 * rng.randn(rows, size), rng.randn(rows, size)
    S = np.tril(0.3 * rng.randn(rows, size, size) / np.sqrt(size)) + np.eye(size) * (0.5 + rng.rand(rows, size, 1))
    S[:, ::3, :] *= np.where(np.eye(size, dtype=bool)[::3], -1.0, 1.0)        # every third diagonal entry negative
    mu, u, S = rnd(mu, p), rnd(u, p), rnd(S, p)
    Sn = np.where(np.triu(np.ones((size, size), bool), 1), np.nan, S)         # dense: NaN wherever the kernel must not read
    return mu, u, S, Sn


def _one_launch(H, rows, size):
    return H._lib.lib().raw("hb_fullrank_one_launch_shape")(rows, size) == 1


FR_FWD = [(1, 1), (5, 7), (3, 64), (3, 65), (64, 128), (65, 128), (1, 1024), (1, 1025)]


@pytest.mark.parametrize("p", ["f32", "f64"])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("rows,size", FR_FWD)
def test_fullrank_forward_forms(H, p, packed, rows, size):
    """(1,1), (5,7), (3,64): thread kernel.  (3,65): the first wave-kernel / one-launch size.  (64,128): rows * size = 8192, the
    one-launch limit with many rows; (65,128): past it -- three launches, the wave grid capped at 2048 partials, a second trip
    of its stride loop.  (1,1024) / (1,1025): the one-launch size limit and the fall-back past it."""
    dt = DT[p]
    mu, u, S, Sn = _fr_inputs(rows, size, p, 7 * rows + size)
    launches = SR.fullrank_fwd_form(rows, size)[1]
    assert _one_launch(H, rows, size) == (launches == 1)
    if (rows, size) == (1, 1025):
        assert not _one_launch(H, rows, size) and _one_launch(H, 1, 1024)
    x_ref, kl_ref, x_scale, kl_scale = SR.fullrank_fwd(mu, S, u)
    Sd = dev(SR.tri_pack(S) if packed else Sn, dt)
    MU, U = dev(mu, dt), dev(u, dt)
    for three in ([0, 1] if launches == 1 else [0]):
        H.debug_set("fullrank_three_launches", three)
        try:
            assert _one_launch(H, rows, size) == (launches == 1 and not three)
            x, kl, uo = H.fullrank_sample_kl_fwd(MU, Sd, u_in=U, packed=packed)
            torch.cuda.synchronize()
        finally:
            H.debug_clear()
        assert torch.equal(uo, U)
        ex, ek = emax(host(x), x_ref, x_scale), abs(kl.item() - kl_ref) / kl_scale
        assert np.isfinite(kl.item())
        if p == "f64":
            assert ex <= 1e-12 and ek <= 1e-12, (ex, ek)
        else:
            tag = "step_fullrank_fwd[%d,%d,%s,%s]/" % (rows, size, "packed" if packed else "dense", "three" if three or launches == 3 else "one")
            observe(tag + "x", ex, 2e-6)       # observed 2.6e-8 .. 2.1e-7 over the 22 fp32 runs
            observe(tag + "kl", ek, 2.5e-7)    # observed 1.6e-10 .. 2.7e-8


@pytest.mark.parametrize("p", ["f32", "f64"])
@pytest.mark.parametrize("rows,size", [(3, 65), (1, 1024)])
def test_fullrank_one_launch_injected_noise_aliasing(H, p, rows, size):
    """u_out is u_in (nothing to copy) and u_out another buffer (workgroup 0 copies), in the one-launch form."""
    dt = DT[p]
    mu, u, S, Sn = _fr_inputs(rows, size, p, 11)
    assert _one_launch(H, rows, size)
    x_ref, kl_ref, x_scale, kl_scale = SR.fullrank_fwd(mu, S, u)
    MU, Sd = dev(mu, dt), dev(Sn, dt)
    for alias in (True, False):
        U = dev(u, dt)
        UO = U if alias else torch.full_like(U, NAN)
        x, kl = torch.full_like(U, NAN), torch.full((1,), NAN, dtype=dt, device="cuda")
        H.fullrank_sample_kl_fwd(MU, Sd, u_in=U, out=(x, kl, UO))
        torch.cuda.synchronize()
        assert torch.equal(U, dev(u, dt)) and torch.equal(UO, U)
        ex, ek = emax(host(x), x_ref, x_scale), abs(kl.item() - kl_ref) / kl_scale
        if p == "f64":
            assert ex <= 1e-12 and ek <= 1e-12, (ex, ek)
        else:
            observe("step_fullrank_alias[%d,%d,%d]/x" % (rows, size, alias), ex, 1.2e-6)    # observed 1.2e-7 .. 1.3e-7
            observe("step_fullrank_alias[%d,%d,%d]/kl" % (rows, size, alias), ek, 8.9e-8)   # observed 2.1e-9 .. 8.99e-9


FR_BWD = [(1, 1, "both"), (5, 7, "both"), (257, 4, "both"), (3, 65, "both"), (1, 1024, "both"), (2, 200, "kl"), (2, 200, "x")]


@pytest.mark.parametrize("p", ["f32", "f64"])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("rows,size,adj", FR_BWD)
def test_fullrank_backward_entry_by_entry(H, p, packed, rows, size, adj):
    """mubar and Sbar against the reference in the layout the kernel writes (the packed gradient is NOT unpacked through
    vec_to_tri: a wrong row index in both would cancel).  Dense: S holds NaN above the diagonal, Sbar must hold exact zeros
    there.  The outputs are pre-filled with NaN: every entry has to be written."""
    dt = DT[p]
    mu, u, S, Sn = _fr_inputs(rows, size, p, 13 * rows + size)
    rng = np.random.RandomState(rows + size)
    x = rnd(SR.fullrank_fwd(mu, S, u)[0], p)             # the forward's sample is an operand: any x will do
    xbar = rnd(rng.randn(rows, size), p) if adj != "kl" else None
    klbar = np.array([1.25]) if adj != "x" else None
    Sd = dev(SR.tri_pack(S) if packed else Sn, dt)
    MB, SB = torch.full((rows, size), NAN, dtype=dt, device="cuda"), torch.full_like(Sd, NAN)
    H.fullrank_sample_kl_bwd(Sd, dev(u, dt), dev(x, dt), None if xbar is None else dev(xbar, dt),
                             None if klbar is None else dev(klbar, dt), out=(MB, SB), packed=packed)
    torch.cuda.synchronize()
    src = SR.tri_pack(S) if packed else S
    mb_ref, sb_ref = SR.fullrank_vjp(src, u, x, xbar, klbar, packed=packed)
    kb = 0.0 if klbar is None else klbar[0]
    mb_scale = (0.0 if xbar is None else np.abs(xbar)) + abs(kb) * np.abs(x)
    i, j = np.tril_indices(size)
    sc = np.abs(mb_scale[:, i] * u[:, j]) + np.where(i == j, abs(kb) / np.abs(SR.tri_pack(S)), 0.0)
    sb_scale = sc if packed else SR.tri_unpack(sc, size)
    got_mb, got_sb = host(MB), host(SB)
    if not packed:
        assert np.all(got_sb[:, np.triu(np.ones((size, size), bool), 1)] == 0.0)
        sb_scale = sb_scale + (sb_scale == 0)            # above the diagonal: exact zeros, any scale
    em, es = emax(got_mb, mb_ref, mb_scale + (mb_scale == 0)), emax(got_sb, sb_ref, sb_scale + (sb_scale == 0))
    if p == "f64":
        assert em <= 1e-12 and es <= 1e-12, (em, es)
    else:
        tag = "step_fullrank_bwd[%d,%d,%s,%s]/" % (rows, size, "packed" if packed else "dense", adj)
        observe(tag + "mubar", em, 5e-7)     # observed 0 .. 5.9e-8 (one multiply-add per entry)
        observe(tag + "Sbar", es, 1e-6)      # observed 1.6e-8 .. 1.15e-7


# =============================================================================================================== Adam
HP = dict(lr=0.05, b1=0.8, b2=0.95, eps=1e-3, gscale=-0.25)


def _adam_state(n, p, seed):
    """Gradients of magnitude 1e-6 .. 1e2 (log-uniform) and random sign; m of the gradient's magnitude and either sign, v of
    its square, theta of magnitude >= 2.  Neither m' = b1 m + (1 - b1) g' (|b1 m| >= 8 |(1 - b1) g'|) nor theta' (the step is
    below 1) is a small difference of large terms, so each entry is its own natural scale."""
    rng = np.random.RandomState(seed)
    gm = 10.0 ** rng.uniform(-6, 2, n)
    g = gm * rng.choice([-1.0, 1.0], n)
    m = gm * (0.5 + np.abs(rng.randn(n))) * rng.choice([-1.0, 1.0], n)
    v = gm * gm * (0.5 + rng.rand(n))
    th = (2.0 + np.abs(rng.randn(n))) * rng.choice([-1.0, 1.0], n)
    return [rnd(a, p) for a in (th, g, m, v)]


@pytest.mark.parametrize("p", ["f32", "f64"])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 2048, 2049, 2051, 4099])
def test_adam_one_step_from_a_running_state(H, p, n, off):
    """n <= 2048: one workgroup, eight elements per thread up front, the tick inside.  Larger n from a 16-byte aligned base:
    the vector kernel with its n % 4 (fp32: 1, 3, 3) or n % 2 (fp64: 1) tail; from a base one element further: the scalar
    multi-block kernel.  eps = 1e-3 dominates sqrt(v') for the small gradients: epsilon under the root, epsilon on a
    bias-corrected root, or a gscale that is not squared into v' move theta' by O(1) of the step."""
    dt = DT[p]
    form = SR.adam_form(n, 4 if p == "f32" else 8, off * (4 if p == "f32" else 8))[0]
    assert form == ("block" if n <= 2048 else ("scalar" if off else "vec"))
    th, g, m, v = _adam_state(n, p, n + off)
    for t0 in (0, 7, 10 ** 6):
        want = SR.adam_step(th, g, m, v, t0, **HP)
        assert np.abs(want[0] - th).max() < 1.0
        for tick in (True, False):
            bufs = [torch.full((n + 4,), NAN, dtype=dt, device="cuda") for _ in range(4)]
            views = [b[off:off + n] for b in bufs]
            for w, a in zip(views, (th, g, m, v)):
                w.copy_(dev(a, dt))
            assert all((w.data_ptr() % 16 == 0) == (off == 0) for w in views)
            t = torch.full((1,), t0, dtype=torch.int64, device="cuda")
            H.adam_step(views[0], views[1], views[2], views[3], t, tick=tick, **HP)
            torch.cuda.synchronize()
            assert t.item() == t0 + (1 if tick else 0)
            assert torch.equal(views[1], dev(g, dt))                              # the gradient is read only
            for b in bufs:                                                        # nothing outside the segment is touched
                assert torch.isnan(b[:off]).all() and torch.isnan(b[off + n:]).all()
            errs = [emax(host(w), r, np.abs(r)) for w, r in zip((views[0], views[2], views[3]), want[:3])]
            if p == "f64":
                assert max(errs) <= 1e-12, errs
            else:
                tag = "step_adam[%d,%d,%d,%d]/" % (n, off, t0, tick)
                observe(tag + "theta", errs[0], 6e-7)      # observed 7.0e-10 .. 6.6e-8 over the 72 fp32 runs
                observe(tag + "m", errs[1], 1.2e-6)        # observed 3.6e-8 .. 1.26e-7
                observe(tag + "v", errs[2], 1.2e-6)        # observed 1.3e-8 .. 1.27e-7


@pytest.mark.parametrize("p", ["f32", "f64"])
def test_adam_empty_segment(H, p):
    """include/henbun_hip.h: the counter is 'incremented by the call when tick != 0' -- n = 0 is no exception (the last
    segment of a step may be empty): nothing is read or written but t.  The serial-chain form does not record an empty
    segment; it launches the same tick."""
    dt = DT[p]
    bufs = [torch.full((4,), 3.0, dtype=dt, device="cuda") for _ in range(4)]
    t = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    ptr = lambda x: H._p(x)

    def call(tick):
        H._lib.lib().call("hb_adam_step_" + p, ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]), 0, HP["lr"], HP["b1"],
                          HP["b2"], HP["eps"], HP["gscale"], ptr(t), int(tick), None, 0, None, None, H.stream())

    call(False)
    assert t.item() == 5
    call(True)
    assert t.item() == 6
    H.chain_begin()
    try:
        call(True)
        H.chain_end()
    finally:
        H.chain_discard()
    assert t.item() == 7
    assert all(torch.equal(b, torch.full_like(b, 3.0)) for b in bufs)


# ========================================================================================================= reductions
RED_SHAPES = [(1, 16384, 1), (1, 16385, 1), (63, 16385, 1), (64, 16385, 1), (3, 40000, 1),
              (1, 2048, 3), (1, 2049, 3), (1, 2049, 64), (1, 2049, 65), (2, 2049, 4000), (127, 2049, 1), (3, 5000, 70)]


@pytest.mark.parametrize("p", ["f32", "f64"])
@pytest.mark.parametrize("K1,R,K2", RED_SHAPES)
def test_reduce_on_both_sides_of_the_split_thresholds(H, p, K1, R, K2):
    """K2 == 1: the row kernel splits R for K1 < 64 and R > 16384.  K2 > 1: the column kernel splits R for fewer than 128
    blocks and R > 2048.  SUM against sum|x|; MAX bit for bit, on an all-negative input (an identity of 0 would win) and on
    an input with a whole -inf row and one +inf entry."""
    dt = DT[p]
    rng = np.random.RandomState(K1 + R + K2)
    x = rnd(rng.randn(K1, R, K2), p)
    got = host(H.reduce_mid(dev(x, dt), K1, R, K2)).reshape(K1, K2)
    err = emax(got, SR.reduce_mid(x, "sum"), np.abs(x).sum(1))
    if p == "f64":
        assert err <= 1e-13, err
    else:
        observe("step_reduce_sum[%d,%d,%d]" % (K1, R, K2), err, 2.5e-7)    # observed 3.2e-10 .. 2.6e-8 over the 12 shapes
    neg = -1.0 - np.abs(x)
    inf = x.copy()
    inf[0, :, 0] = -np.inf                    # one output whose every entry is -inf
    inf[K1 - 1, R // 2, K2 - 1] = np.inf      # (the same output when there is only one: +inf wins)
    for name, a in (("random", x), ("negative", neg), ("inf", inf)):
        a = rnd(a, p)
        got = host(H.reduce_mid(dev(a, dt), K1, R, K2, op=H.RED_MAX)).reshape(K1, K2)
        assert np.array_equal(got, SR.reduce_mid(a, "max")), name
    if K1 * K2 > 1:
        assert got[0, 0] == -np.inf and got[K1 - 1, K2 - 1] == np.inf


@pytest.mark.parametrize("p", ["f32", "f64"])
def test_reduce_empty_axis_sums_to_zero(H, p):
    out = torch.full((15,), NAN, dtype=DT[p], device="cuda")
    H.reduce_mid(torch.empty((3, 0, 5), dtype=DT[p], device="cuda"), 3, 0, 5, out=out)
    assert torch.equal(out, torch.zeros_like(out))
