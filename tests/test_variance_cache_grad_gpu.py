"""hb_gram_predict_grad and the exact GP's gradient routes on the GPU (hip_ops.gram_predict_grad, ExactPosterior.predict_grad /
acquisition(grad=True) / maximise, ExactGPR.suggest(steps=...)) against the float64 restatement
tests/variance_cache_grad_ref.py (pinned on the host by tests/test_variance_cache_grad_cpu.py against central
differences), against hb_gram_predict's own bits and against acq_ref's tail.

Bounds, per element, with A_s = sum_i |V_si|, W_sj = sum_i |V_si| K_ij, G_jk = max_i |x2_ik - x_jk| / ell_k^2 and
Wd_sjk = sum_i |V_si| K_ij |x2_ik - x_jk| / ell_k^2:
  t (tests/test_gram_matvec_gpu.py):  float64 1e-11 |scale| A_s;  float32 (11 + d + min(N, CHUNK) + 1) 2^-24 |scale| W_sj.
  u:  float64 1e-11 |scale| A_s G_jk;  float32 (16 + d + min(N, CHUNK) + 1) 2^-24 |scale| Wd_sjk.  16 + d is the 11 + d of the
      K value plus the roundings of the derivative operand as csrc/gram_predict_grad.hip forms it,
      b * ((f - x) * ie2) with ie2 = 1 / (ell * ell): the difference 1, ell * ell and the reciprocal 2, the two products 2.
  dvar:  2 sum_{s >= P} (|t| du + |u| dt + dt du), the bounds above propagated through the products, plus one rounding of
      the stored result (2^-53 / 2^-24 of |dvar|).  The double sum's own roundings, (S - P + 1) 2^-53 sum |t| |u|, are below
      1e-5 of the |u| dt term for S <= 65 and not carried.
Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from henbun_amd import _lib, hip_ops as H
from henbun_amd.models import ExactGPR

import acq_ref as AR
import variance_cache_grad_ref as VG
import variance_cache_ref as VC

pytestmark = pytest.mark.gpu

TORCH = {"float64": torch.float64, "float32": torch.float32}
NP = {"float64": np.float64, "float32": np.float32}
CHUNK = 2048
EPS_OUT = {"float64": 2.0 ** -53, "float32": 2.0 ** -24}


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def host(t):
    return t.cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------ 1. the kernel
# (n, N, P, S, d, dl): the strip edge (127, 128, 129, 130); row tiles of 16, 32 and beyond 64 right-hand sides; d = 1 .. 4 in
# registers, d = 5 (one full and one partial group of dimensions) and d = 9 (two full groups and one partial); one chunk, two
# chunks, 17 chunks in two groups; S == P
SWEEP = [
    (1, 1, 1, 1, 1, 1),
    (127, 33, 1, 17, 2, 2),
    (129, 31, 1, 33, 3, 1),
    (128, 32, 3, 35, 4, 4),
    (129, CHUNK, 1, 65, 5, 5),
    (130, CHUNK + 1, 1, 17, 5, 1),
    (33, CHUNK + 1, 1, 16, 9, 9),
    (5, 16 * CHUNK + 5, 1, 3, 2, 2),
]
SCALE = 1.7
_SWEEP = {}


def _sweep_case(case, dtype):
    """The inputs of tests/test_gram_matvec_gpu.py's _case (rounded to the dtype) on the host and on the device, the
    restatement's (t, u) and the magnitudes of the bounds: computed once, shared and left unchanged."""
    if (case, dtype) not in _SWEEP:
        n, N, P, S, d, dl = case
        rng = np.random.default_rng(n + 3 * N + 5 * S + 7 * d + dl)
        x = rng.uniform(0.0, 4.0, (n, d)).astype(NP[dtype])
        x2 = rng.uniform(0.0, 4.0, (N, d)).astype(NP[dtype])
        ell = (np.array([0.8]) if dl == 1 else 0.7 + 0.2 * np.arange(d)).astype(NP[dtype])
        V = rng.standard_normal((S, N)).astype(NP[dtype])
        arrays = (x, x2, ell, V)
        _SWEEP[(case, dtype)] = (tuple(dev(a, TORCH[dtype]) for a in arrays), _reference(dtype, x, x2, ell, V, SCALE))
    return _SWEEP[(case, dtype)]


def _reference(dtype, x, x2, ell, V, scale):
    """dict(t, u, dt, du): the restatement on the inputs as the device holds them and the bounds of the docstring."""
    N, d = x2.shape
    t, u = VG.products(x, x2, ell, V, scale=scale, chunk=CHUNK)
    A, W, G, Wd = VG.magnitudes(x, x2, ell, V)
    if dtype == "float64":
        dt = 1e-11 * abs(scale) * A * np.ones_like(W)
        du = 1e-11 * abs(scale) * A[:, :, None] * G[None]
    else:
        dt = (11 + d + min(N, CHUNK) + 1) * 2.0 ** -24 * abs(scale) * W
        du = (16 + d + min(N, CHUNK) + 1) * 2.0 ** -24 * abs(scale) * Wd
    return dict(t=t, u=u, dt=dt, du=du)


def _dvar_bound(dtype, ref, P, dvar_ref):
    t, u, dt, du = (ref[k][P:] for k in ("t", "u", "dt", "du"))
    at, adt = np.abs(t)[:, :, None], dt[:, :, None]
    return 2.0 * (at * du + np.abs(u) * adt + adt * du).sum(0) + EPS_OUT[dtype] * np.abs(dvar_ref)


def _q_bound(ref, P):
    t, dt = ref["t"][P:], ref["dt"][P:]
    return (2.0 * np.abs(t) * dt + dt * dt).sum(0)


def _check_moment_gradients(label, dtype, ref, P, prior, dmean, dvar):
    """dmean against u[:P] within du; dvar against the restatement within _dvar_bound wherever prior - q is clear of 0
    by the bound of q, exactly 0 wherever it is negative by more than that."""
    _, _, dmean_ref, dvar_ref, raw = VG.moments_grad(ref["t"], ref["u"], P, prior)
    assert np.all(np.isfinite(dmean)) and np.all(np.isfinite(dvar))
    e_m = np.abs(dmean - dmean_ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        w_m = np.where(e_m == 0.0, 0.0, e_m / ref["du"][:P])
    qb = _q_bound(ref, P)
    free, clamped = raw > qb, raw < -qb
    dv_free = -2.0 * VG.ordered_dq(ref["t"], ref["u"], P) if ref["t"].shape[0] > P else np.zeros_like(dvar)
    e_v = np.abs(dvar - dv_free)[free]
    b_v = _dvar_bound(dtype, ref, P, dv_free)[free]
    with np.errstate(invalid="ignore", divide="ignore"):
        w_v = np.where(e_v == 0.0, 0.0, e_v / b_v)
    print("%s: dmean error / bound %.3e (max |dmean| %.3e); dvar error / bound %.3e on %d columns, %d clamped (max |dvar| %.3e)"
          % (label, w_m.max(), np.abs(dmean_ref).max(), w_v.max() if w_v.size else 0.0, int(free.sum()), int(clamped.sum()),
             np.abs(dvar_ref).max()))
    assert w_m.max() <= 1.0
    assert w_v.size == 0 or w_v.max() <= 1.0
    assert np.all(dvar[clamped] == 0.0)
    return free, clamped


def test_the_chunk_is_the_one_the_shapes_straddle():
    assert H.gram_matvec_chunk() == CHUNK


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "n%d-N%d-P%d-S%d-d%d-dl%d" % c)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_gradients_against_the_restatement(dtype, case):
    """u for EVERY row of V (a call with P = S: every row is a mean row and dmean is u) within the bound of the docstring;
    then the call with the case's P: its dmean carries the bits of those rows, its dvar meets the propagated bound.  prior
    is the median of q: both sides of the clamp occur (n > 1, cache rows)."""
    n, N, P, S, d, dl = case
    (x, x2, ell, V), ref = _sweep_case(case, dtype)
    q = VG.ordered_q(ref["t"], P)
    prior = 0.3 if S == P else (float(np.median(q)) if n > 1 else 2.0 * float(q[0]) + 0.1)
    _, _, _, u_all, _, _ = H.gram_predict_grad(x, x2, ell, V, P=S, scale=SCALE, prior=prior, mean=False, var=False, dvar=False)
    mean, var, val, dmean, dvar, dval = H.gram_predict_grad(x, x2, ell, V, P=P, scale=SCALE, prior=prior)
    torch.cuda.synchronize()
    assert val is None and dval is None
    assert u_all.shape == (S, n, d) and dmean.shape == (P, n, d) and dvar.shape == (n, d) and mean.shape == (P, n) and var.shape == (n,)
    assert all(t.dtype == TORCH[dtype] for t in (u_all, mean, var, dmean, dvar))
    got = host(u_all)
    err = np.abs(got - ref["u"])
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = np.where(err == 0.0, 0.0, err / ref["du"])
    print("gram_predict_grad %s %s: u max error %.3e, largest error / bound %.3e" % (dtype, case, err.max(), worst.max()))
    assert np.all(np.isfinite(got)) and worst.max() <= 1.0
    assert torch.equal(dmean, u_all[:P])
    free, clamped = _check_moment_gradients("gram_predict_grad %s %s" % (dtype, case), dtype, ref, P, prior, host(dmean), host(dvar))
    if S == P:
        assert bool((dvar == 0).all()) and bool((var == float(NP[dtype](prior))).all())
    elif n > 1:
        assert free.any() and clamped.any()


VALUE_CASES = {"one-chunk-d2": (300, 257, 1, 21, 2, 2), "17-chunks-d2": (127, 16 * CHUNK + 5, 1, 16, 2, 2),
               "one-chunk-d5": (129, CHUNK, 1, 65, 5, 5)}


def _value_inputs(case, dtype):
    n, N, P, S, d, dl = case
    rng = np.random.default_rng(n + 3 * N + 5 * S + 7 * d + dl)
    x = rng.uniform(0.0, 4.0, (n, d)).astype(NP[dtype])
    x2 = rng.uniform(0.0, 4.0, (N, d)).astype(NP[dtype])
    ell = (np.array([0.8]) if dl == 1 else 0.7 + 0.2 * np.arange(d)).astype(NP[dtype])
    V = rng.standard_normal((S, N)).astype(NP[dtype])
    return tuple(dev(a, TORCH[dtype]) for a in (x, x2, ell, V))


@pytest.mark.parametrize("name", sorted(VALUE_CASES))
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_values_are_the_bits_of_gram_predict(dtype, name):
    """mean, var and val from hb_gram_predict_grad are torch.equal to hb_gram_predict's: one chunk and 17, d in registers
    and d = 5 through the dimension groups; prior at the median of q, so both sides of the clamp are compared."""
    x, x2, ell, V = _value_inputs(VALUE_CASES[name], dtype)
    t = host(H.gram_matvec(x, x2, ell, V[1:].contiguous(), scale=1.3))
    kw = dict(P=1, scale=1.3, prior=float(np.median((t * t).sum(0))), acq="ei", best=0.1, param=0.01, var_floor=1e-6)
    mean0, var0, val0, _, _ = H.gram_predict(x, x2, ell, V, value=True, **kw)
    mean, var, val, dmean, dvar, dval = H.gram_predict_grad(x, x2, ell, V, **kw)
    only = H.gram_predict_grad(x, x2, ell, V, dmean=False, dvar=False, dvalue=False, **kw)
    torch.cuda.synchronize()
    assert bool((var0 == 0).any()) and bool((var0 > 0).any())
    assert torch.equal(mean, mean0) and torch.equal(var, var0) and torch.equal(val, val0)
    assert torch.equal(only[0], mean0) and torch.equal(only[1], var0) and torch.equal(only[2], val0) and only[3:] == (None, None, None)
    assert all(bool(torch.isfinite(g).all()) for g in (dmean, dvar, dval))


def _acq_case(dtype, n=300, N=257, r=20, seed=3):
    """One latent function with r cache rows, N within one chunk, q < prior everywhere (tests/test_variance_cache_gpu.py):
    (x, x2, ell, V, scale, prior)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, 4.5, (n, 2)).astype(NP[dtype])
    x2 = rng.uniform(0.0, 4.0, (N, 2)).astype(NP[dtype])
    V = np.concatenate([0.1 * rng.standard_normal((1, N)), 0.01 * rng.standard_normal((r, N))]).astype(NP[dtype])
    return tuple(dev(a, TORCH[dtype]) for a in (x, x2, np.array([0.9, 1.2]), V)) + (1.3, 1.3)


def _own_moments(x, x2, ell, V, scale, prior):
    """The kernel's own double (t[0], prior - q) for one chunk, restated exactly: with scale 1 hb_gram_matvec returns the
    chunk's accumulator itself, t is that times scale in double, q the ordered sum."""
    t = scale * host(H.gram_matvec(x, x2, ell, V, scale=1.0))
    return t[0], prior - VG.ordered_q(t, 1)


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("kind", ["ei", "pi", "ucb"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_tail_chain(dtype, kind, largest):
    """dval against sgn a_mu dmean + a_v dvar with a_mu, a_v from acq_ref's tail at the kernel's own moments and dmean, dvar
    read back from a call without an acquisition (in float32 each is the double rounded once: 2^-23 for the two).  Bound:
    (1e-12 + [float32: 2^-23]) (|a_mu dmean| + |a_v dvar|) + [float32: 2^-24] |dval|.  Nothing is clamped (asserted)."""
    x, x2, ell, V, scale, prior = _acq_case(dtype)
    m_d, v_d = _own_moments(x, x2, ell, V, scale, prior)
    best = float(np.quantile(m_d, 0.7 if largest else 0.3))
    a = dict(best=best, param=1.5 if kind == "ucb" else 0.01, var_floor=1e-6)
    _, _, _, dmean, dvar, _ = H.gram_predict_grad(x, x2, ell, V, P=1, scale=scale, prior=prior, mean=False, var=False)
    _, _, val, _, _, dval = H.gram_predict_grad(x, x2, ell, V, P=1, scale=scale, prior=prior, acq=kind, largest=largest, mean=False,
                                                var=False, dmean=False, dvar=False, **a)
    torch.cuda.synchronize()
    _, a_mu, a_v, clamped = AR.tail(kind, m_d, v_d, a["best"], a["param"], 1.0, largest, a["var_floor"])
    assert not clamped.any() and v_d.min() > a["var_floor"]
    sgn = 1.0 if largest else -1.0
    pm, pv = (sgn * a_mu)[:, None] * host(dmean)[0], a_v[:, None] * host(dvar)
    f32 = dtype == "float32"
    bound = (1e-12 + (2.0 ** -23 if f32 else 0.0)) * (np.abs(pm) + np.abs(pv)) + (2.0 ** -24 if f32 else 0.0) * np.abs(host(dval))
    err = np.abs(host(dval) - (pm + pv))
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = np.where(err == 0.0, 0.0, err / bound)
    print("gram_predict_grad tail %s %s largest=%s: dval error / bound %.3e, max |dval| %.3e, |a_v dvar| up to %.3e of |a_mu dmean|"
          % (dtype, kind, largest, worst.max(), np.abs(host(dval)).max(), (np.abs(pv).sum(1) / np.abs(pm).sum(1)).max()))
    assert np.abs(pv).max() > 0.0 and worst.max() <= 1.0


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_clamps(dtype):
    """prior = 0 clamps every variance: var == 0 and dvar == 0 exactly, and dval is (T)(sgn a_mu u0) -- for 'ucb' (a_mu = 1)
    sgn dmean bit for bit; for every kind the bits of the call WITHOUT cache rows at prior 0, which evaluates the same
    a_mu (sigma^2 = var_floor in both) and has no variance term to add.  var_floor above every variance: dvar is not 0, yet
    dval carries no variance term -- again the bits of the call without cache rows.  S == P: dvar == 0."""
    x, x2, ell, V, scale, prior = _acq_case(dtype)
    m_d, v_d = _own_moments(x, x2, ell, V, scale, prior)
    V0 = V[:1].contiguous()
    for kind, largest in (("ei", True), ("pi", False), ("ucb", True), ("ucb", False)):
        a = dict(P=1, scale=scale, acq=kind, largest=largest, best=float(np.median(m_d)), param=1.5 if kind == "ucb" else 0.01)
        _, var, _, dmean, dvar, dval = H.gram_predict_grad(x, x2, ell, V, prior=0.0, var_floor=1e-2, **a)
        _, _, _, _, dvar0, dval0 = H.gram_predict_grad(x, x2, ell, V0, prior=0.0, var_floor=1e-2, **a)
        floor = 2.0 * float(v_d.max())
        _, varf, _, _, dvarf, dvalf = H.gram_predict_grad(x, x2, ell, V, prior=prior, var_floor=floor, **a)
        _, _, _, _, _, dvalf0 = H.gram_predict_grad(x, x2, ell, V0, prior=prior, var_floor=floor, **a)
        torch.cuda.synchronize()
        assert bool((var == 0).all()) and bool((dvar == 0).all()) and bool((dvar0 == 0).all())
        assert bool(torch.isfinite(dval).all()) and bool((dval != 0).any()) and torch.equal(dval, dval0)
        if kind == "ucb":
            assert torch.equal(dval, dmean[0] if largest else -dmean[0])
        assert bool((varf > 0).all()) and bool((dvarf != 0).any()) and float(varf.max()) < floor
        assert torch.equal(dvalf, dvalf0)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_results_are_a_function_of_the_column(dtype, monkeypatch):
    """x in ragged pieces (cuts that are no multiple of 128) carries the bits of the whole call for all six outputs, with
    one chunk and with 17; the wrapper forced to cut x into pieces of 128 columns returns the same; two calls are equal."""
    for case, cuts in (((300, 257, 1, 21, 2, 2), (0, 100, 131, 300)), ((127, 16 * CHUNK + 5, 1, 16, 2, 2), (0, 3, 126, 127))):
        n, N, P, S, d, dl = case
        x, x2, ell, V = _acq_case(dtype)[:4] if N == 257 else _value_inputs(case, dtype)
        t = host(H.gram_matvec(x, x2, ell, V[1:].contiguous(), scale=1.3))
        kw = dict(P=1, scale=1.3, prior=float(np.median((t * t).sum(0))), acq="ei", best=0.1, param=0.01, var_floor=1e-6)
        whole = H.gram_predict_grad(x, x2, ell, V, **kw)
        again = H.gram_predict_grad(x, x2, ell, V, **kw)
        pieces = [H.gram_predict_grad(x[a:b].contiguous(), x2, ell, V, **kw) for a, b in zip(cuts[:-1], cuts[1:])]
        monkeypatch.setattr(H, "GRAM_PREDICT_WS_BYTES", 1)
        assert H._gram_predict_grad_piece(n, N, d, S, TORCH[dtype]) == 128
        forced = H.gram_predict_grad(x, x2, ell, V, **kw)
        monkeypatch.undo()
        torch.cuda.synchronize()
        for k in range(6):
            assert torch.equal(whole[k], again[k]) and torch.equal(whole[k], forced[k]), k
            assert torch.equal(whole[k], torch.cat([p[k] for p in pieces], dim=1 if k in (0, 3) else 0)), k


def test_bad_arguments_never_reach_a_launch():
    """The library's own checks (raw calls with real device buffers) and the wrapper's: each raises, and the NaN-filled
    outputs keep their NaNs."""
    dt = torch.float32
    x, x2, V, ell = dev(np.ones((5, 3)), dt), dev(np.ones((4, 3)), dt), dev(np.ones((2, 4)), dt), dev(np.ones(1), dt)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=dt, device="cuda")
    mean, var, val, dmean, dvar, dval = nan(2, 5), nan(5), nan(5), nan(2, 5, 3), nan(5, 3), nan(5, 3)
    ws = torch.empty(1024, dtype=dt, device="cuda")
    p = lambda t: None if t is None else H._p(t)

    def raw(kind=H.KERN_RBF, dl=1, P=2, acq=-1, ws_=ws, val_=None, dval_=None, prior=1.0, outs=True):
        o = (mean, var, val_, dmean, dvar, dval_) if outs else (None,) * 6
        _lib.lib().call("hb_gram_predict_grad_f32", kind, p(x), p(x2), p(ell), dl, p(V), P, 1.0, prior, acq, 0.0, 0.0, 1, 0.0, p(o[0]),
                        p(o[1]), p(o[2]), p(o[3]), p(o[4]), p(o[5]), 5, 4, 3, 2, p(ws_), H.stream())

    for kw, word in ((dict(kind=H.KERN_SQDIST), "UnitRBF"), (dict(dl=2), "lengthscales"), (dict(P=0), "mean rows"),
                     (dict(P=3), "mean rows"), (dict(outs=False), "at least one"), (dict(dval_=dval), "need an acquisition"),
                     (dict(val_=val), "need an acquisition"), (dict(acq=H.ACQ["ei"], P=2, val_=val, dval_=dval), "one latent function"),
                     (dict(acq=5, P=1, dval_=dval), "unknown acquisition"), (dict(ws_=ws[1:]), "aligned"), (dict(ws_=None), "workspace"),
                     (dict(prior=float("nan")), "prior")):
        with pytest.raises(_lib.HipBackendError, match=word):
            raw(**kw)
    with pytest.raises(_lib.HipBackendError, match="UnitRBF"):
        H.gram_predict_grad(x, x2, ell, V, kind=H.KERN_SQDIST)
    with pytest.raises(ValueError, match="mean rows"):
        H.gram_predict_grad(x, x2, ell, V, P=3)
    with pytest.raises(ValueError, match="one latent function"):
        H.gram_predict_grad(x, x2, ell, V, P=2, acq="ei")
    with pytest.raises(ValueError, match="acq must be one of"):
        H.gram_predict_grad(x, x2, ell, V, P=1, acq="thompson")
    with pytest.raises(ValueError, match="need an acquisition"):
        H.gram_predict_grad(x, x2, ell, V, dvalue=True)
    with pytest.raises(ValueError, match="at least one"):
        H.gram_predict_grad(x, x2, ell, V, mean=False, var=False, dmean=False, dvar=False)
    with pytest.raises(ValueError, match="entries"):
        H.gram_predict_grad(x, x2, dev(np.ones(2), dt), V)
    with pytest.raises(ValueError, match="columns"):
        H.gram_predict_grad(x, x2, ell, dev(np.ones((2, 5)), dt))
    with pytest.raises(TypeError, match="dtype"):
        H.gram_predict_grad(x, x2.double(), ell, V)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (mean, var, val, dmean, dvar, dval))


# ------------------------------------------------------------------------------------------------ 2. the model
_FIT = {}
BOX = (np.zeros(2), 5.0 * np.ones(2))


def _case(dtype):
    """The 600-point case of variance_cache_ref (ell = 1, noise_var = 0.09) with X and Xnew as a session of `dtype` holds
    them, and a 4 x 4 candidate grid of spacing 5 / 3 > the lengthscale."""
    X, ell, k_var, noise_var, Xnew = VC.square_case(600, 5.0)
    Y = np.sin(X.sum(1, keepdims=True)) + 0.1 * np.random.default_rng(1).standard_normal((600, 1))
    g = np.linspace(0.0, 5.0, 4)
    grid = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)
    rnd = lambda a: a.astype(NP[dtype]).astype(np.float64)
    return rnd(X), Y, ell, k_var, noise_var, rnd(Xnew), rnd(grid)


def _fit(dtype):
    """ExactGPR on the case with a rank-64 cache, fitted once per dtype."""
    if dtype not in _FIT:
        X, Y, ell, k_var, noise_var, _, _ = _case(dtype)
        m = ExactGPR(X=X, Y=Y, dtype=dtype)
        m.gp.kern.lengthscales = ell.copy()
        m.k_var = np.ones(1) * k_var
        m.var = np.ones(1) * noise_var
        m.fit(cache_rank=64)
        _FIT[dtype] = m
    return _FIT[dtype]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_predict_grad_end_to_end(dtype):
    """predict_grad's mean and var_upper are the bits of predict_f(var='cache'); dmean and dvar meet the restatement on the
    posterior's own operands (X, lengthscales, V = [alpha; R_c] read back) within the sweep's bounds; acquisition(grad=True)
    returns the bits of acquisition() and the gradient hb_gram_predict_grad gives on those operands (its tail chain is
    pinned by test_tail_chain)."""
    X, Y, ell, k_var, noise_var, Xnew, _ = _case(dtype)
    post = object.__getattribute__(_fit(dtype), "posterior")
    assert post.cache_info["rank"] == 64
    mean, v, dmean, dvar = post.predict_grad(Xnew)
    m0, v0 = post.predict_f(Xnew, var="cache")
    assert np.array_equal(mean, m0) and np.array_equal(v, v0)
    assert dmean.shape == (1, 256, 2) and dvar.shape == (256, 2) and dmean.dtype == dvar.dtype == NP[dtype]
    ref = _reference(dtype, Xnew, host(post._X), host(post._ell), host(post._V), post.k_var)
    free, _ = _check_moment_gradients("predict_grad %s" % dtype, dtype, ref, 1, post.k_var, dmean.astype(np.float64),
                                      dvar.astype(np.float64))
    assert free.any()
    a = dict(best=float(m0.max()), param=0.01, var_floor=1e-6)
    val, g = post.acquisition(Xnew, "ei", grad=True, **a)
    _, _, val_k, _, _, g_k = H.gram_predict_grad(dev(Xnew, TORCH[dtype]), post._X, post._ell, post._V, scale=post.k_var, prior=post.k_var,
                                                 acq="ei", mean=False, var=False, dmean=False, dvar=False, **a)
    assert np.array_equal(val, post.acquisition(Xnew, "ei", **a)) and g.shape == (256, 2) and g.dtype == NP[dtype]
    assert np.array_equal(val, val_k.cpu().numpy()) and np.array_equal(g, g_k.cpu().numpy()) and np.all(np.isfinite(g))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_maximise_and_suggest(dtype):
    """maximise never returns less than its start, a_best is the bits of acquisition(x_best), x_best lies in the box; from a
    candidate grid coarser than a lengthscale the ascent improves 'ucb' strictly.  suggest(Xcand) is suggest(Xcand,
    steps=0) -- index, value and x_next of the arg-max -- and steps=20 returns a value at least as large."""
    X, Y, ell, k_var, noise_var, Xnew, grid = _case(dtype)
    m = _fit(dtype)
    post = object.__getattribute__(m, "posterior")
    mean_X, _ = post.predict_f(X, var=False)
    best = float(mean_X.max())
    for kind, kw in (("ei", dict(best=best, param=0.01)), ("ucb", dict(param=2.0))):
        idx, top = post.argmax(grid, kind, **kw)
        x1, a1, info = post.maximise(grid, kind, steps=20, bounds=BOX, **kw)
        xs, as_, infos = post.maximise(grid, kind, steps=20, bounds=BOX, starts=Xnew[:5].clip(0.0, 5.0), **kw)
        print("%s %s: start %d value %.6e -> %.6e at %s; five starts %s -> %s"
              % (dtype, kind, idx, float(top), float(a1[0]), x1[0], infos["start_value"], as_))
        assert set(info) == {"start_idx", "start_value", "steps"} and info["steps"] == 20 and int(info["start_idx"][0]) == idx
        assert info["start_value"][0] == top and infos["start_idx"] is None
        assert x1.shape == (1, 2) and a1.shape == (1,) and xs.shape == (5, 2) and as_.shape == (5,)
        assert x1.dtype == a1.dtype == xs.dtype == as_.dtype == NP[dtype]
        assert np.all(a1 >= info["start_value"]) and np.all(as_ >= infos["start_value"])
        assert np.array_equal(a1, post.acquisition(x1, kind, **kw)) and np.array_equal(as_, post.acquisition(xs, kind, **kw))
        for xb in (x1, xs):
            assert np.all(xb >= BOX[0]) and np.all(xb <= BOX[1])
        if kind == "ucb":
            assert a1[0] > info["start_value"][0] and np.all(as_ > infos["start_value"])
        x0, v0, i0 = m.suggest(grid, kind=kind, **{k: v for k, v in kw.items() if k != "best"})
        xz, vz, iz = m.suggest(grid, kind=kind, steps=0, **{k: v for k, v in kw.items() if k != "best"})
        xg, vg, ig = m.suggest(grid, kind=kind, steps=20, bounds=BOX, **{k: v for k, v in kw.items() if k != "best"})
        assert i0["index"] == iz["index"] == idx and v0 == vz == top and np.array_equal(x0, xz)
        assert np.array_equal(x0, grid[idx].astype(NP[dtype])) and set(i0) == {"best", "index", "cache"} and i0["best"] == best
        assert vg >= v0 and ig["start_value"] == v0 and ig["steps"] == 20 and ig["index"] == idx
        assert np.array_equal(np.asarray(vg), a1[0]) and np.array_equal(xg, x1[0])
    with pytest.raises(ValueError, match="steps"):
        post.maximise(grid, "ucb", param=2.0, steps=-1)
    with pytest.raises(ValueError, match="bounds"):
        post.maximise(grid, "ucb", param=2.0, bounds=(np.zeros(3), np.ones(3)))
    with pytest.raises(ValueError, match="starts"):
        post.maximise(grid, "ucb", param=2.0, starts=np.zeros((2, 3)))
