"""Input gradients of the closed-form predictive and the closed-form acquisition functions on the GPU: hb_sgp_predict_grad
and hb_sgp_acq against the numpy restatement tests/acq_ref.py (pinned on the host by tests/test_acq_cpu.py), and
SparsePosterior / SVGP.posterior / SVGP.suggest through the models.

fp64 bounds are fixed: 1e-10 of the absolute-sum scale of each derivative (acq_ref.grad_scale).  fp32 bounds are not
constants: the device's error against float64 arithmetic on the same rounded inputs is held to 4 x the error the float32
restatement makes, the margin this suite gives a different summation order; the inputs are conditioned so that this
means something (the float32 restatement itself within 1e-4 max|dmean| and 2e-3 max|dvar|).  Everything said to be the
same is compared bit for bit.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd import hip_ops as H
from henbun_amd.models import SVGP

import acq_ref as R
import sites_ref as SR

pytestmark = pytest.mark.gpu

TORCH = {"float64": torch.float64, "float32": torch.float32}
NP = {"float64": np.float64, "float32": np.float32}
MODE = {"diagonal": H.SGP_DIAGONAL, "neglected": H.SGP_NEGLECTED, "fullrank": H.SGP_FULLRANK}


def dev(a, dt):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def frag_images(W):
    """The two fragment-major images of W hb_cholesky_inverse leaves (include/henbun_hip.h), built on the host: element
    (t, Q, v, lane = (li, h), s) = W[32 t + li][32 Q + 16 h + 4 v + s], then the same of W^T."""
    M = W.shape[0]
    nT = M // 32
    i = np.arange(M * M)
    s, lane, v, blk = i & 3, (i >> 2) & 63, (i >> 8) & 3, i >> 10
    Q, tt, li, h = blk % nT, blk // nT, lane & 31, lane >> 5
    r, k = 32 * tt + li, 32 * Q + 16 * h + 4 * v + s
    return np.concatenate([np.where(k <= r, W[r, k], 0), np.where(r <= k, W[k, r], 0)]).astype(W.dtype)


# ------------------------------------------------------------------------------------------------ 1. the kernels
# (n, M, d, dl, wscale): one point; a ragged strip with an odd tile count (the middle-tile path); M = 512; d = 3 with one
# and three lengthscales; the general form (M no multiple of 32; d > 4); and 1.5 W, which puts sum A^2 above 1 (rho = -1)
SHAPES = [(1, 32, 1, 1, 1.0), (33, 96, 1, 1, 1.0), (257, 512, 1, 1, 1.0), (1000, 96, 3, 1, 1.0), (1000, 96, 3, 3, 1.0),
          (130, 40, 2, 1, 1.0), (70, 64, 5, 1, 1.0), (33, 96, 1, 1, 1.5)]
_CASE, _REF = {}, {}


def _case(shape, dtype):
    """The inputs rounded to the dtype (numpy and device), with the fragment images where M allows them: built once."""
    key = (shape, dtype)
    if key not in _CASE:
        n, M, d, dl, ws = shape
        x, z, ell, W, m, S, s, jitter = R.case(n, M, d, dl, seed=n + M + d + dl, wscale=ws)
        host = tuple(a.astype(NP[dtype]) for a in (x, z, ell, W, m, S, s))
        frag = dev(frag_images(host[3]), TORCH[dtype]) if (dtype == "float32" and M % 32 == 0) else None
        _CASE[key] = (host, tuple(dev(a, TORCH[dtype]) for a in host), frag, jitter)
    return _CASE[key]


def _ref(shape, dtype, mode, s_kind):
    """float64 arithmetic on the rounded inputs, the scales and (float32) the restatement's own error per dimension."""
    key = (shape, dtype, mode, s_kind)
    if key not in _REF:
        (x, z, ell, W, m, S, s), _, _, jitter = _case(shape, dtype)
        Sq = s if s_kind == "diag" else S
        ref = R.moments_grad(x, z, ell, W, m, Sq, mode, jitter)
        scale = R.grad_scale(x, z, ell, W, m, Sq, mode)
        rerr = None
        if dtype == "float32":
            r32 = R.moments_grad(x, z, ell, W, m, Sq, mode, jitter, dtype=np.float32)
            rerr = (np.abs(r32[2] - ref[2]).max(0), np.abs(r32[3] - ref[3]).max(0))
        _REF[key] = (ref, scale, rerr)
    return _REF[key]


def _device(shape, dtype, mode, s_kind, **kw):
    _, (x, z, ell, W, m, S, s), frag, jitter = _case(shape, dtype)
    tril = s_kind == "tril"
    return H.sgp_predict_grad(x, z, ell, W, m, S if tril else s, s_kind=H.SGP_S_TRIL if tril else H.SGP_S_DIAG, mode=MODE[mode],
                              jitter=jitter, wfrag=frag, **kw)


@pytest.mark.parametrize("s_kind", ["diag", "tril"])
@pytest.mark.parametrize("mode", ["diagonal", "neglected", "fullrank"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-M%d-d%d-dl%d-w%g" % s)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_predict_grad_against_the_restatement(dtype, shape, mode, s_kind):
    """hb_sgp_predict_grad_f64 / _f32, fused (fp32, M % 32 == 0, d <= 4) and general form.  fp64: each derivative within
    1e-10 of its absolute-sum scale.  fp32: the device's error at most 4 x the float32 restatement's, the restatement
    itself within 1e-4 max|dmean| and 2e-3 max|dvar|.  Observed on MI355X (profiles/sgp_acq.txt): fp64 dmean <= 4.1e-16,
    dvar <= 6.5e-16 of scale; fp32 device / restatement error per shape, dmean and dvar: (1, 32, 1) 0.23, 0.24 .. 0.53;
    (33, 96, 1) 0.94, 0.67 .. 1.68; (257, 512, 1) 1.46, 1.01 .. 1.86; (1000, 96, 3) 0.38 .. 0.93, 0.76 .. 1.33;
    (130, 40, 2) 0.78 .. 0.90, 0.65 .. 1.44; (70, 64, 5) 0.58 .. 1.24, 0.38 .. 1.70; 1.5 W: 0.94, 0.52 .. 2.40; the
    restatement itself at most 2.7e-5 max|dmean|, 7.1e-5 max|dvar|."""
    (mean, var, dmean, dvar), (sm, sv), rerr = _ref(shape, dtype, mode, s_kind)
    out = _device(shape, dtype, mode, s_kind)
    torch.cuda.synchronize()
    gm, gv, gdm, gdv = (t.cpu().numpy().astype(np.float64) for t in out)
    n, d = shape[0], shape[2]
    assert gm.shape == (n,) and gv.shape == (n,) and gdm.shape == (n, d) and gdv.shape == (n, d)
    em, ev = np.abs(gdm - dmean).max(0), np.abs(gdv - dvar).max(0)
    tag = "predict_grad %s %s %s %s:" % (dtype, shape, mode, s_kind)
    if dtype == "float64":
        print(tag, "dmean %.3e dvar %.3e of scale; mean %.3e var %.3e" % (
            (em / sm).max(), (ev / sv).max(), np.abs(gm - mean).max() / np.abs(mean).max(), np.abs(gv - var).max() / np.abs(var).max()))
        assert np.abs(gm - mean).max() <= 1e-10 * max(np.abs(mean).max(), 1.0) and np.abs(gv - var).max() <= 1e-10 * max(np.abs(var).max(), 1.0)
        assert np.all(em <= 1e-10 * sm) and np.all(ev <= 1e-10 * sv)
    else:
        rm, rv = rerr
        cm, cv = rm.max() / np.abs(dmean).max(), rv.max() / np.abs(dvar).max()
        print(tag, "device / restatement error dmean %s dvar %s; restatement %.2e max|dmean| %.2e max|dvar|"
              % (np.array2string(em / rm, precision=2), np.array2string(ev / rv, precision=2), cm, cv))
        assert cm <= 1e-4 and cv <= 2e-3
        assert np.all(em <= 4.0 * rm) and np.all(ev <= 4.0 * rv)


# ------------------------------------------------------------------------------------------------ 2. bitwise properties
def _model300(dtype, s_kind):
    """x [300, 2] on M = 64 (float32: the fused form) or M = 40 (float64: the general form), as device tensors."""
    M = 64 if dtype == "float32" else 40
    x, z, ell, W, m, S, s, jitter = (a if np.isscalar(a) else a.astype(NP[dtype]) for a in R.case(300, M, 2, 1, seed=5))
    frag = dev(frag_images(W), TORCH[dtype]) if dtype == "float32" else None
    tril = s_kind == "tril"
    ops = tuple(dev(a, TORCH[dtype]) for a in (z, ell, W, m, S if tril else s))
    kw = dict(s_kind=H.SGP_S_TRIL if tril else H.SGP_S_DIAG, mode=H.SGP_DIAGONAL, jitter=jitter, wfrag=frag)
    return dev(x, TORCH[dtype]), ops, kw


ACQ_KW = dict(best=0.2, param=0.01, scale=1.2, var_floor=1e-6)


@pytest.mark.parametrize("s_kind", ["diag", "tril"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_bits_do_not_depend_on_the_call(dtype, s_kind):
    """mean, var are the bits of H.sgp_predict; x [300, 2] whole, twice, and in pieces of 1, 37, 128 and 134 points gives
    the same bits of mean, var, dmean, dvar and of the acquisition's value and gradient; NULL mean / var leave
    sentinel-filled buffers untouched and change nothing else."""
    x, ops, kw = _model300(dtype, s_kind)
    z, ell, W, m, s = ops
    whole = [t.cpu().numpy() for t in H.sgp_predict_grad(x, *ops, **kw)]
    again = [t.cpu().numpy() for t in H.sgp_predict_grad(x, *ops, **kw)]
    pm, pv = H.sgp_predict(x, z, ell, W, m.reshape(1, -1), s, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(whole, again))
    assert np.array_equal(whole[0], pm.cpu().numpy().reshape(-1)) and np.array_equal(whole[1], pv.cpu().numpy().reshape(-1))
    aw = [t.cpu().numpy() for t in H.sgp_acq(x, *ops, "ei", grad=True, **ACQ_KW, **kw)[:2]]
    pieces, apieces, j0 = [], [], 0
    for c in (1, 37, 128, 134):
        xc = x[j0:j0 + c].contiguous()
        pieces.append([t.cpu().numpy() for t in H.sgp_predict_grad(xc, *ops, **kw)])
        apieces.append([t.cpu().numpy() for t in H.sgp_acq(xc, *ops, "ei", grad=True, **ACQ_KW, **kw)[:2]])
        j0 += c
    assert j0 == 300
    for i in range(4):
        assert np.array_equal(whole[i], np.concatenate([p[i] for p in pieces]))
    for i in range(2):
        assert np.array_equal(aw[i], np.concatenate([p[i] for p in apieces]))
    # NULL mean / var
    sent = [torch.full((300,), -7.0, dtype=x.dtype, device=x.device) for _ in range(2)]
    bufs = sent + [torch.empty((300, 2), dtype=x.dtype, device=x.device) for _ in range(2)]
    mean, var, dmean, dvar = H.sgp_predict_grad(x, *ops, out=bufs, values=False, **kw)
    assert mean is None and var is None
    assert all(bool((t == -7.0).all()) for t in sent)
    assert np.array_equal(dmean.cpu().numpy(), whole[2]) and np.array_equal(dvar.cpu().numpy(), whole[3])


# ------------------------------------------------------------------------------------------------ 3. the acquisition tail
@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("kind", ["ei", "pi", "ucb"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_acquisition_tail_against_the_restatement(dtype, kind, largest):
    """val and grad against the restatement's tail evaluated at the device's own (mean, var, dmean, dvar): relative 1e-12
    of the value and of every gradient entry themselves in fp64 storage; in fp32 storage the tail is double, so the
    rounding of the stored result, 2^-24 relative, comes on top.  The values span twelve decades (EI down to 2.5e-12) and
    the gradient's two terms cancel up to 865-fold; an error of one ulp in u moves EI by |u| ulp, so 1e-12 leaves room.
    A call for the values alone (which skips the gradient's phases) returns the same bits."""
    x, ops, kw = _model300(dtype, "tril")
    mean, var, dmean, dvar = (t.cpu().numpy().astype(np.float64) for t in H.sgp_predict_grad(x, *ops, **kw))
    best = float(np.quantile(1.2 * mean, 0.7 if largest else 0.3))
    a = dict(best=best, param=1.5 if kind == "ucb" else 0.01, scale=1.2, var_floor=1e-6)
    val, grad, _, _ = H.sgp_acq(x, *ops, kind, largest=largest, grad=True, **a, **kw)
    only, _, _, _ = H.sgp_acq(x, *ops, kind, largest=largest, **a, **kw)
    assert torch.equal(val, only)
    val, grad = val.cpu().numpy().astype(np.float64), grad.cpu().numpy().astype(np.float64)
    rv, a_mu, a_v, clamped = R.tail(kind, mean, var, a["best"], a["param"], a["scale"], largest, a["var_floor"])
    _, rg = R.acquisition(kind, mean, var, dmean, dvar, a["best"], a["param"], a["scale"], largest, a["var_floor"])
    bound = 1e-12 + (0.0 if dtype == "float64" else 2.0 ** -24)
    ev, eg = np.abs(val - rv) / np.abs(rv), np.abs(grad - rg) / np.abs(rg)
    print("acq tail %s %s largest=%s: val relative %.3e, grad relative %.3e (bound %.3e); clamped %d; |val| in [%.3e, %.3e], "
          "|grad| in [%.3e, %.3e]" % (dtype, kind, largest, ev.max(), eg.max(), bound, clamped.sum(), np.abs(rv).min(),
                                      np.abs(rv).max(), np.abs(rg).min(), np.abs(rg).max()))
    assert not clamped.any() and np.abs(rv).min() > 1e-30 and np.abs(rg).min() > 1e-30
    assert ev.max() <= bound
    assert eg.max() <= bound


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_expected_improvement_far_below_the_incumbent_on_the_device(dtype, largest):
    """The incumbent twelve standard deviations beyond column 7 (u = -12 there; the other columns lie between u = -13 and
    wherever their mean puts them): EI and PI are positive and finite on the device and match the restatement at the
    device's own moments, relative 1e-12 (+ 2^-24 in fp32 storage, for results that float32 holds as normal numbers), on
    every column down to u = -13 -- an fp32 u Phi(u) + phi(u) is zero or negative there."""
    x, ops, kw = _model300(dtype, "diag")
    mean, var, dmean, dvar = (t.cpu().numpy().astype(np.float64) for t in H.sgp_predict_grad(x, *ops, **kw))
    sc, s = 1.2, (1.0 if largest else -1.0)
    best = sc * mean[7] + s * 12.0 * sc * np.sqrt(var[7])
    u = (s * sc * mean - s * best) / (sc * np.sqrt(var))
    far = u >= -13.0
    bound = 1e-12 + (0.0 if dtype == "float64" else 2.0 ** -24)
    assert far[7] and abs(u[7] + 12.0) < 1e-9 and far.sum() >= 2
    for kind in ("ei", "pi"):
        val, grad, _, _ = H.sgp_acq(x, *ops, kind, best=best, param=0.0, scale=sc, largest=largest, var_floor=1e-6, grad=True, **kw)
        val, grad = val.cpu().numpy().astype(np.float64), grad.cpu().numpy().astype(np.float64)
        rv, rg = R.acquisition(kind, mean, var, dmean, dvar, best, 0.0, sc, largest, 1e-6)
        # (float32 storage: the relative rounding bound holds for normal numbers, |.| >= 2^-126; smaller entries are left out)
        tiny = 0.0 if dtype == "float64" else float(np.finfo(np.float32).tiny)
        okv, okg = far & (rv >= tiny), far[:, None] & (np.abs(rg) >= tiny)
        assert okv[7] and okv.sum() >= 2 and okg.sum() >= 2
        ev, eg = np.abs(val[okv] - rv[okv]) / rv[okv], np.abs(grad[okg] - rg[okg]) / np.abs(rg[okg])
        print("far tail %s %s largest=%s: %d columns with u in [%.2f, %.2f]; %s at u = -12: %.6e (restatement %.6e); val relative "
              "%.3e, grad relative %.3e (bound %.3e)" % (dtype, kind, largest, far.sum(), u[far].min(), u[far].max(), kind, val[7],
                                                         rv[7], ev.max(), eg.max(), bound))
        assert np.all(np.isfinite(val[far])) and np.all(val[far] > 0.0) and 0.0 < val[7] < 1e-30
        assert ev.max() <= bound and eg.max() <= bound


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_clamped_variance_passes_no_gradient(dtype):
    """A candidate equal to an inducing point, with var_floor above its variance: a_v = 0 there, so the gradient is the
    mean's term alone -- the restatement's value with the clamp, and not the one without it."""
    x, ops, kw = _model300(dtype, "diag")
    x = x.clone()
    # the inducing point whose variance is smallest, so that the floor just above it leaves other columns unclamped
    k = int(np.argmin(H.sgp_predict_grad(ops[0].contiguous(), *ops, **kw)[1].cpu().numpy()))
    x[17] = ops[0][k]
    mean, var, dmean, dvar = (t.cpu().numpy().astype(np.float64) for t in H.sgp_predict_grad(x, *ops, **kw))
    sc = 1.2
    floor = 1.001 * sc * sc * var[17]
    a = dict(best=float(np.median(sc * mean)), param=0.01, scale=sc, var_floor=floor)
    _, grad, _, _ = H.sgp_acq(x, *ops, "ei", value=False, grad=True, **a, **kw)
    grad = grad.cpu().numpy().astype(np.float64)
    _, a_mu, a_v, clamped = R.tail("ei", mean, var, a["best"], a["param"], sc, True, floor)
    _, a_mu0, a_v0, _ = R.tail("ei", mean, var, a["best"], a["param"], sc, True, 0.0)
    assert clamped[17] and a_v[17] == 0.0 and a_v0[17] > 0.0 and not clamped.all()
    want = sc * a_mu[17] * dmean[17]
    tol = (1e-12 if dtype == "float64" else 2.0 ** -23) * np.abs(want).max()
    print("clamped column %s: grad %s, the mean's term alone %s, var term without the clamp %s"
          % (dtype, grad[17], want, sc * sc * a_v0[17] * dvar[17]))
    assert np.abs(grad[17] - want).max() <= tol
    assert np.abs(sc * sc * a_v0[17] * dvar[17]).max() > 100 * tol


# ------------------------------------------------------------------------------------------------ 4. the arg-max
def _argmax_case(dtype, n):
    M = 32 if dtype == "float32" else 40
    x, z, ell, W, m, S, s, jitter = (a if np.isscalar(a) else a.astype(NP[dtype]) for a in R.case(n, M, 1, 1, seed=n))
    frag = dev(frag_images(W), TORCH[dtype]) if dtype == "float32" else None
    ops = tuple(dev(a, TORCH[dtype]) for a in (z, ell, W, m, s))
    return x, ops, dict(mode=H.SGP_DIAGONAL, jitter=jitter, wfrag=frag, best=0.0, param=0.01, scale=1.0, var_floor=1e-6)


@pytest.mark.parametrize("n", [1, 31, 33, 1000, 4099])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_argmax_is_numpys(dtype, n):
    """idx, best_val equal np.argmax of val and the value it points at, bit for bit; with every candidate duplicated the
    tie goes to the lowest row; a NaN row is never chosen; all rows NaN gives idx = -1 and best_val = -inf."""
    x, ops, kw = _argmax_case(dtype, n)
    dt = TORCH[dtype]
    for kind in ("ei", "ucb"):
        val, _, bv, bi = H.sgp_acq(dev(x, dt), *ops, kind, argmax=True, **kw)
        _, _, bv2, bi2 = H.sgp_acq(dev(x, dt), *ops, kind, value=False, argmax=True, **kw)
        val = val.cpu().numpy()
        assert bi.dtype == torch.int64 and int(bi[0]) == int(np.argmax(val)) and bv.cpu().numpy()[0] == val.max()
        assert torch.equal(bi, bi2) and torch.equal(bv, bv2)
    # duplicates: [x; x] has every value twice
    val, _, bv, bi = H.sgp_acq(dev(np.concatenate([x, x]), dt), *ops, "ei", argmax=True, **kw)
    val = val.cpu().numpy()
    assert np.array_equal(val[:n], val[n:]) and int(bi[0]) == int(np.argmax(val)) < n
    # a NaN row at the best candidate
    j = int(np.argmax(val[:n]))
    xn = x.copy()
    xn[j] = np.nan
    val, _, bv, bi = H.sgp_acq(dev(xn, dt), *ops, "ei", argmax=True, **kw)
    val = val.cpu().numpy()
    assert np.isnan(val[j])
    if n > 1:
        assert int(bi[0]) == int(np.nanargmax(val)) != j and bv.cpu().numpy()[0] == np.nanmax(val)
    _, _, bv, bi = H.sgp_acq(dev(np.full_like(x, np.nan), dt), *ops, "ei", value=False, argmax=True, **kw)
    assert int(bi[0]) == -1 and bv.cpu().numpy()[0] == -np.inf


def test_more_than_one_launch_of_the_fused_form():
    """float32, M = 32, d = 1, n = 2^20 + 37: the fused form takes its columns in two launches, whose outputs are offset and
    whose arg-max partials the second fold carries over.  idx, best_val equal np.argmax of val bit for bit with the best
    candidate in the first launch, in the second, and duplicated in both (the tie stays with the first); the values and
    gradients of the second launch's columns are the bits of a call on those columns alone."""
    n = (1 << 20) + 37
    x, ops, kw = _argmax_case("float32", 4099)
    rng = np.random.RandomState(11)
    big = rng.uniform(x.min(), x.max(), (n, 1)).astype(np.float32)
    X = dev(big, torch.float32)
    val, grad, bv, bi = H.sgp_acq(X, *ops, "ei", grad=True, argmax=True, **kw)
    _, _, bv2, bi2 = H.sgp_acq(X, *ops, "ei", value=False, argmax=True, **kw)
    v = val.cpu().numpy()
    j = int(np.argmax(v))
    print("two fused launches: arg-max %d (launch %d), value %.6e" % (j, j >> 20, v[j]))
    assert int(bi[0]) == j and bv.cpu().numpy()[0] == v[j] and torch.equal(bi, bi2) and torch.equal(bv, bv2)
    tv, tg, _, _ = H.sgp_acq(X[1 << 20:].contiguous(), *ops, "ei", grad=True, **kw)
    assert torch.equal(tv, val[1 << 20:]) and torch.equal(tg, grad[1 << 20:])
    other = (1 << 20) + 5 if j < (1 << 20) else 5          # a copy of the best candidate in the other launch
    big2 = big.copy()
    big2[other] = big[j]
    _, _, bv, bi = H.sgp_acq(dev(big2, torch.float32), *ops, "ei", value=False, argmax=True, **kw)
    assert int(bi[0]) == min(j, other) and bv.cpu().numpy()[0] == v[j]
    big3 = big.copy()                                       # the best candidate moved to the other launch
    big3[other], big3[j] = big[j], big[other]
    _, _, bv, bi = H.sgp_acq(dev(big3, torch.float32), *ops, "ei", value=False, argmax=True, **kw)
    v3 = H.sgp_acq(dev(big3, torch.float32), *ops, "ei", **kw)[0].cpu().numpy()
    assert int(bi[0]) == int(np.argmax(v3)) and bv.cpu().numpy()[0] == v3.max()


def test_more_than_one_chunk_of_the_general_form():
    """float64, M = 40, d = 2, n = 32768 + 2000 + 13: two chunks of the general form.  dmean, dvar against the
    restatement within 1e-10 of scale over all columns; the arg-max equals np.argmax of val, also with the best candidate
    copied into the other chunk; the second chunk's columns are the bits of a call on them alone."""
    n = 32768 + 2013
    x, z, ell, W, m, S, s, jitter = R.case(n, 40, 2, 1, seed=3)
    ops = tuple(dev(a, torch.float64) for a in (z, ell, W, m, S))
    kw = dict(s_kind=H.SGP_S_TRIL, mode=H.SGP_DIAGONAL, jitter=jitter)
    X = dev(x, torch.float64)
    out = H.sgp_predict_grad(X, *ops, **kw)
    ref = R.moments_grad(x, z, ell, W, m, S, "diagonal", jitter)
    sm, sv = R.grad_scale(x, z, ell, W, m, S, "diagonal")
    em, ev = np.abs(out[2].cpu().numpy() - ref[2]).max(0) / sm, np.abs(out[3].cpu().numpy() - ref[3]).max(0) / sv
    print("two general chunks: dmean %.3e dvar %.3e of scale" % (em.max(), ev.max()))
    assert em.max() <= 1e-10 and ev.max() <= 1e-10
    tail = H.sgp_predict_grad(X[32768:].contiguous(), *ops, **kw)
    assert all(torch.equal(a, b[32768:]) for a, b in zip(tail, out))
    a = dict(best=float(np.quantile(ref[0], 0.9)), param=0.01, scale=1.0, var_floor=1e-6)
    val, _, bv, bi = H.sgp_acq(X, *ops, "ei", argmax=True, **a, **kw)
    v = val.cpu().numpy()
    j = int(np.argmax(v))
    assert int(bi[0]) == j and bv.cpu().numpy()[0] == v[j]
    other = 32768 + 5 if j < 32768 else 5
    x2 = x.copy()
    x2[other], x2[j] = x[j], x[other]
    val, _, bv, bi = H.sgp_acq(dev(x2, torch.float64), *ops, "ei", argmax=True, **a, **kw)
    v = val.cpu().numpy()
    assert int(bi[0]) == int(np.argmax(v)) == other and bv.cpu().numpy()[0] == v.max()
    x2[j] = x[j]                                            # the same candidate in both chunks: the lower row
    _, _, bv, bi = H.sgp_acq(dev(x2, torch.float64), *ops, "ei", value=False, argmax=True, **a, **kw)
    assert int(bi[0]) == min(j, other)


# ------------------------------------------------------------------------------------------------ 5. through the models
_MODEL = {}
CAND = np.linspace(0.5, 15.5, 41)[:, None]


def _model(dtype, q_shape="diagonal"):
    """A fitted 1-D SVGP (N = 2000, M = 32, q from fit_q) and its posterior(), built once."""
    key = (dtype, q_shape)
    if key not in _MODEL:
        X, y, Z = SR.problem(SR.GAUSSIAN, N=2000)
        m = SVGP(X=X, Y=y, Z=Z, q_shape=q_shape, dtype=dtype)
        m.var = np.ones(1) * 0.09
        m.gp.kern.lengthscales = SR.ELL.copy()
        m.k_var = np.ones(1) * SR.K_VAR
        m.initialize()
        m.fit_q()
        _MODEL[key] = (m, m.posterior())
    return _MODEL[key]


def _snapshot(post):
    return tuple(np.array(a, np.float64) for a in (post.z, post.lengthscales, post.W, post.m, post.S))   # writable copies


@pytest.mark.parametrize("q_shape", ["diagonal", "fullrank"])
def test_posterior_predict_is_predict_f(q_shape):
    """float64: posterior().predict equals SVGP.predict_f to 1e-10; predict_grad carries the same moments and its
    gradients are autograd's of the restatement's predict on the snapshot, within 1e-8 of their scale.  Observed on
    MI355X: predict against predict_f 0 (the same bits); dmean 1.1e-16, dvar 4.3e-15 of scale."""
    m, post = _model("float64", q_shape)
    assert isinstance(post, hb.gp.SparsePosterior)
    fm, fv = m.predict_f(CAND)
    pm, pv = post.predict(CAND)
    gm, gv, dm, dv = post.predict_grad(CAND)
    print("posterior %s: predict against predict_f mean %.3e var %.3e" % (q_shape, np.abs(pm - fm[0]).max(), np.abs(pv - fv[0]).max()))
    assert pm.shape == (41,) and dm.shape == (41, 1)
    assert np.abs(pm - fm[0]).max() <= 1e-10 and np.abs(pv - fv[0]).max() <= 1e-10
    assert np.array_equal(gm, pm) and np.array_equal(gv, pv)
    z, ell, W, mm, S = _snapshot(post)
    xt = torch.tensor(CAND, dtype=torch.float64, requires_grad=True)
    tm, tv = R.predict_torch(xt, *(torch.tensor(a) for a in (z, ell, W, mm, S)), "diagonal")
    am, = torch.autograd.grad(tm.sum(), xt, retain_graph=True)
    av, = torch.autograd.grad(tv.sum(), xt)
    sm, sv = R.grad_scale(CAND, z, ell, W, mm, S, "diagonal")
    sc = np.sqrt(post.k_var)
    em, ev = np.abs(dm - sc * am.numpy()).max() / (sc * sm[0]), np.abs(dv - post.k_var * av.numpy()).max() / (post.k_var * sv[0])
    print("posterior %s: predict_grad against autograd dmean %.3e dvar %.3e of scale" % (q_shape, em, ev))
    assert em <= 1e-8 and ev <= 1e-8


def test_posterior_in_a_float32_session():
    """float32: predict is predict_f up to the scaling's rounding (the same kernel; sqrt(k_var) is applied on the host in
    double, by the plan in float32: 4 x 2^-24 relative); argmax and maximise keep their contracts."""
    m, post = _model("float32")
    fm, fv = m.predict_f(CAND)
    pm, pv = post.predict(CAND)
    em, ev = np.abs(pm - fm[0]).max() / np.abs(fm).max(), np.abs(pv - fv[0]).max() / np.abs(fv).max()
    print("posterior float32: predict against predict_f mean %.3e var %.3e relative" % (em, ev))
    assert em <= 2.0 ** -22 and ev <= 2.0 ** -22
    best = float(pm.max())
    A = post.acquisition(CAND, "ei", best=best)
    idx, val = post.argmax(CAND, "ei", best=best)
    assert A.dtype == np.float32 and idx == int(np.argmax(A)) and val == A[idx]
    xb, ab, info = post.maximise(CAND, "ei", best=best)
    assert xb.dtype == np.float32 and ab[0] >= A.max() and np.array_equal(ab, post.acquisition(xb, "ei", best=best))
    assert CAND.min() <= xb[0, 0] <= CAND.max()


@pytest.mark.parametrize("kind,largest", [("ei", True), ("ucb", True), ("pi", False)])
def test_maximise_follows_the_restatement(kind, largest):
    """float64, 41 candidates on [0.5, 15.5]: a_best >= the candidates' maximum and equals acquisition(x_best) bit for
    bit; x_best reproduces the restatement's within 1e-8, from the arg-max candidate, in a box that cuts the domain, and
    from given starts; steps=0 returns the arg-max candidate itself.  Observed on MI355X: x_best within 1.3e-13 of the
    restatement's, a_best within 9.5e-14."""
    m, post = _model("float64")
    z, ell, W, mm, S = _snapshot(post)
    pm, _ = post.predict(CAND)
    best = float(pm.max() if largest else pm.min())
    kw = dict(best=best, xi=0.01, beta=1.5, largest=largest)
    rkw = dict(mode="diagonal", jitter=post.jitter, k_var=post.k_var, best=best, param=1.5 if kind == "ucb" else 0.01,
               largest=largest, var_floor=post.k_var * post.jitter)
    A, G = post.acquisition(CAND, kind, grad=True, **kw)
    rA, rG = R.acquisition(kind, *R.moments_grad(CAND, z, ell, W, mm, S, "diagonal"), best, rkw["param"], np.sqrt(post.k_var),
                           largest, rkw["var_floor"])
    print("maximise %s: acquisition against the restatement %.3e, gradient %.3e (max|A| %.3e, max|G| %.3e)"
          % (kind, np.abs(A - rA).max(), np.abs(G - rG).max(), np.abs(rA).max(), np.abs(rG).max()))
    assert np.abs(A - rA).max() <= 1e-9 * np.abs(rA).max() and np.abs(G - rG).max() <= 1e-8 * np.abs(rG).max()
    idx, val = post.argmax(CAND, kind, **kw)
    assert idx == int(np.argmax(A)) and val == A[idx]
    x0, a0, info = post.maximise(CAND, kind, steps=0, **kw)
    assert np.array_equal(x0, CAND[idx:idx + 1]) and a0[0] == val and info["steps"] == 0 and int(info["start_idx"][0]) == idx
    starts = np.array([[3.3], [8.1], [12.7]])
    for bounds, st in ((None, None), ((np.array([4.0]), np.array([9.0])), None), (None, starts)):
        X = CAND if bounds is None else CAND[(CAND[:, 0] >= 4.0) & (CAND[:, 0] <= 9.0)]
        xb, ab, info = post.maximise(X, kind, bounds=bounds, starts=st, **kw)
        rx, ra, ridx = R.maximise(X, z, ell, W, mm, S, kind, bounds=bounds, starts=st, **rkw)
        lo, hi = (X.min(0), X.max(0)) if bounds is None else bounds
        print("maximise %s (bounds=%s, starts=%s): x_best within %.3e of the restatement's, a_best within %.3e; gain %s"
              % (kind, bounds is not None, st is not None, np.abs(xb - rx).max(), np.abs(ab - ra).max(), ab - info["start_value"]))
        assert xb.shape == rx.shape and info["steps"] == 50
        assert (st is None and int(info["start_idx"][0]) == ridx) or (st is not None and info["start_idx"] is None)
        assert np.abs(xb - rx).max() <= 1e-8
        assert np.all(ab >= info["start_value"]) and np.all(xb >= lo) and np.all(xb <= hi)
        if st is None:
            assert ab[0] >= post.acquisition(X, kind, **kw).max()
        assert np.array_equal(ab, post.acquisition(xb, kind, **kw))


def test_suggest_and_bad_arguments():
    """SVGP.suggest returns a point inside the bounds with the incumbent it used; malformed arguments raise ValueError,
    several latent functions NotImplementedError."""
    m, post = _model("float64")
    for kind, largest in (("ei", True), ("ucb", False)):
        x, a, info = m.suggest(CAND, kind=kind, largest=largest, steps=10)
        mean, _ = post.predict(object.__getattribute__(m, "X"))
        assert x.shape == (1,) and CAND.min() <= x[0] <= CAND.max() and np.isfinite(a)
        assert info["best"] == (mean.max() if largest else mean.min()) and info["steps"] == 10
    inside = CAND[(CAND[:, 0] >= 2.0) & (CAND[:, 0] <= 3.0)]
    x, a, info = m.suggest(inside, bounds=(np.array([2.0]), np.array([3.0])), steps=5)
    assert len(inside) == 3 and 2.0 <= x[0] <= 3.0
    with pytest.raises(ValueError):
        post.acquisition(CAND, "ei")                      # no incumbent
    with pytest.raises(ValueError):
        post.acquisition(CAND, "thompson", best=0.0)
    with pytest.raises(ValueError):
        post.acquisition(np.zeros((4, 2)), "ucb")         # another width
    with pytest.raises(ValueError):
        post.maximise(CAND, "ucb", steps=-1)
    with pytest.raises(ValueError):
        post.maximise(CAND, "ucb", lr=0.0)
    with pytest.raises(ValueError):
        post.maximise(CAND, "ucb", bounds=(np.array([2.0]), np.array([1.0])))
    with pytest.raises(ValueError):
        post.maximise(CAND, "ucb", starts=np.zeros((2, 3)))
    with pytest.raises(ValueError):
        post.argmax(CAND, "ei", best=0.0, var_floor=-1.0)
    q = object.__getattribute__(m, "u")
    with pytest.raises(ValueError):
        m.gp.posterior(q, k_var=0.0)
    with pytest.raises(ValueError):
        m.gp.posterior(q, residual="sideways")
    with pytest.raises(NotImplementedError):
        m.gp.posterior(q, residual="fullrank")
    M = post.z.shape[0]
    with pytest.raises(NotImplementedError, match="one latent function"):
        m.gp.posterior((np.zeros((2, M)), np.eye(M)))
    with pytest.raises(ValueError):
        m.gp.posterior((np.zeros((1, M)), np.eye(M + 1)))

    class Other(hb.model.Model):
        def setUp(self, Z, kern):
            self.gp = hb.gp.SparseGP(kern=kern, z=Z)

    Z, prior = SR.problem(SR.GAUSSIAN)[2], (np.zeros((1, M)), np.eye(M))
    with pytest.raises(NotImplementedError, match="UnitRBF"):
        Other(Z=Z, kern=hb.gp.kernels.UnitMatern52(np.ones(1)), dtype="float64").gp.posterior(prior)
    with pytest.raises(NotImplementedError, match="one expert"):
        Other(Z=np.stack([Z, Z]), kern=hb.gp.kernels.UnitRBF(np.ones((2, 1))), dtype="float64").gp.posterior(prior)
    # the C entries validate before any launch
    z, ell, W, mm, S = (dev(a, torch.float64) for a in _snapshot(post))
    x = dev(CAND, torch.float64)
    with pytest.raises(Exception):
        H._lib.lib().call("hb_sgp_acq_f64", H.KERN_CSYM_RBF, H._p(x), H._p(z), H._p(ell), 1, H._p(W), None, H._p(mm), H._p(S), H.SGP_S_DIAG,
                          H.SGP_DIAGONAL, 0.0, 0, 0.0, 0.0, 1.0, 1, 0.0, H._p(x), None, None, None, 41, M, 1, H._p(W), H.stream())
    with pytest.raises(Exception):   # no output at all
        H._lib.lib().call("hb_sgp_acq_f64", H.KERN_RBF, H._p(x), H._p(z), H._p(ell), 1, H._p(W), None, H._p(mm), H._p(S), H.SGP_S_DIAG,
                          H.SGP_DIAGONAL, 0.0, 0, 0.0, 0.0, 1.0, 1, 0.0, None, None, None, None, 41, M, 1, H._p(W), H.stream())
