"""Heteroscedastic regression on the MI355X: the hb_lik_hetgauss_* entries, SparseGP.natgrad_q and elbo_and_grad_multi
with likelihoods.HeteroscedasticGaussian, and models.SVGPHetero, against the numpy restatement tests/hetgauss_ref.py
(pinned on the host by tests/test_hetgauss_cpu.py).

Bounds.  float64 entries, those of tests/test_sites_gpu.py: lam 1e-12 relative (one exp of an argument below 750), beta and
r 1e-12 (1 + |lam mu|) absolute, sum l 1e-12 of sum |l_j|.  float32 entries: one float32 ulp of the double restatement on
the same float32 inputs (double arithmetic, one rounding), saturation included.  natgrad_q in float64: 1e-8 of the
restatement; in float32: 4 x the error of the restatement run on float32-rounded inputs.  Gradients: 4 x max(gap, 1e-10
scale), gap = the central difference's own error (its change from h to 2 h).  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd import _lib
from henbun_amd import hip_ops as H

import hetgauss_ref as R

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
MS, VS = float(np.sqrt(1.7)), 1.7
FMAX = float(np.finfo(np.float32).max)


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


@functools.lru_cache(maxsize=None)
def _site_inputs(N, c, seed=0):
    """Unit-variance marginals [2, N] of f and g with some exact v = 0 entries, and y drawn from the model at them, so that
    (y - mu_f) sqrt(e) stays of order one whatever c.  Where v_f = 0, lam_g = (y - mu_f)^2 e / 2 has the conditioning of
    the difference y - mu_f: two correct float64 evaluations that round mscale * mean differently (a fused multiply-add
    does not round it at all) differ by ulp(mu_f) / |y - mu_f| relative, 1e-11 at |y - mu_f| = 1e-4.  No relative bound
    holds there, so y is kept at least half a noise standard deviation away from mu_f at those points."""
    rs = np.random.RandomState(seed + N)
    mean = np.stack([rs.uniform(-3, 3, N), rs.uniform(-1.5, 1.5, N)])
    var = rs.uniform(0.01, 1.5, (2, N))
    var[:, ::7] = 0.0
    t = rs.randn(N)
    t[::7] = np.sign(t[::7]) * (0.5 + np.abs(t[::7]))
    y = MS * mean[0] + 1.5 * np.exp(0.5 * (MS * mean[1] + c)) * t
    return y, mean, var


def _padded(a, dt):
    """[2, N] as a view of rows padded to 16 bytes (what hb_sgp_mwstats asks of its weights)."""
    N = a.shape[1]
    q = 16 // H._elem_bytes(dt)
    buf = torch.zeros((2, -(-N // q) * q), dtype=dt, device="cuda")
    buf[:, :N] = dev(a, dt)
    return buf[:, :N]


def _ulp32(ref):
    ref32 = np.clip(ref, -FMAX, FMAX).astype(np.float32)
    below = np.nextafter(np.abs(ref32), np.float32(0.0))          # (the spacing above the largest float32 is infinite)
    return ref32, np.maximum(np.abs(ref32).astype(np.float64) - below.astype(np.float64), float(np.finfo(np.float32).tiny) * 2.0 ** -23)


@pytest.mark.parametrize("c", [0.0, -2.0, -4.0])
@pytest.mark.parametrize("N", [1, 77, 1000, 300001])
def test_sites_float64_against_the_restatement(N, c):
    """N = 300001 walks the grid-stride loop more than once (1024 blocks of 256).  Padded rows and contiguous rows hold
    the same bits; two calls return the same bits.
    Observed on MI355X: lam <= 8.1e-14, beta and r <= 5.4e-14 of their bounds' scale, sum l <= 1.6e-16."""
    y, mean, var = _site_inputs(N, c)
    yd, md, vd = dev(y, F64), _padded(mean, F64), _padded(var, F64)
    lam, beta, r, lsum = H.lik_hetgauss_sites(yd, md, vd, param=c, mscale=MS, vscale=VS, grad=True)
    rl, rb, rr, l = R.sites(y, mean, var, c, MS, VS)
    lam, beta, r = (t.cpu().numpy() for t in (lam, beta, r))
    lm = np.abs(rl * MS * mean)
    e_lam = (np.abs(lam - rl) / rl).max()
    e_beta, e_r = (np.abs(beta - rb) / (1.0 + lm)).max(), (np.abs(r - rr) / (1.0 + lm)).max()
    e_l = abs(float(lsum.cpu()[0]) - l.sum()) / np.abs(l).sum()
    print("hetgauss sites f64 N=%d c=%g: lam %.2e beta %.2e r %.2e sum l %.2e" % (N, c, e_lam, e_beta, e_r, e_l))
    assert np.all(lam >= 0.0)
    assert e_lam <= 1e-12 and e_beta <= 1e-12 and e_r <= 1e-12 and e_l <= 1e-12
    # dl/dc = dl/dmu_g, and without grad the same lam, beta, lsum
    lam2, beta2, none, lsum2 = H.lik_hetgauss_sites(yd, dev(mean, F64), dev(var, F64), param=c, mscale=MS, vscale=VS)
    assert none is None and lam2.is_contiguous()
    assert np.array_equal(lam2.cpu().numpy(), lam) and np.array_equal(beta2.cpu().numpy(), beta)
    assert float(lsum2.cpu()[0]) == float(lsum.cpu()[0])


@pytest.mark.parametrize("N", [77, 1000])
def test_sites_float32_within_one_ulp_and_saturated(N):
    """float32 storage: the double restatement on the float32 inputs, rounded once.  The last points have
    -mu_g - c + v_g / 2 > 90: e = exp(.) passes float32's range and lam, beta, r saturate at the largest finite value."""
    c = -2.0
    y, mean, var = _site_inputs(N, c)
    mean, var = mean.copy(), var.copy()
    mean[1, -5:] = -(92.0 + np.arange(5)) / MS
    y32, m32, v32 = (a.astype(np.float32) for a in (y, mean, var))
    lam, beta, r, lsum = H.lik_hetgauss_sites(dev(y32, F32), _padded(m32, F32), _padded(v32, F32), param=c, mscale=MS, vscale=VS,
                                              grad=True)
    rl, rb, rr, l = R.sites(y32.astype(np.float64), m32.astype(np.float64), v32.astype(np.float64), c, MS, VS)
    assert (-MS * m32[1, -5:].astype(np.float64) - c + 0.5 * VS * v32[1, -5:] > 90).all()
    worst = 0.0
    for name, got, ref in (("lam", lam, rl), ("beta", beta, rb), ("r", r, rr)):
        got = got.cpu().numpy()
        ref32, ulp = _ulp32(ref)
        assert np.all(np.isfinite(got)), name
        err = (np.abs(got.astype(np.float64) - ref32.astype(np.float64)) / ulp).max()
        worst = max(worst, err)
        assert err <= 1.0, (name, err)
    assert np.all(lam.cpu().numpy()[0, -5:] == np.float32(FMAX))
    e_l = abs(float(lsum.cpu()[0]) - l.sum()) / np.abs(l).sum()
    print("hetgauss sites f32 N=%d: worst %.2f ulp, sum l %.2e" % (N, worst, e_l))
    assert e_l <= 1e-12


@pytest.mark.parametrize("dt", [F64, F32])
def test_predict_and_logdens_against_the_restatement(dt):
    """hb_lik_hetgauss_predict and _logdens.  float64: 1e-12 (1 + |value|) (at most 21 exp and 21 log per point); float32:
    one ulp of the double restatement on the float32 inputs.  The sum: 1e-12 of sum |logdens_j|."""
    N, c = 1000, -2.0
    y, mean, var = _site_inputs(N, c)
    npd = np.float64 if dt == F64 else np.float32
    y, mean, var = (a.astype(npd).astype(np.float64) for a in (y, mean, var))
    ym, yv = H.lik_hetgauss_predict(_padded(mean, dt), _padded(var, dt), param=c)
    rm, rv = R.predictive(mean, var, c)
    ld, total = H.lik_hetgauss_logdens(dev(y, dt), _padded(mean, dt), _padded(var, dt), param=c, mscale=MS, vscale=VS)
    rld = R.logdens(y, mean, var, c, MS, VS)
    for name, got, ref in (("ymean", ym, rm), ("yvar", yv, rv), ("logdens", ld, rld)):
        got = got.cpu().numpy().astype(np.float64)
        if dt == F64:
            err, bound = (np.abs(got - ref) / (1.0 + np.abs(ref))).max(), 1e-12
        else:
            ref32, ulp = _ulp32(ref)
            err, bound = (np.abs(got - ref32.astype(np.float64)) / ulp).max(), 1.0
        print("hetgauss %s %s: %.3e (bound %g)" % (name, dt, err, bound))
        assert err <= bound, name
    assert abs(float(total.cpu()[0]) - rld.sum()) <= 1e-12 * np.abs(rld).sum()
    none, total2 = H.lik_hetgauss_logdens(dev(y, dt), _padded(mean, dt), _padded(var, dt), param=c, mscale=MS, vscale=VS,
                                          pointwise=False)
    assert none is None and float(total2.cpu()[0]) == float(total.cpu()[0])


def test_entry_refusals():
    """Return codes before any launch: N < 0, rows closer than N, a c that is not finite, a negative vscale, NULL
    pointers; N = 0 writes the sum 0.  The one-latent entries refuse the id.  The wrapper refuses rows of two strides."""
    N = 8
    f64 = dict(dtype=F64, device="cuda")
    y, mean, var, out = torch.zeros(N, **f64), torch.zeros((2, N), **f64), torch.ones((2, N), **f64), torch.empty((2, N), **f64)
    one = torch.full((1,), 7.0, **f64)
    ws = H.workspace(F64, y.device, 1024)
    call, p = _lib.lib().call, H._p

    def sites(n=N, ld=N, c=0.0, vs=1.0, lam=out):
        call("hb_lik_hetgauss_sites_f64", p(y), p(mean), p(var), ld, 1.0, vs, c, p(lam), p(out), None, p(one), n, p(ws), H.stream())

    for kw in (dict(n=-1), dict(ld=N - 1), dict(c=float("nan")), dict(c=float("inf")), dict(vs=-1.0), dict(lam=None)):
        with pytest.raises(_lib.HipBackendError):
            sites(**kw)
    assert float(one.cpu()[0]) == 7.0
    sites(n=0, ld=0)
    assert float(one.cpu()[0]) == 0.0
    for entry in ("lik_sites", "lik_logdens"):
        with pytest.raises(_lib.HipBackendError, match="hb_lik_hetgauss"):
            getattr(H, entry)(H.LIK_HETGAUSS, y, mean[0].contiguous(), var[0].contiguous(), param=0.0)
    with pytest.raises(_lib.HipBackendError, match="hb_lik_hetgauss"):
        H.lik_predict(H.LIK_HETGAUSS, mean[0].contiguous(), var[0].contiguous(), param=0.0)
    with pytest.raises(ValueError, match="row stride"):
        H.lik_hetgauss_sites(y, mean, torch.ones((2, N + 2), **f64)[:, :N])
    with pytest.raises(ValueError, match="row"):
        H.lik_hetgauss_sites(y, mean, var, out=(out, torch.empty((2, N + 2), **f64)[:, :N]))
    with pytest.raises(ValueError):
        H.lik_hetgauss_sites(y.float(), mean, var)


# ------------------------------------------------------------------------------------------------ natgrad_q
K_VAR, RHO, KSPLIT = 1.3, 0.5, 432          # KSPLIT: columns per float32 block of the restatement (tests/test_sites_gpu.py)


class _Holder(hb.model.Model):
    def setUp(self, Z, ell):
        self.gp = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(np.ones(1) * ell), z=Z)


def _device_W(Z, ell, dt):
    z = dev(Z, dt)
    _, W, info = H.cholesky_inverse(H.gram_fwd(z, z, dev(np.ones(1) * ell, dt), diag_add=float(hb.settings.numerics.jitter_level)))
    assert int(info.cpu()[0]) == 0
    return W.cpu().numpy()


@pytest.mark.parametrize("residual", ["diagonal", "neglected"])
def test_natgrad_q_float64_follows_the_restatement(residual, monkeypatch):
    """12 half steps from the prior in a float64 session (N = 400, M = 32, d = 1, c = -2, k_var = 1.3): the ELBO trace, the
    residual trace, m and every S S^T to 1e-8 of the restatement on the device's own W.  Every step takes its marginals
    from ONE sgp_predict_multi call and none from sgp_predict; the ELBO rises at every step.
    Observed on MI355X: elbo 5.3e-15, residual 3.9e-14, m 8.1e-13, S S^T 1.1e-13; ELBO -5678.85 -> -235.69."""
    c = -2.0
    X, Y, Z, _ = R.data(400, 32, c, 1)
    m = _Holder(Z=Z, ell=1.0, dtype="float64")
    m.initialize()
    calls = dict(multi=0, one=0)
    multi, one = H.sgp_predict_multi, H.sgp_predict
    monkeypatch.setattr(H, "sgp_predict_multi", lambda *a, **k: (calls.__setitem__("multi", calls["multi"] + 1), multi(*a, **k))[1])
    monkeypatch.setattr(H, "sgp_predict", lambda *a, **k: (calls.__setitem__("one", calls["one"] + 1), one(*a, **k))[1])
    lik = hb.likelihoods.HeteroscedasticGaussian(c)
    qm, S, info = m.gp.natgrad_q(X, Y, lik, k_var=K_VAR, residual=residual, steps=12, rho=RHO, tol=0.0)
    assert calls == dict(multi=13, one=0)
    rm, rS, rinfo = R.natgrad(X, Y[:, 0], Z, np.ones(1), K_VAR, c, residual, RHO, 12, 0.0, W=_device_W(Z, 1.0, F64))
    assert info["steps"] == 12 and len(info["elbo"]) == 13 and qm.shape == (2, 32) and S.shape == (2, 32, 32)
    assert np.array_equal(S, np.tril(S))
    e_elbo = np.abs(info["elbo"] / rinfo["elbo"] - 1).max()
    e_res = (np.abs(info["residual"] - rinfo["residual"]) / rinfo["residual"]).max()
    e_m = np.abs(qm - rm).max() / np.abs(rm).max()
    SS, rSS = S @ S.transpose(0, 2, 1), rS @ rS.transpose(0, 2, 1)
    e_S = np.abs(SS - rSS).max() / np.abs(rSS).max()
    print("natgrad_q hetgauss f64 %s: elbo %.2e residual %.2e m %.2e S S^T %.2e; elbo %.4f -> %.4f, residual %.2e"
          % (residual, e_elbo, e_res, e_m, e_S, info["elbo"][0], info["elbo"][-1], info["residual"][-1]))
    assert e_elbo <= 1e-8 and e_res <= 1e-8 and e_m <= 1e-8 and e_S <= 1e-8
    assert np.diff(info["elbo"]).min() >= -1e-9 * np.abs(info["elbo"]).max()
    # a start from a given q continues the same trace
    r20 = R.natgrad(X, Y[:, 0], Z, np.ones(1), K_VAR, c, residual, RHO, 20, 0.0, W=_device_W(Z, 1.0, F64))[2]
    _, _, cont = m.gp.natgrad_q(X, Y, lik, k_var=K_VAR, residual=residual, q0=(rm, rS), steps=8, rho=RHO, tol=0.0)
    assert np.abs(cont["elbo"] / r20["elbo"][12:] - 1).max() <= 1e-8


def test_float32_session_predicts_within_the_float32_restatements_error():
    """SVGPHetero in a float32 session (N = 1000, M = 64, d = 2: the fused strip kernel), 12 half steps from the prior, then
    predict_f and predict_noise_variance at X against the float64 restatement; bound: 4 x the error of the float32
    restatement (float32 A, marginals and weighted products, lam and beta rounded to float32, float64 tails) on the model's
    own float32 W.
    Observed on MI355X (device / float32 restatement): mean 7.1e-5 / 5.8e-5 (1.23 x), variance 1.0e-5 / 8.5e-6 (1.20 x),
    noise variance 2.8e-5 / 3.2e-5 (0.88 x); ELBO -497.0760 on both."""
    from henbun_amd.models import SVGPHetero

    c, ell = -2.0, 2.0
    X, Y, Z, _ = R.data(1000, 64, c, 2, d=2)
    m = SVGPHetero(X=X, Y=Y, Z=Z, log_var_mean=c, learn_likelihood=False, dtype="float32")
    m.gp.kern.lengthscales = np.ones(1) * ell
    m.k_var = np.ones(1) * K_VAR
    m.initialize()
    assert H.sgp_predict_multi_fused(F32, 1000, 64, 2, 2, True)
    m.reset_q()
    _, _, info = m.fit_q(steps=12, tol=0.0)
    fm, fv = m.predict_f(X)
    nv = m.predict_noise_variance(X)
    assert fm.dtype == np.float32 and fm.shape == (2, 1000) and nv.shape == (1000,)
    ells = np.ones(1) * ell

    def moments(dtype, W):
        q = R.natgrad(X, Y[:, 0], Z, ells, K_VAR, c, "neglected", RHO, 12, 0.0, dtype=dtype, W=W, ksplit=KSPLIT)
        dt = np.dtype(dtype).type
        d = (Z.astype(dt)[:, None, :] - X.astype(dt)[None, :, :]) / dt(ell)
        A = W.astype(dt) @ np.exp(dt(-0.5) * (d * d).sum(-1))
        mean, var = R.marginals(A, q[0].astype(dt), q[1].astype(dt), "neglected")
        mean, var = np.sqrt(K_VAR) * mean.astype(np.float64), K_VAR * var.astype(np.float64)
        return mean, var, np.exp(mean[1] + c + 0.5 * var[1]), q[2]

    r = moments(np.float64, _device_W(Z, ell, F64))
    q = moments(np.float32, _device_W(Z, ell, F32))
    for name, got, i in (("mean", fm, 0), ("var", fv, 1), ("noise variance", nv, 2)):
        b, g = np.abs(q[i] - r[i]).max(), np.abs(got - r[i]).max()
        print("hetgauss fp32 session %s: error %.3e (float32 restatement %.3e, %.2f x)" % (name, g, b, g / b))
        assert g <= 4.0 * b, name
    print("   elbo %.4f (float64 restatement %.4f)" % (info["elbo"][-1], r[3]["elbo"][-1]))


# ------------------------------------------------------------------------------------------------ elbo_and_grad_multi
def _bound(gap, scale):
    return 4.0 * max(gap, 1e-10 * scale)


@pytest.mark.parametrize("residual", ["diagonal", "neglected"])
def test_elbo_and_grad_multi_against_central_differences_of_the_restatement(residual):
    """float64, N = 300, M = 32, d = 1, at the q of 3 half steps from the prior (away from the fixed point).  Value: 1e-10
    relative.  Gradients of z, the lengthscale, k_var and c (lik_param): against central differences of the restatement at
    h = 1e-4, bound 4 x max(gap, 1e-10 scale) with gap = |difference at h - difference at 2 h| (three times the
    truncation error of the reference itself) and scale = max |gradient| of the block.
    Observed on MI355X (device error / gap): value 6.4e-15 relative; z 5.8e-7 / 1.8e-6, lengthscale 6.9e-6 / 2.1e-5, k_var
    2.7e-7 / 8.0e-7, lik_param 1.7e-7 / 5.0e-7 -- a third of the gap each, the truncation error of the difference at h."""
    c, h = -2.0, 1e-4
    jitter = float(hb.settings.numerics.jitter_level)
    X, Y, Z, _ = R.data(300, 32, c, 3)
    m = _Holder(Z=Z, ell=1.0, dtype="float64")
    m.initialize()
    lik = hb.likelihoods.HeteroscedasticGaussian(c)
    qm, qS, info = m.gp.natgrad_q(X, Y, lik, k_var=K_VAR, residual=residual, steps=3, rho=RHO, tol=0.0)
    assert info["residual"][-1] > 1e-6
    val, g = m.gp.elbo_and_grad_multi(X, Y, lik, (qm, qS), k_var=K_VAR, residual=residual, lik_grad=True)
    assert set(g) == {"z", "lengthscales", "k_var", "lik_param"} and g["z"].shape == (32, 1)
    y = Y[:, 0]
    f = lambda z=Z, ell=np.ones(1), k=K_VAR, cc=c: R.elbo(X, y, z, ell, k, cc, qm, qS, residual, jitter)
    ref = f()
    print("elbo_and_grad_multi hetgauss %s: value %.9f ref %.9f (rel %.2e)" % (residual, val, ref, abs(val / ref - 1)))
    assert abs(val - ref) <= 1e-10 * abs(ref)
    assert abs(val - info["elbo"][-1]) <= 1e-8 * abs(val)
    rows = []
    for name, got, fun, x0 in (("z", g["z"], lambda t: f(z=t), Z), ("lengthscales", g["lengthscales"], lambda t: f(ell=t), np.ones(1)),
                               ("k_var", np.array([g["k_var"]]), lambda t: f(k=float(t[0])), np.array([K_VAR])),
                               ("lik_param", np.array([g["lik_param"]]), lambda t: f(cc=float(t[0])), np.array([c]))):
        d1, d2 = R.central(fun, x0, h), R.central(fun, x0, 2 * h)
        rows.append((name, np.abs(np.reshape(got, d1.shape) - d1).max(), np.abs(d1 - d2).max(), np.abs(d1).max()))
    for name, err, gap, scale in rows:
        print("   %-12s device %.3e, gap %.3e, max|grad| %.3e, bound %.3e" % (name, err, gap, scale, _bound(gap, scale)))
    for name, err, gap, scale in rows:
        assert err <= _bound(gap, scale), name
    # lik_grad=False: the same bits without lik_param; a likelihood's parameter is the sum of r_g
    val2, g2 = m.gp.elbo_and_grad_multi(X, Y, lik, (qm, qS), k_var=K_VAR, residual=residual)
    assert val2 == val and set(g2) == {"z", "lengthscales", "k_var"} and all(np.array_equal(g[n], g2[n]) for n in g2)


# ------------------------------------------------------------------------------------------------ the model
def test_svgp_hetero_end_to_end():
    """N = 400, M = 24, d = 1, float64, c learnt.  reset_q(); fit_q() raises the ELBO at every step (to 1e-9) and writes
    blocks the model reads back unchanged; predict_noise_variance recovers the generating noise standard deviation within
    twice the restatement's own error on this set at the same hyper-parameters; predict_y is predict_f's mean and variance
    plus the noise variance; predict_log_density sums its points; fit_hyper(5) does not lower the fitted ELBO and moves c;
    the sampled ELBO over all rows (analytic KL, 128 draws) agrees with the closed-form value within 4 standard errors.
    Observed on MI355X: fit_q 23 steps to -235.4785 (the restatement's value), noise error 6.40 % (restatement 6.40 %);
    fit_hyper(5) -235.48 -> -234.36, c -2.693 -> -2.643; sampled ELBO -234.34 +- 0.26 against -234.36 (0.07 s.e.)."""
    from henbun_amd.models import SVGPHetero

    K = 128
    X, Y, Z, sd = R.data(400, 24, -2.0, 1)
    cfg = hb.settings.get_settings()
    cfg.numerics.kl_form = "analytic"
    with hb.settings.temp_settings(cfg):
        m = SVGPHetero(X=X, Y=Y, Z=Z, dtype="float64")
        m.gp.kern.lengthscales = np.ones(1)
        m.k_var = np.ones(1)
        m.initialize()
        c0 = m.current_likelihood().param
        assert abs(c0 - np.log(0.1 * np.var(Y))) <= 1e-12
        m.reset_q()
        qm, S, info = m.fit_q()
        bm, bS = m._current_blocks()
        assert qm.shape == (2, 24) and np.allclose(bm, qm, rtol=0, atol=1e-14) and np.allclose(bS, S, rtol=0, atol=1e-14)
        assert np.diff(info["elbo"]).min() >= -1e-9 * np.abs(info["elbo"]).max() and info["steps"] < 50
        nv = m.predict_noise_variance(X)
        rq = R.natgrad(X, Y[:, 0], Z, np.ones(1), 1.0, c0, "neglected", RHO, 50, 1e-8, jitter=float(cfg.numerics.jitter_level))
        rmean, rvar = R.marginals(R.whitened(X, Z, np.ones(1), float(cfg.numerics.jitter_level)), rq[0], rq[1], "neglected")
        err_ref = np.mean(np.abs(np.sqrt(np.exp(rmean[1] + c0 + 0.5 * rvar[1])) - sd) / sd)
        err = np.mean(np.abs(np.sqrt(nv) - sd) / sd)
        print("SVGPHetero: fit_q %d steps, elbo %.4f (restatement %.4f); noise sd error %.4f (restatement %.4f)"
              % (info["steps"], info["elbo"][-1], rq[2]["elbo"][-1], err, err_ref))
        assert err <= 2.0 * err_ref
        fm, fv = m.predict_f(X[:50])
        ym, yv = m.predict_y(X[:50])
        assert fm.shape == (2, 50) and np.array_equal(ym, fm[0]) and np.allclose(yv, fv[0] + nv[:50], rtol=1e-12)
        ld, total = m.predict_log_density(X[:50], Y[:50])
        ref_ld = R.logdens(Y[:50, 0], fm, fv, c0)
        assert np.abs(ld - ref_ld).max() <= 1e-10 * (1 + np.abs(ref_ld).max()) and abs(total - ld.sum()) <= 1e-12 * np.abs(ld).sum()
        trace = m.fit_hyper(5)
        c1 = m.current_likelihood().param
        print("   fit_hyper(5): %s; c %.4f -> %.4f" % (np.round(trace, 4), c0, c1))
        assert len(trace) == 6 and trace[-1] >= trace[0] and c1 != c0
        value = m.elbo_and_grad()[0]
        opt = m.ELBO()
        opt._ensure_compiled()
        obj = opt._trace(None)
        plan = m._session.make_plan([obj], minibatch=None)
        o = []
        for _ in range(K):
            plan.run()
            plan.check()
            o.append(float(np.ravel(plan.value(obj))[0]))
        mean, se = np.mean(o), np.std(o, ddof=1) / np.sqrt(K)
        print("   sampled ELBO %.3f +- %.3f, closed form %.3f (%.2f s.e.)" % (mean, se, value, abs(mean - value) / se))
        assert se > 0 and abs(mean - value) <= 4.0 * se
