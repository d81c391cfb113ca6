"""Likelihoods with a parameter of their own (Laplace, Gamma, negative binomial, binomial) on the GPU, against the numpy
restatement tests/lik_zoo_ref.py (itself pinned on the host by tests/test_lik_zoo_cpu.py): the four kernels, natgrad_q,
elbo_and_grad(lik_grad=True), SVGPLik end to end and SVGPLik(learn_likelihood=True).fit_hyper.

Bounds are those of tests/test_sites_gpu.py.  float64 storage: 1e-12 per element, relative to the reference -- except
beta = g + lam mu, against the magnitudes of g's terms + |lam mu|, and sum_j dl_j/dparam, against the sum of the
magnitudes of its terms; sum_j l_j against sum_j |l_j| and the sum of the log densities against the sum of theirs; a
reference value below the smallest normal double (the Laplace lam at the corners underflows) absolutely against that
number.  float32 storage: 2 float32 ulps of the reference (double arithmetic, one rounding).  End to end: 1e-8.  Every
figure is printed before it is asserted."""
import math

import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd import graph as G
from henbun_amd import hip_ops as H
from henbun_amd.models import SVGPLik

import lik_zoo_ref as Z
import optimal_q_ref as R
import sites_ref as SR

pytestmark = pytest.mark.gpu

TINY = float(np.finfo(np.float64).tiny)
FMAX = float(np.finfo(np.float32).max)


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def _ulps32(got, ref):
    """|got - ref| in units of the float32 spacing at ref (ref saturated to the float32 range, as the kernels do): the
    measure of tests/test_sites_gpu.py."""
    ref = np.clip(ref, -FMAX, FMAX)
    a32 = np.maximum(np.abs(ref.astype(np.float32)), np.finfo(np.float32).tiny)
    with np.errstate(over="ignore"):
        up = np.nextafter(a32, np.float32(np.inf)) - a32
    ulp = np.where(np.isfinite(up), up, a32 - np.nextafter(a32, np.float32(0)))
    return np.abs(got.astype(np.float64) - ref) / ulp.astype(np.float64)


KERNEL_PARAM = {Z.GAUSSIAN: 0.7, Z.BERNOULLI: 1.0, Z.POISSON: 1.0, Z.LAPLACE: 0.7, Z.GAMMA: 2.5, Z.NEGBINOMIAL: 1.7,
                Z.BINOMIAL: 1000.0}
MS, VS = 1.25, 0.8
CLASSES = {Z.GAUSSIAN: hb.likelihoods.Gaussian, Z.LAPLACE: hb.likelihoods.Laplace, Z.GAMMA: hb.likelihoods.Gamma,
           Z.NEGBINOMIAL: hb.likelihoods.NegativeBinomial, Z.BINOMIAL: hb.likelihoods.Binomial}


def _rel(got, ref, scale=None):
    """max |got - ref| / scale; scale defaults to |ref|, and where that is below the smallest normal double, to it."""
    scale = np.abs(ref) if scale is None else scale
    return float((np.abs(got - ref) / np.maximum(scale, TINY)).max())


# ------------------------------------------------------------------------------------------------ 5. the kernels
@pytest.mark.parametrize("N", [1, 255, 1500])
@pytest.mark.parametrize("lik", Z.NEW)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_sites_predict_and_param_grad_against_the_restatement(dtype, lik, N):
    """hb_lik_sites / hb_lik_predict / hb_lik_param_grad for the four new ids: one element, one block minus one, several
    blocks with a ragged tail; the corners mu = +-30, v in {1e-12, 25}; a count of 1000 (the binomial's total count), a
    Gamma y of 1e-6; non-unit scales.  Everything finite; two runs of every sum bitwise equal; the binomial has no
    parameter gradient and says so."""
    dt = torch.float64 if dtype == "float64" else torch.float32
    npdt = np.float64 if dtype == "float64" else np.float32
    param = KERNEL_PARAM[lik]
    y, mu, v = (a.astype(npdt) for a in Z.site_inputs(lik, N, 7 * N + lik, param))
    yd, mud, vd = dev(y, dt), dev(mu, dt), dev(v, dt)
    lam, beta, lsum = H.lik_sites(lik, yd, mud, vd, param=param, mscale=MS, vscale=VS)
    _, _, lsum2 = H.lik_sites(lik, yd, mud, vd, param=param, mscale=MS, vscale=VS)
    ym, yv = H.lik_predict(lik, mud, vd, param=param)
    torch.cuda.synchronize()
    assert torch.equal(lsum, lsum2) and lsum.dtype == torch.float64
    lam, beta, ym, yv = (t.cpu().numpy() for t in (lam, beta, ym, yv))
    lsum = float(lsum.cpu()[0])
    y64, m64, v64 = y.astype(np.float64), MS * mu.astype(np.float64), VS * v.astype(np.float64)
    s = Z.site_terms(lik, y64, m64, v64, param)
    rbeta = s["g"] + s["lam"] * m64
    rym, ryv = Z.predict_y(lik, mu.astype(np.float64), v.astype(np.float64), param)
    assert all(np.all(np.isfinite(a)) for a in (lam, beta, ym, yv)) and np.isfinite(lsum)
    e_sum = abs(lsum - s["l"].sum()) / np.abs(s["l"]).sum()
    if lik == Z.BINOMIAL:
        with pytest.raises(RuntimeError, match="no continuous parameter"):
            H.lik_param_grad(lik, yd, mud, vd, param=param, mscale=MS, vscale=VS)
        e_l2 = e_dl = 0.0
    else:
        pg = H.lik_param_grad(lik, yd, mud, vd, param=param, mscale=MS, vscale=VS)
        pg2 = H.lik_param_grad(lik, yd, mud, vd, param=param, mscale=MS, vscale=VS)
        torch.cuda.synchronize()
        assert torch.equal(pg, pg2) and pg.dtype == torch.float64 and pg.shape == (2,)
        pg = pg.cpu().numpy()
        assert np.all(np.isfinite(pg))
        e_l2, e_dl = abs(pg[0] - s["l"].sum()) / np.abs(s["l"]).sum(), abs(pg[1] - s["dl"].sum()) / s["dl_mag"].sum()
    if dtype == "float64":
        e_lam = _rel(lam, s["lam"])
        e_beta = _rel(beta, rbeta, s["g_mag"] + np.abs(s["lam"] * m64))
        e_ym, e_yv = _rel(ym, rym), _rel(yv, ryv)
        print("%s float64 N=%d: lam %.2e beta %.2e sum %.2e; predict mean %.2e var %.2e; param grad: sum l %.2e, sum dl %.2e"
              % (Z.NAMES[lik], N, e_lam, e_beta, e_sum, e_ym, e_yv, e_l2, e_dl))
        assert max(e_lam, e_beta, e_sum, e_ym, e_yv, e_l2, e_dl) <= 1e-12
        return
    u = [float(_ulps32(a, b).max()) for a, b in ((lam, s["lam"]), (beta, rbeta), (ym, rym), (yv, ryv))]
    print("%s float32 N=%d: ulps lam %.2f beta %.2f predict mean %.2f var %.2f; sum %.2e; param grad: sum l %.2e, sum dl %.2e"
          % (Z.NAMES[lik], N, *u, e_sum, e_l2, e_dl))
    assert max(u) <= 2.0
    assert max(e_sum, e_l2, e_dl) <= 1e-12


@pytest.mark.parametrize("N", [1, 255, 1500])
@pytest.mark.parametrize("lik", (Z.GAUSSIAN, Z.BERNOULLI, Z.POISSON) + Z.NEW)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_logdens_against_the_restatement(dtype, lik, N):
    """hb_lik_logdens for all seven ids on the same inputs: per element, the sum against the sum of the magnitudes, the
    sum against the per-point values' own sum, two runs bitwise equal, everything finite; out = NULL gives the same sum."""
    dt = torch.float64 if dtype == "float64" else torch.float32
    npdt = np.float64 if dtype == "float64" else np.float32
    param = KERNEL_PARAM[lik]
    y, mu, v = (a.astype(npdt) for a in (Z.site_inputs(lik, N, 7 * N + lik, param) if lik in Z.NEW + (Z.BERNOULLI, Z.POISSON)
                                         else _gaussian_inputs(N, 7 * N + lik)))
    yd, mud, vd = dev(y, dt), dev(mu, dt), dev(v, dt)
    out, total = H.lik_logdens(lik, yd, mud, vd, param=param, mscale=MS, vscale=VS)
    _, total2 = H.lik_logdens(lik, yd, mud, vd, param=param, mscale=MS, vscale=VS)
    none, total3 = H.lik_logdens(lik, yd, mud, vd, param=param, mscale=MS, vscale=VS, pointwise=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(total, total2) and torch.equal(total, total3) and total.dtype == torch.float64
    out, total = out.cpu().numpy(), float(total.cpu()[0])
    ref = Z.logdens(lik, y.astype(np.float64), MS * mu.astype(np.float64), VS * v.astype(np.float64), param)
    assert np.all(np.isfinite(out)) and np.isfinite(total) and np.all(np.isfinite(ref))
    e_sum = abs(total - ref.sum()) / np.abs(ref).sum()
    if dtype == "float64":
        e = _rel(out, ref)
        e_own = abs(total - out.sum()) / np.abs(out).sum()
        print("%s float64 N=%d: log density %.2e, sum %.2e, sum against its own points %.2e" % (Z.NAMES[lik], N, e, e_sum, e_own))
        assert max(e, e_sum, e_own) <= 1e-12
        return
    u = float(_ulps32(out, ref).max())
    print("%s float32 N=%d: log density %.2f ulps, sum %.2e" % (Z.NAMES[lik], N, u, e_sum))
    assert u <= 2.0 and e_sum <= 1e-12


def _gaussian_inputs(N, seed):
    y, mu, v = Z.site_inputs(Z.LAPLACE, N, seed, 1.0)
    return y, mu, v


def test_binomial_of_one_trial_is_the_bernoulli_kernel():
    """Binomial(1) against the Bernoulli branch on the device: the same rule, to 1e-12 (the constant lgamma terms are 0)."""
    y, mu, v = Z.site_inputs(Z.BERNOULLI, 700, 3, 1.0)
    yd, mud, vd = (dev(a, torch.float64) for a in (y, mu, v))
    a = H.lik_sites(Z.BINOMIAL, yd, mud, vd, param=1.0, mscale=MS, vscale=VS)
    b = H.lik_sites(Z.BERNOULLI, yd, mud, vd, mscale=MS, vscale=VS)
    pa, pb = H.lik_predict(Z.BINOMIAL, mud, vd, param=1.0), H.lik_predict(Z.BERNOULLI, mud, vd)
    s = Z.site_terms(Z.BERNOULLI, y, MS * mu, VS * v)
    assert _rel(a[0].cpu().numpy(), b[0].cpu().numpy()) <= 1e-12
    assert _rel(a[1].cpu().numpy(), b[1].cpu().numpy(), np.abs(s["g"]) + np.abs(s["lam"] * MS * mu)) <= 1e-12
    assert abs(float(a[2].cpu()[0]) - float(b[2].cpu()[0])) <= 1e-12 * np.abs(s["l"]).sum()
    assert _rel(pa[0].cpu().numpy(), pb[0].cpu().numpy()) <= 1e-12 and _rel(pa[1].cpu().numpy(), pb[1].cpu().numpy()) <= 1e-12


# ------------------------------------------------------------------------------------------------ the models
_MODELS, _REF = {}, {}


def _likelihood(lik, param=None):
    return CLASSES[lik](Z.PARAM[lik] if param is None else param)


def _model(lik, dtype="float64", learn=False, param=None, data_param=None, cache=True):
    """(model, X, y, Zi) on lik_zoo_ref.problem(lik): lengthscale and k_var of the restatement; one model per key."""
    key = (lik, dtype, learn, param, data_param)
    if not cache or key not in _MODELS:
        X, y, Zi = Z.problem(lik, data_param)
        m = SVGPLik(X=X, Y=y, Z=Zi, likelihood=_likelihood(lik, param), learn_likelihood=learn, dtype=dtype)
        m.gp.kern.lengthscales = Z.ELL.copy()
        m.k_var = np.ones(1) * Z.K_VAR
        m.initialize()
        if not cache:
            return m, X, y, Zi
        _MODELS[key] = (m, X, y, Zi)
    return _MODELS[key]


def _ref(lik, rho, steps=8, tol=0.0, param=None):
    """The float64 restatement of the iteration from the prior on problem(lik, param), computed once per key."""
    key = (lik, rho, steps, tol, param)
    if key not in _REF:
        X, y, Zi = Z.problem(lik, param)
        _REF[key] = Z.natgrad(X, y, Zi, Z.ELL, hb.settings.numerics.jitter_level, lik, Z.PARAM[lik] if param is None else param,
                              Z.K_VAR, steps=steps, rho=rho, tol=tol)
    return _REF[key]


# ------------------------------------------------------------------------------------------------ 6. natgrad_q
@pytest.mark.parametrize("rho", [1.0, 0.5])
@pytest.mark.parametrize("lik", Z.NEW)
def test_natgrad_q_fp64_follows_the_restatement(lik, rho):
    """8 steps from the prior in a float64 session, as tests/test_sites_gpu.py holds Bernoulli and Poisson: the ELBO trace
    to 1e-8 relative, the residual trace to 1e-8, m and S S^T to 1e-8 of their largest entry; no CholeskyError at either
    rho (log-concavity).  tol = 0 still stops an iteration whose ELBO repeats to the last bit (the binomial's does after
    7 steps in the restatement): the traces are compared over their common length, which must be at least 8 entries.
    The parameters are lik_zoo_ref.NATGRAD_PARAM: the other tests' except the Laplace scale, 1 here.  At scale 0.3 the
    undamped Laplace iteration diverges (ELBO -1.2e4 -> -1.7e7 at rho = 1; likelihoods.Laplace.natgrad_rho) and the
    restatement's own traces move by 9.5e-7 under a one-ulp change of the labels (tests/test_lik_zoo_cpu.py), so 1e-8
    asks nothing there.  Observed on MI355X at scale 0.3, rho = 1: ELBO trace 5.3e-9, residual trace 4.6e-7, m 2.4e-13,
    S S^T 4.3e-12; at rho = 0.5 all four within 1e-8."""
    assert hb.settings.numerics.jitter_level == SR.JITTER
    p = Z.NATGRAD_PARAM[lik]
    m, X, y, Zi = _model(lik, param=p, data_param=p)
    qm, S, info = m.gp.natgrad_q(X, y, _likelihood(lik, p), k_var=Z.K_VAR, steps=8, rho=rho, tol=0.0)
    rm, rS, rinfo = _ref(lik, rho, param=p)
    n = min(len(info["elbo"]), len(rinfo["elbo"]))
    assert n >= 8 and len(info["residual"]) == len(info["elbo"])
    assert qm.shape == (1, 32) and S.shape == (32, 32) and np.array_equal(S, np.tril(S)) and np.all(np.diag(S) > 0)
    e_elbo = np.abs(info["elbo"][:n] / rinfo["elbo"][:n] - 1).max()
    e_res = np.abs(info["residual"][:n] - rinfo["residual"][:n]).max()
    e_m = np.abs(qm - rm).max() / np.abs(rm).max()
    e_S = np.abs(S @ S.T - rS @ rS.T).max() / np.abs(rS @ rS.T).max()
    print("natgrad_q fp64 %s rho %.1f: elbo %.3f -> %.3f (rel err %.2e), residual -> %.2e (err %.2e), m %.2e S S^T %.2e"
          % (Z.NAMES[lik], rho, info["elbo"][0], info["elbo"][-1], e_elbo, info["residual"][-1], e_res, e_m, e_S))
    assert e_elbo <= 1e-8 and e_res <= 1e-8 and e_m <= 1e-8 and e_S <= 1e-8


# ------------------------------------------------------------------------------------------------ 7. elbo_and_grad
@pytest.mark.parametrize("lik", Z.TRAINABLE)
def test_elbo_and_grad_lik_param_against_the_restatement(lik):
    """grad['lik_param'] at the restatement's q (8 steps from the prior at the likelihood's own damping) against the
    restated sum_j dl_j/dparam at the restated marginals of that q: 1e-10 of the sum of the magnitudes of its terms (a
    chunked float64 sum, one order looser than per element).  The other entries and the value are bitwise those of
    lik_grad=False."""
    m, X, y, Zi = _model(lik)
    qm, S, _ = _ref(lik, Z.RHO.get(lik, 1.0))
    val, grad = m.gp.elbo_and_grad(X, y, _likelihood(lik), (qm, S), k_var=Z.K_VAR, lik_grad=True)
    val0, grad0 = m.gp.elbo_and_grad(X, y, _likelihood(lik), (qm, S), k_var=Z.K_VAR)
    assert sorted(grad) == ["k_var", "lengthscales", "lik_param", "z"] and sorted(grad0) == ["k_var", "lengthscales", "z"]
    assert val == val0 and all(np.array_equal(grad[k], grad0[k]) for k in grad0)
    mu, v = Z.marginals_of(X, Zi, Z.ELL, hb.settings.numerics.jitter_level, qm, S, Z.K_VAR)
    s = Z.site_terms(lik, y, mu, v, Z.PARAM[lik])
    e = abs(grad["lik_param"] - s["dl"].sum()) / s["dl_mag"].sum()
    print("%s: lik_param %.6f (restatement %.6f), %.2e of the terms' magnitudes" % (Z.NAMES[lik], grad["lik_param"], s["dl"].sum(), e))
    assert isinstance(grad["lik_param"], float) and e <= 1e-10


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_elbo_and_grad_default_is_bitwise_what_lik_grad_leaves(dtype):
    """In a float32 and a float64 session (the routine is float64 either way): value and the three other entries with
    lik_grad=True are the bits of the default call, for a new likelihood and for the Gaussian; Bernoulli refuses."""
    for lik in (Z.NEGBINOMIAL, Z.GAUSSIAN):
        m, X, y, Zi = _model(lik, dtype)
        rng = np.random.RandomState(11)
        q = (0.3 * rng.randn(1, 32), np.tril(0.05 * rng.randn(32, 32)) + 0.5 * np.eye(32))
        val, grad = m.gp.elbo_and_grad(X, y, _likelihood(lik), q, k_var=Z.K_VAR, lik_grad=True)
        val0, grad0 = m.gp.elbo_and_grad(X, y, _likelihood(lik), q, k_var=Z.K_VAR)
        assert val == val0 and sorted(grad0) == ["k_var", "lengthscales", "z"] and np.isfinite(grad["lik_param"])
        assert all(np.array_equal(grad[k], grad0[k]) for k in grad0)
    with pytest.raises(ValueError, match="lik_grad"):
        m.gp.elbo_and_grad(X, y, hb.likelihoods.Bernoulli(), q, k_var=Z.K_VAR, lik_grad=True)


def test_gaussian_lik_param_is_the_collapsed_bounds_noise_gradient():
    """Gaussian(s2) at q = optimal_q: lik_param equals collapsed_bound_and_grad's noise_var entry (envelope property) to
    1e-8 relative."""
    m, X, y, Zi = _model(Z.GAUSSIAN)
    s2 = 0.4
    q = m.gp.optimal_q(X, y, s2, Z.K_VAR)
    _, grad = m.gp.elbo_and_grad(X, y, hb.likelihoods.Gaussian(s2), q, k_var=Z.K_VAR, lik_grad=True)
    _, cgrad = m.gp.collapsed_bound_and_grad(X, y, s2, Z.K_VAR)
    print("Gaussian: lik_param %.9f, collapsed bound's noise_var %.9f" % (grad["lik_param"], cgrad["noise_var"]))
    assert abs(grad["lik_param"] / cgrad["noise_var"] - 1) <= 1e-8


# ------------------------------------------------------------------------------------------------ 8. SVGPLik end to end
def _param_grad_plan(m):
    """(plan, d objective / d raw lik_param) of the model's own sampled ELBO on ALL rows (tests/test_sites_gpu.py)."""
    opt = m.ELBO()
    opt._ensure_compiled()
    m.initialize()
    obj = opt._trace(None)
    grads = G.gradients(obj, [object.__getattribute__(m, "lik_param")._leaf])
    return m._session.make_plan([obj] + grads, minibatch=None), grads[0]


@pytest.mark.parametrize("lik", Z.NEW)
def test_svgplik_end_to_end(lik):
    """reset_q(); fit_q() with the likelihood's own damping, then against the restatement of the same iteration (20 steps,
    tol 1e-8): predict_y is the restated predictive of the restated marginals (1e-8 relative) and predict_log_density of
    the first 200 rows the restated log density (1e-8 of max(1, |.|)), its sum the sum of its points (1e-12).  With
    learn_likelihood=True (the binomial has nothing to learn) the model starts at the same parameter, so all of the
    above is asked of IT, and the gradient of its sampled ELBO (all rows, analytic KL, 64 draws) with respect to the raw
    lik_param agrees with elbo_and_grad()'s closed-form entry within 4 standard errors of the average."""
    cfg = hb.settings.get_settings()
    cfg.numerics.kl_form = "analytic"
    with hb.settings.temp_settings(cfg):
        learn = lik in Z.TRAINABLE
        m, X, y, Zi = _model(lik, learn=learn, cache=False)
        param, rho = Z.PARAM[lik], Z.RHO.get(lik, 1.0)
        assert abs(m.current_likelihood().param / param - 1) <= 1e-14
        m.reset_q()
        qm, S, info = m.fit_q()
        rm, rS, rinfo = _ref(lik, rho, steps=20, tol=1e-8)
        assert info["steps"] == rinfo["steps"]
        xs = np.linspace(-1.0, 17.0, 200)[:, None]
        ym, yv = m.predict_y(xs)
        rmu, rv = R.predict(xs, Zi, Z.ELL, hb.settings.numerics.jitter_level, rm, rS, Z.K_VAR)
        rym, ryv = Z.predict_y(lik, rmu, rv, param)
        e_ym, e_yv = _rel(ym, rym), _rel(yv, ryv)
        ld, total = m.predict_log_density(X[:200], y[:200])
        rmu, rv = R.predict(X[:200], Zi, Z.ELL, hb.settings.numerics.jitter_level, rm, rS, Z.K_VAR)
        rld = Z.logdens(lik, y[:200], rmu, rv, param).reshape(1, -1)
        e_ld = _rel(ld, rld, np.maximum(1.0, np.abs(rld)))
        print("%s: fit_q %d steps, elbo %.3f (restatement %.3f); predict_y mean %.2e var %.2e; log density %.2e, sum %.4f"
              % (Z.NAMES[lik], info["steps"], info["elbo"][-1], rinfo["elbo"][-1], e_ym, e_yv, e_ld, total))
        assert ym.shape == (1, 200) and ld.shape == (1, 200)
        assert max(e_ym, e_yv, e_ld) <= 1e-8
        assert abs(total - ld.sum()) <= 1e-12 * np.abs(ld).sum()
        if not learn:
            return
        K = 64
        plan, gleaf = _param_grad_plan(m)
        g = []
        for _ in range(K):
            plan.run()
            plan.check()
            g.append(float(np.ravel(plan.value(gleaf))[0]))
        mean, se = np.mean(g), np.std(g, ddof=1) / np.sqrt(K)
        _, grad = m.elbo_and_grad()
        closed = float(np.ravel(grad["lik_param"])[0])
        print("%s: d ELBO / d raw lik_param: sampled %.4f +- %.4f, closed form %.4f (%.2f s.e.)"
              % (Z.NAMES[lik], mean, se, closed, abs(mean - closed) / se))
        assert se > 0 and abs(mean - closed) <= 4.0 * se


# ------------------------------------------------------------------------------------------------ 9. learning the parameter
@pytest.mark.parametrize("lik", Z.TRAINABLE)
def test_fit_hyper_learns_the_likelihood_parameter(lik):
    """Data drawn with theta* (Laplace scale 0.3, Gamma shape 4, negative binomial dispersion 2, Gaussian variance 0.09),
    the model started at 3 theta*: after fit_hyper(steps=30, lr=0.05, train_z=False) the last ELBO exceeds the first and
    theta is closer to theta* in log than log 3 (tests/test_lik_zoo_cpu.py shows both attainable in the restatement).  The
    likelihood object handed in keeps its parameter.  With learn_likelihood=False the model has no lik_param, leaves the
    parameter alone, and two such models, run at the same settings, give bitwise the same trace."""
    star = Z.THETA_STAR[lik]
    m, X, y, Zi = _model(lik, learn=True, param=3.0 * star, data_param=star, cache=False)
    handed = object.__getattribute__(m, "likelihood")
    assert list(m._hyper_variables()) == ["z", "lengthscales", "k_var", "lik_param"]
    m.reset_q()
    trace = m.fit_hyper(steps=30, lr=0.05, train_z=False)
    end = m.current_likelihood().param
    print("%s: theta %.4f -> %.4f (theta* %.4f), ELBO %.3f -> %.3f" % (Z.NAMES[lik], 3.0 * star, end, star, trace[0], trace[-1]))
    assert len(trace) == 31 and np.all(np.isfinite(trace))
    assert trace[-1] > trace[0]
    assert abs(math.log(end / star)) < math.log(3.0)
    assert handed.param == 3.0 * star
    traces = []
    for _ in range(2):
        m0, _, _, _ = _model(lik, learn=False, param=3.0 * star, data_param=star, cache=False)
        assert list(m0._hyper_variables()) == ["z", "lengthscales", "k_var"]
        m0.reset_q()
        traces.append(m0.fit_hyper(steps=30, lr=0.05, train_z=False))
        assert object.__getattribute__(m0, "likelihood").param == 3.0 * star == m0.current_likelihood().param
    assert np.array_equal(traces[0], traces[1])
