"""tests/acq_ref.py, the restatement the GPU tests of hb_sgp_predict_grad / hb_sgp_acq compare against, pinned on the
host: its gradients against torch autograd of predict-style code written independently (optimal_q_ref.predict's
formulas) and against finite differences, its acquisition tails against scipy.stats.norm closed forms and autograd."""
import numpy as np
import pytest
import torch
from scipy.stats import norm

import acq_ref as R
import optimal_q_ref as OQ

MODES = ("diagonal", "neglected", "fullrank")


def _case(n, M, d, dl, wscale=1.0):
    return R.case(n, M, d, dl, seed=7 * n + M + d + dl, wscale=wscale)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("s_kind", ["diag", "tril"])
@pytest.mark.parametrize("shape", [(9, 12, 1, 1, 1.0), (14, 20, 3, 3, 1.0), (11, 16, 2, 1, 1.5)])
def test_gradients_against_autograd(shape, s_kind, mode):
    """mean, var against optimal_q_ref.predict; dmean, dvar against torch autograd of the same formulas in float64, within
    1e-10 of the absolute-sum scale grad_scale returns.  wscale 1.5 puts sum A^2 above 1 (rho = -1)."""
    n, M, d, dl, ws = shape
    x, z, ell, W, m, S, s, jitter = _case(n, M, d, dl, ws)
    Sq = s if s_kind == "diag" else S
    mean, var, dmean, dvar = R.moments_grad(x, z, ell, W, m, Sq, mode, jitter)
    if mode != "fullrank":
        pm, pv = OQ.predict(x, z, ell, jitter, m[None, :], Sq, residual=mode, W=W)
        assert np.abs(mean - pm[0]).max() <= 1e-12 * np.abs(pm).max() and np.abs(var - pv[0]).max() <= 1e-12 * np.abs(pv).max()
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    tm, tv = R.predict_torch(xt, *(torch.tensor(a, dtype=torch.float64) for a in (z, ell, W, m, Sq)), mode, jitter)
    gm, = torch.autograd.grad(tm.sum(), xt, retain_graph=True)
    gv, = torch.autograd.grad(tv.sum(), xt)
    sm, sv = R.grad_scale(x, z, ell, W, m, Sq, mode)
    em, ev = np.abs(dmean - gm.numpy()).max(0) / sm, np.abs(dvar - gv.numpy()).max(0) / sv
    if ws > 1.0:
        A = OQ.A_of(W, z, x, ell)
        assert ((A * A).sum(0) > 1.0).mean() > 0.5
    print("acq_ref %s %s %s: dmean %.2e dvar %.2e of scale" % (shape, s_kind, mode, em.max(), ev.max()))
    assert np.abs(mean - tm.detach().numpy()).max() <= 1e-12 * np.abs(mean).max()
    assert em.max() <= 1e-10 and ev.max() <= 1e-10


@pytest.mark.parametrize("mode", MODES)
def test_directional_finite_differences(mode):
    """Central differences of the restatement's own mean and var along a random direction, h = 1e-5: truncation h^2 / 6
    |f'''| and rounding eps scale / h both stay below 1e-6 of the scale."""
    x, z, ell, W, m, S, s, jitter = _case(12, 16, 3, 3)
    rng = np.random.RandomState(1)
    v = rng.randn(*x.shape)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    h = 1e-5
    mean, var, dmean, dvar = R.moments_grad(x, z, ell, W, m, S, mode, jitter)
    mp, vp = R.moments_grad(x + h * v, z, ell, W, m, S, mode, jitter)[:2]
    mm, vm = R.moments_grad(x - h * v, z, ell, W, m, S, mode, jitter)[:2]
    sm, sv = R.grad_scale(x, z, ell, W, m, S, mode)
    em = np.abs((mp - mm) / (2 * h) - (dmean * v).sum(1)).max() / sm.max()
    ev = np.abs((vp - vm) / (2 * h) - (dvar * v).sum(1)).max() / sv.max()
    print("acq_ref finite differences %s: dmean %.2e dvar %.2e of scale" % (mode, em, ev))
    assert em <= 1e-6 and ev <= 1e-6


@pytest.mark.parametrize("largest", [True, False])
def test_tails_against_scipy_and_autograd(largest):
    """EI, PI, UCB and their partials in mu' and v against scipy.stats.norm closed forms (1e-12 relative to the value's
    size) and against torch autograd through erfc; a clamped variance gives a_v = 0."""
    rng = np.random.RandomState(3)
    mean, var = rng.randn(50), rng.uniform(0.01, 2.0, 50)
    var[:3] = 1e-9
    best, xi, beta, sc, floor = 0.3, 0.05, 1.7, 1.3, 1e-6
    s = 1.0 if largest else -1.0
    mu, v = s * sc * mean, np.maximum(sc * sc * var, floor)
    sg = np.sqrt(v)
    u = (mu - s * best - xi) / sg
    want = dict(ei=(sg * (u * norm.cdf(u) + norm.pdf(u)), norm.cdf(u), norm.pdf(u) / (2 * sg)),
                pi=(norm.cdf(u), norm.pdf(u) / sg, -u * norm.pdf(u) / (2 * v)),
                ucb=(mu + beta * sg, np.ones_like(mu), beta / (2 * sg)))
    for kind in ("ei", "pi", "ucb"):
        par = beta if kind == "ucb" else xi
        val, a_mu, a_v, clamped = R.tail(kind, mean, var, best, par, sc, largest, floor)
        assert np.array_equal(clamped, sc * sc * var < floor) and clamped[:3].all() and np.all(a_v[clamped] == 0.0)
        wv, wm, wa = want[kind]
        for got, w in ((val, wv), (a_mu, wm), (a_v[~clamped], wa[~clamped])):
            assert np.abs(got - w).max() <= 1e-12 * max(1.0, np.abs(w).max())
        # autograd in (mu', v)
        tmu = torch.tensor(mu, requires_grad=True)
        tv = torch.tensor(v, requires_grad=True)
        tsg = torch.sqrt(tv)
        tu = (tmu - s * best - xi) / tsg
        Phi = 0.5 * torch.erfc(-tu / np.sqrt(2.0))
        phi = torch.exp(-0.5 * tu * tu) / np.sqrt(2.0 * np.pi)
        f = dict(ei=tsg * (tu * Phi + phi), pi=Phi, ucb=tmu + beta * tsg)[kind]
        g_mu, g_v = torch.autograd.grad(f.sum(), (tmu, tv))
        assert np.abs(a_mu - g_mu.numpy()).max() <= 1e-10 * max(1.0, np.abs(a_mu).max())
        assert np.abs(a_v[~clamped] - g_v.numpy()[~clamped]).max() <= 1e-10 * max(1.0, np.abs(a_v).max())
        # the chain rule of acquisition() on top
        dmean, dvar = rng.randn(50, 2), rng.randn(50, 2)
        val2, grad = R.acquisition(kind, mean, var, dmean, dvar, best, par, sc, largest, floor)
        assert np.array_equal(val2, val)
        assert np.allclose(grad, (s * sc * a_mu)[:, None] * dmean + (sc * sc * a_v)[:, None] * dvar, rtol=1e-15, atol=0)


def test_expected_improvement_far_below_the_incumbent():
    """u = -12: an fp32 u Phi(u) + phi(u) cancels to nothing there; the double tail through erfc stays positive, finite and
    within 1e-10 of scipy's log-space value."""
    sg = 0.5
    val, a_mu, a_v, _ = R.tail("ei", np.array([-12.0 * sg]), np.array([sg * sg]), best=0.0)
    want = sg * (-12.0 * norm.cdf(-12.0) + norm.pdf(-12.0))
    assert np.isfinite(val[0]) and val[0] > 0.0 and a_mu[0] > 0.0 and a_v[0] > 0.0
    assert abs(val[0] / want - 1.0) <= 1e-10


def test_maximise_improves_on_the_candidates():
    """The restated ascent never returns less than the best candidate, stays in the box, and moves towards a stationary
    point of the acquisition (the gradient at x_best is smaller than at the start)."""
    x, z, ell, W, m, S, s, jitter = _case(40, 16, 1, 1)
    kw = dict(mode="diagonal", jitter=jitter, k_var=1.3, best=0.5, param=0.01, var_floor=1e-6)
    xb, ab, idx = R.maximise(x, z, ell, W, m, s, "ei", **kw)
    sc = np.sqrt(1.3)
    a0, g0 = R.acquisition("ei", *R.moments_grad(x[idx:idx + 1], z, ell, W, m, s, "diagonal", jitter), 0.5, 0.01, sc, True, 1e-6)
    a1, g1 = R.acquisition("ei", *R.moments_grad(xb, z, ell, W, m, s, "diagonal", jitter), 0.5, 0.01, sc, True, 1e-6)
    assert ab[0] >= a0[0] and ab[0] == a1[0] and x.min() <= xb[0, 0] <= x.max()
    assert np.abs(g1).max() <= np.abs(g0).max() or ab[0] > a0[0]
