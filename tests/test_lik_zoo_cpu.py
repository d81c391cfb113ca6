"""Likelihoods with a parameter of their own (Laplace, Gamma, negative binomial, binomial) on the host.  The numpy
restatement the GPU tests lean on (tests/lik_zoo_ref.py) is pinned independently -- against scipy's adaptive quadrature of
log p N and p N, and against torch autograd of its torch twin for g = dl/dmu, lam = -2 dl/dv and dl/dparam; the new C
entries are bound and refuse bad arguments before any launch; the Python classes carry the ids and validate; the graph
expressions of logp equal the restatement on the CPU graph oracle; and the loop that learns the parameter works in the
restatement alone, which shows that what tests/test_lik_zoo_gpu.py asks of SVGPLik.fit_hyper is attainable.  No HIP kernel
runs here.

Bounds.  Closed-form quantities (Laplace, Gamma; every dl/dparam and every g, which are exact derivatives of the rule):
1e-12 relative to the sum of the magnitudes of the terms added, plus the error estimate adaptive quadrature returns where
it is the reference.  Quantities that carry the error of the 20-node rule: at most 4 x the largest difference between the
20-node and the 96-node restatement measured on the box mu in [-4, 4], v in [e^-6, 1] (the figures DESIGN.md 3 quotes,
recorded below; the test measures them again and holds them to that) -- GH20_SITES for l, g, lam and the predictive
moments of the negative binomial and the binomial, GH20_LOGDENS for the log densities by the rule.  The latter are large
where a sharply peaked likelihood meets a wide marginal (a Poisson count of 42 at v = 0.64: 0.43 nats): the rule's
property, which is why the log densities are ALSO held to round-off against quadrature where v <= 0.02, the
marginals a fitted model predicts with."""
import math

import numpy as np
import pytest
import scipy.integrate
import torch

import lik_zoo_ref as Z
import sites_ref as SR

PARAM = {Z.LAPLACE: 0.7, Z.GAMMA: 2.5, Z.NEGBINOMIAL: 1.7, Z.BINOMIAL: 12.0}
# largest |20 nodes - 96 nodes| on the box as measured by test_twenty_nodes_against_ninety_six_on_the_box (400 points): the
# rule's own error at v <= 1, not round-off.  Sites and predictive moments relative to the terms' magnitudes (worst: lam of
# the negative binomial, the predictive variance of the binomial); log densities absolute (they are logarithms)
GH20_SITES = {Z.NEGBINOMIAL: 6.2e-10, Z.BINOMIAL: 9.7e-9}
GH20_LOGDENS = {Z.BERNOULLI: 1.5e-10, Z.POISSON: 0.44, Z.GAMMA: 5.8e-4, Z.NEGBINOMIAL: 3.7e-5, Z.BINOMIAL: 3.6e-5}


def _box(lik, n=40, seed=5):
    """(y, mu, v) on the box mu in [-4, 4], v in [e^-6, 1]: its four corners, then uniform draws; y from the likelihood."""
    rng = np.random.RandomState(seed + lik)
    mu, v = rng.uniform(-4, 4, n), np.exp(rng.uniform(-6, 0, n))
    for i, (a, c) in enumerate([(-4.0, math.exp(-6)), (4.0, math.exp(-6)), (-4.0, 1.0), (4.0, 1.0)]):
        mu[i], v[i] = a, c
    y = Z.draw(lik, mu, PARAM.get(lik, 0.5), rng)
    if lik == Z.GAMMA:
        y = np.maximum(y, 1e-6)
    return y, mu, v


def _quad(fun, mu, v, breaks=()):
    """(integral of fun(f) N(f; mu, v) df, error estimate) over mu +- 14 sd."""
    sd = math.sqrt(v)
    lo, hi = mu - 14 * sd, mu + 14 * sd
    pts = [p for p in breaks if lo < p < hi] or None
    g = lambda f: fun(f) * math.exp(-0.5 * ((f - mu) / sd) ** 2) / (sd * math.sqrt(2 * math.pi))
    val, err = scipy.integrate.quad(g, lo, hi, points=pts, epsabs=0.0, epsrel=1e-13, limit=400)
    return val, err


# ---------------------------------------------------------------- 1. the restatement, pinned independently
@pytest.mark.parametrize("lik", Z.NEW)
def test_restated_l_against_adaptive_quadrature(lik):
    """l = E log p against scipy.integrate.quad of log p N (Laplace: break point at y).  The two closed forms with 20
    nodes' worth of nothing: 1e-12 of the terms' magnitudes; the two Gauss-Hermite likelihoods through the 96-node
    restatement, which must be converged (1e-12 too), the 20-node one then within 4 x GH20_SITES of it."""
    y, mu, v = _box(lik)
    p = PARAM[lik]
    nodes = 96 if lik in Z.QUADRATURE else 20
    s = Z.site_terms(lik, y, mu, v, p, nodes=nodes)
    worst = raw = 0.0
    for j in range(y.size):
        ref, err = _quad(lambda f: float(Z.log_p(lik, y[j], f, p)), mu[j], v[j], breaks=(y[j],))
        worst, raw = max(worst, (abs(s["l"][j] - ref) - err) / s["l_mag"][j]), max(raw, abs(s["l"][j] - ref) / s["l_mag"][j])
    print("%s: l against quad, worst %.2e of the terms (%.2e beyond quad's own estimate)" % (Z.NAMES[lik], raw, worst))
    assert worst <= 1e-12
    if lik in Z.QUADRATURE:
        s20 = Z.site_terms(lik, y, mu, v, p)
        assert (np.abs(s20["l"] - s["l"]) / s["l_mag"]).max() <= 4.0 * GH20_SITES[lik]


@pytest.mark.parametrize("lik", Z.NEW + (Z.GAUSSIAN,))
def test_restated_g_lam_and_param_gradient_against_autograd(lik):
    """torch.autograd (float64) of the restated l: dl/dmu = g, -2 dl/dv = lam, dl/dparam.  g and dl/dparam are exact
    derivatives of what l is (closed form or the rule itself): 1e-12 of their terms.  lam = -2 dl/dv is exact for the
    closed forms -- for Laplace dA/dv is the difference of two terms (1 + delta^2 / v) times its size, which is what its
    error is measured against -- and Stein's identity up to the rule's error for the other two: 4 x GH20_SITES."""
    y, mu, v = _box(lik)
    p = PARAM.get(lik, 0.5)
    s = Z.site_terms(lik, y, mu, v, p)
    ty, tmu, tv = (torch.tensor(a, dtype=torch.float64) for a in (y, mu, v))
    tmu.requires_grad_(True), tv.requires_grad_(True)
    tp = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    lt = Z.l_torch(lik, ty, tmu, tv, tp)
    assert np.abs(lt.detach().numpy() - s["l"]).max() <= 1e-12 * s["l_mag"].max()
    gmu, gv = (a.numpy() for a in torch.autograd.grad(lt.sum(), [tmu, tv], retain_graph=True))
    e_g = (np.abs(gmu - s["g"]) / s["g_mag"]).max()
    lam_mag = s["lam"] * (1.0 + (mu - y) ** 2 / v) if lik == Z.LAPLACE else np.maximum(s["lam"], s["g_mag"])
    e_lam = (np.abs(-2.0 * gv - s["lam"]) / np.maximum(lam_mag, np.finfo(np.float64).tiny)).max()
    print("%s: g %.2e lam %.2e" % (Z.NAMES[lik], e_g, e_lam))
    assert e_g <= 1e-12
    assert e_lam <= (4.0 * GH20_SITES[lik] if lik in Z.QUADRATURE else 1e-12)
    if lik in Z.TRAINABLE:
        dps = np.array([float(torch.autograd.grad(lt[j], tp, retain_graph=True)[0]) for j in range(y.size)])
        e_p = (np.abs(dps - s["dl"]) / s["dl_mag"]).max()
        print("%s: dl/dparam %.2e" % (Z.NAMES[lik], e_p))
        assert e_p <= 1e-12
    else:
        assert np.all(s["dl"] == 0.0)


def test_twenty_nodes_against_ninety_six_on_the_box():
    """The measured error of the 20-node rule on the box, every quantity the kernels take from it: l, g, lam (relative to
    the terms' magnitudes) and the predictive moments (relative), and the log density (absolute, it is a logarithm).
    Printed; held to 4 x the recorded figures."""
    for lik in (Z.NEGBINOMIAL, Z.BINOMIAL, Z.BERNOULLI, Z.POISSON, Z.GAMMA):
        y, mu, v = _box(lik, n=400)
        p = PARAM.get(lik, 1.0)
        if lik in Z.QUADRATURE:
            a, b = Z.site_terms(lik, y, mu, v, p), Z.site_terms(lik, y, mu, v, p, nodes=96)
            worst = max(float((np.abs(a[k] - b[k]) / b[m]).max()) for k, m in (("l", "l_mag"), ("g", "g_mag"), ("lam", "g_mag")))
            if lik == Z.BINOMIAL:
                pa, pb = Z.predict_y(lik, mu, v, p), Z.predict_y(lik, mu, v, p, nodes=96)
                worst = max(worst, float(np.abs(pa[0] / pb[0] - 1).max()), float(np.abs(pa[1] / pb[1] - 1).max()))
            print("%s: sites, 20 against 96 nodes on the box: %.3e (recorded %.3e)" % (Z.NAMES[lik], worst, GH20_SITES[lik]))
            assert worst <= 4.0 * GH20_SITES[lik]
        d = np.abs(Z.logdens(lik, y, mu, v, p) - Z.logdens(lik, y, mu, v, p, nodes=96))
        print("%s: log density, 20 against 96 nodes on the box: %.3e (recorded %.3e); where v <= 0.1: %.3e"
              % (Z.NAMES[lik], d.max(), GH20_LOGDENS[lik], d[v <= 0.1].max()))
        assert d.max() <= 4.0 * GH20_LOGDENS[lik]


def test_binomial_one_is_bernoulli_and_gamma_one_is_exponential():
    y, mu, v = _box(Z.BERNOULLI)
    for a, b in zip(Z.sites(Z.BINOMIAL, y, mu, v, 1.0), SR.sites(SR.BERNOULLI, y, mu, v)):
        assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1.0)
    pa, pb = Z.predict_y(Z.BINOMIAL, mu, v, 1.0), SR.predict_y(SR.BERNOULLI, mu, v)
    assert np.abs(pa[0] - pb[0]).max() <= 1e-12
    assert np.abs(pa[1] - pb[1]).max() <= 1e-12          # n E s(1-s) + n^2 E(s-p)^2 = p (1 - p) at n = 1
    assert np.abs(Z.logdens(Z.BINOMIAL, y, mu, v, 1.0) - Z.logdens(Z.BERNOULLI, y, mu, v)).max() <= 1e-12
    y, mu, v = _box(Z.GAMMA)
    f = np.linspace(-3, 3, 7)
    assert np.abs(Z.log_p(Z.GAMMA, y[:, None], f[None, :], 1.0) - (-f[None, :] - y[:, None] * np.exp(-f[None, :]))).max() <= 1e-12
    l = Z.sites(Z.GAMMA, y, mu, v, 1.0)[0]
    ref = -mu - y * np.exp(-mu + 0.5 * v)
    assert np.abs(l - ref).max() <= 1e-12 * (np.abs(mu) + y * np.exp(-mu + 0.5 * v)).max()


def _logdens_by_quad(lik, y, mu, v, p):
    """log integral p(y | f) N df by adaptive quadrature of exp(log p - c), c = the largest log p on a grid (no underflow)."""
    grid = np.linspace(mu - 14 * math.sqrt(v), mu + 14 * math.sqrt(v), 201)
    c = float(np.max(Z.log_p(lik, y, grid, p)))
    val, err = _quad(lambda f: math.exp(float(Z.log_p(lik, y, f, p)) - c), mu, v, breaks=(y,))
    return c + math.log(val), err / val


@pytest.mark.parametrize("lik", (Z.GAUSSIAN, Z.BERNOULLI, Z.POISSON) + Z.NEW)
def test_restated_log_density_against_adaptive_quadrature(lik):
    """log integral p(y | f) N(f; mu, v) df against quad of p N on the box.  Gaussian and Laplace (closed form): 1e-12
    plus quad's own relative error estimate; the others carry the 20-node rule's error: 4 x GH20_LOGDENS on the box, and
    1e-12 (plus quad's estimate) where v <= 0.02, where the rule has converged.  Laplace also at |y - mu| / b = 40 with
    v = 1e-8 on either side, and at v = 25: finite, and right in log space."""
    y, mu, v = _box(lik)
    p = PARAM.get(lik, 0.5)
    if lik == Z.LAPLACE:
        y = np.concatenate([y, [1.0 + 40 * p, 1.0 - 40 * p, 0.3, -2.0]])
        mu = np.concatenate([mu, [1.0, 1.0, 0.2, 30.0]])
        v = np.concatenate([v, [1e-8, 1e-8, 25.0, 25.0]])
    got = Z.logdens(lik, y, mu, v, p)
    assert np.all(np.isfinite(got))
    worst = narrow = 0.0
    for j in range(y.size):
        ref, rel = _logdens_by_quad(lik, y[j], mu[j], v[j], p)
        worst = max(worst, abs(got[j] - ref) - rel)
        if v[j] <= 0.02:
            narrow = max(narrow, abs(got[j] - ref) - rel)
    closed = lik in (Z.GAUSSIAN, Z.LAPLACE)
    print("%s: log density against quad, worst %.2e; where v <= 0.02 (%d points) %.2e" % (Z.NAMES[lik], worst, (v <= 0.02).sum(), narrow))
    assert (v <= 0.02).sum() >= 10
    assert worst <= (1e-12 * max(1.0, np.abs(got).max()) if closed else 4.0 * GH20_LOGDENS[lik])
    assert narrow <= 1e-12 * max(1.0, np.abs(got).max())
    if lik == Z.LAPLACE:
        assert abs(got[-4] - (-math.log(2 * p) - 40.0 + 1e-8 / (2 * p * p))) <= 1e-12 * 40


def test_restated_predictive_moments_against_adaptive_quadrature():
    """E y and var y under f ~ N(mu, v) from the conditional moments by quad: Gamma, negative binomial (closed form,
    1e-12 plus quad's estimate) and binomial (the rule: 4 x GH20_SITES)."""
    for lik in (Z.GAMMA, Z.NEGBINOMIAL, Z.BINOMIAL, Z.LAPLACE):
        _, mu, v = _box(lik, n=12)
        p = PARAM[lik]
        sig = lambda f: 1.0 / (1.0 + math.exp(-f))
        mean_f = {Z.GAMMA: math.exp, Z.NEGBINOMIAL: math.exp, Z.BINOMIAL: lambda f: p * sig(f), Z.LAPLACE: lambda f: f}[lik]
        var_f = {Z.GAMMA: lambda f: math.exp(2 * f) / p, Z.NEGBINOMIAL: lambda f: math.exp(f) + math.exp(2 * f) / p,
                 Z.BINOMIAL: lambda f: p * sig(f) * (1 - sig(f)), Z.LAPLACE: lambda f: 2 * p * p}[lik]
        ym, yv = Z.predict_y(lik, mu, v, p)
        worst = 0.0
        for j in range(mu.size):
            m1, e1 = _quad(mean_f, mu[j], v[j])
            m2, e2 = _quad(lambda f: var_f(f) + (mean_f(f) - m1) ** 2, mu[j], v[j])
            worst = max(worst, (abs(ym[j] - m1) - e1) / max(abs(m1), 1e-300), (abs(yv[j] - m2) - e2) / m2)
        print("%s: predictive moments against quad, worst %.2e" % (Z.NAMES[lik], worst))
        assert worst <= (4.0 * GH20_SITES[lik] if lik == Z.BINOMIAL else 1e-12)


# ---------------------------------------------------------------- 2. the C entries
NEW_SYMBOLS = ("hb_lik_param_grad_f32", "hb_lik_param_grad_f64", "hb_lik_param_grad_ws_elems", "hb_lik_logdens_f32",
               "hb_lik_logdens_f64")


def _call(lib, entry, suffix, lik=1, N=10, param=1.0):
    """(the pointers are the integer 1: any launch would fault -- every case must return before one)"""
    if entry == "hb_lik_sites":
        return lib.raw(entry + suffix)(lik, 1, 1, 1, 1.0, 1.0, param, 1, 1, 1, N, 1, None)
    if entry == "hb_lik_predict":
        return lib.raw(entry + suffix)(lik, 1, 1, param, 1, 1, N, None)
    if entry == "hb_lik_param_grad":
        return lib.raw(entry + suffix)(lik, 1, 1, 1, 1.0, 1.0, param, 1, N, 1, None)
    return lib.raw(entry + suffix)(lik, 1, 1, 1, 1.0, 1.0, param, 1, 1, N, 1, None)


ENTRIES = ("hb_lik_sites", "hb_lik_predict", "hb_lik_param_grad", "hb_lik_logdens")


def test_new_symbols_are_exported_and_bound_and_the_version_stays():
    from henbun_amd import _lib

    names, lib = _lib.declared_symbols(), _lib.lib()
    for n in NEW_SYMBOLS:
        assert n in names and lib.raw(n) is not None
    assert lib.raw("hb_version")() == 2
    f, g = lib.raw("hb_lik_param_grad_ws_elems"), lib.raw("hb_lik_sites_ws_elems")
    assert f(1) == 2 and f(257) == 4 and f(10 ** 6) == f(10 ** 8) == 2 * g(10 ** 8) <= 2048


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_points_refuse_before_launching(entry, suffix):
    from henbun_amd import _lib

    lib = _lib.lib()
    cases = [(dict(lik=16, param=0.0), "scale"), (dict(lik=16, param=-1.0), "scale"), (dict(lik=17, param=0.0), "shape"),
             (dict(lik=17, param=-2.0), "shape"), (dict(lik=18, param=0.0), "dispersion"),
             (dict(lik=18, param=float("nan")), "dispersion"), (dict(lik=19, param=0.5), "total count"),
             (dict(lik=19, param=2.5), "total count"), (dict(lik=19, param=0.0), "total count")]
    cases += [(dict(lik=i), "unknown likelihood") for i in list(range(3, 16)) + [20, -1]]
    cases += [(dict(lik=i, N=-1), "negative N") for i in (0, 16, 17, 18, 19)]
    if entry == "hb_lik_param_grad":
        cases += [(dict(lik=i), "no continuous parameter") for i in (1, 2, 19)]
    for bad, word in cases:
        rc = _call(lib, entry, suffix, **bad)
        assert rc < 0 and word in lib.last_error() and entry in lib.last_error(), (bad, rc, lib.last_error())


# ---------------------------------------------------------------- 3. the classes
def test_likelihood_classes():
    import henbun_amd as hb
    from henbun_amd import hip_ops as H

    L = hb.likelihoods
    liks = dict(laplace=L.Laplace(0.7), gamma=L.Gamma(2.5), exponential=L.Exponential(), negbin=L.NegativeBinomial(1.7),
                binomial=L.Binomial(12))
    assert [liks[k].lik_id for k in ("laplace", "gamma", "exponential", "negbin", "binomial")] == [16, 17, 17, 18, 19]
    assert (H.LIK_LAPLACE, H.LIK_GAMMA, H.LIK_NEGBINOMIAL, H.LIK_BINOMIAL) == Z.NEW == (16, 17, 18, 19)
    assert [liks[k].param for k in ("laplace", "gamma", "exponential", "negbin", "binomial")] == [0.7, 2.5, 1.0, 1.7, 12.0]
    trainable = dict(laplace=True, gamma=True, exponential=False, negbin=True, binomial=False)
    assert {k: v.trainable for k, v in liks.items()} == trainable
    assert L.Gaussian(0.3).trainable and not L.Bernoulli().trainable and not L.Poisson().trainable
    for make in (lambda: L.Laplace(0.0), lambda: L.Gamma(-1.0), lambda: L.NegativeBinomial(0.0), lambda: L.Binomial(0),
                 lambda: L.Binomial(2.5), lambda: L.Gaussian(0.0), lambda: L.Bernoulli().with_param(2.0),
                 lambda: L.Exponential().with_param(2.0), lambda: L.Laplace(0.7).with_param(-1.0)):
        with pytest.raises(ValueError):
            make()
    for lik in (L.Gaussian(0.3), liks["laplace"], liks["gamma"], liks["negbin"], liks["binomial"]):
        other = lik.with_param(3.0)
        assert other is not lik and type(other) is type(lik) and other.param == 3.0 and other.lik_id == lik.lik_id
        assert lik.param != 3.0


def test_learn_likelihood_needs_a_trainable_likelihood():
    """(raises in setUp, before any session exists: this runs without a device)"""
    import henbun_amd as hb
    from henbun_amd.models import SVGPLik

    X, y, Zi = SR.problem(SR.BERNOULLI, N=50, M=8)
    for lik in (hb.likelihoods.Bernoulli(), hb.likelihoods.Poisson(), hb.likelihoods.Binomial(3), hb.likelihoods.Exponential()):
        with pytest.raises(ValueError, match="learn_likelihood"):
            SVGPLik(X=X, Y=y, Z=Zi, likelihood=lik, learn_likelihood=True, dtype="float64")
    m = SVGPLik(X=X, Y=y, Z=Zi, likelihood=hb.likelihoods.Laplace(0.3), learn_likelihood=True, dtype="float64")
    assert list(m._hyper_variables()) == ["z", "lengthscales", "k_var", "lik_param"]
    m = SVGPLik(X=X, Y=y, Z=Zi, likelihood=hb.likelihoods.Laplace(0.3), dtype="float64")
    assert list(m._hyper_variables()) == ["z", "lengthscales", "k_var"] and not hasattr(m, "lik_param")


@pytest.mark.parametrize("as_tensor", [False, True])
def test_logp_graph_values_equal_the_restatement(as_tensor):
    """likelihood.logp(f, y) -- and logp(f, y, param=tensor) with ANOTHER value than the stored float -- evaluated on the
    CPU graph oracle (torch float64) against lik_zoo_ref.log_p: 1e-12 of the largest magnitude."""
    import henbun_amd as hb
    from henbun_amd import graph as G

    import graph_oracle

    L = hb.likelihoods
    rng = np.random.RandomState(3)
    f = rng.randn(1, 30) * 1.5
    cases = [(L.Gaussian(0.4), Z.GAUSSIAN, 0.4), (L.Laplace(0.7), Z.LAPLACE, 0.7), (L.Gamma(2.5), Z.GAMMA, 2.5),
             (L.Exponential(), Z.GAMMA, 1.0), (L.NegativeBinomial(1.7), Z.NEGBINOMIAL, 1.7), (L.Binomial(12), Z.BINOMIAL, 12.0),
             (L.Bernoulli(), Z.BERNOULLI, 1.0), (L.Poisson(), Z.POISSON, 1.0)]
    for lik, lid, p in cases:
        if as_tensor and not lik.trainable:
            continue
        y = Z.draw(lid, f, p, rng)
        use = 1.3 * p if as_tensor else p
        ft, yt = G.constant(f), G.constant(y)
        out = lik.logp(ft, yt, param=G.constant(np.ones(1) * use)) if as_tensor else lik.logp(ft, yt)
        got = graph_oracle.evaluate([out], {})[out].numpy()
        ref = Z.log_p(lid, y, f, use)
        assert got.shape == f.shape
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (type(lik).__name__, np.abs(got - ref).max())


# ---------------------------------------------------------------- 4. the iteration and the learning loop, in the restatement alone
@pytest.mark.parametrize("rho", [1.0, 0.5])
@pytest.mark.parametrize("lik", Z.NEW)
def test_iterations_the_gpu_test_follows_are_reproducible_in_the_restatement(lik, rho):
    """tests/test_lik_zoo_gpu.py holds natgrad_q to the restatement's 8-step traces at 1e-8.  That asks something only
    where the restatement itself is determined far better than that: a one-ulp change of every label must move its ELBO
    and residual traces by at most 1e-10.  It is why the Laplace case runs at scale 1 (lik_zoo_ref.NATGRAD_PARAM): at
    scale 0.3 the undamped iteration diverges and this figure is 9.5e-7 at rho = 1 (printed)."""
    p = Z.NATGRAD_PARAM[lik]
    X, y, Zi = Z.problem(lik, p)
    bump = 1.0 + np.finfo(np.float64).eps * np.sign(np.sin(np.arange(y.size)))[:, None]
    a = Z.natgrad(X, y, Zi, Z.ELL, Z.JITTER, lik, p, Z.K_VAR, steps=8, rho=rho, tol=0.0)[2]
    b = Z.natgrad(X, y * bump, Zi, Z.ELL, Z.JITTER, lik, p, Z.K_VAR, steps=8, rho=rho, tol=0.0)[2]
    n = min(len(a["elbo"]), len(b["elbo"]))
    d_elbo = np.abs(a["elbo"][:n] / b["elbo"][:n] - 1).max()
    d_res = np.abs(a["residual"][:n] - b["residual"][:n]).max()
    print("%s rho %.1f: one ulp on the labels moves the ELBO trace by %.1e, the residual trace by %.1e" % (Z.NAMES[lik], rho, d_elbo, d_res))
    assert n >= 8 and d_elbo <= 1e-10 and d_res <= 1e-10
    if lik == Z.LAPLACE and rho == 1.0:
        X, y, Zi = Z.problem(lik, 0.3)
        a = Z.natgrad(X, y, Zi, Z.ELL, Z.JITTER, lik, 0.3, Z.K_VAR, steps=8, rho=rho, tol=0.0)[2]
        b = Z.natgrad(X, y * bump, Zi, Z.ELL, Z.JITTER, lik, 0.3, Z.K_VAR, steps=8, rho=rho, tol=0.0)[2]
        print("laplace at scale 0.3, rho 1: ELBO %.3f -> %.3e; one ulp moves the residual trace by %.1e"
              % (a["elbo"][0], a["elbo"][-1], np.abs(a["residual"] - b["residual"]).max()))
        assert a["elbo"][-1] < a["elbo"][1]            # it diverges: the reason for likelihoods.Laplace.natgrad_rho



@pytest.mark.parametrize("lik", Z.TRAINABLE)
def test_learning_loop_in_the_restatement(lik):
    """The data and the settings of the GPU test (N = 3000, M = 32, theta* drawn, start 3 theta*, 30 steps at lr 0.05):
    natural-gradient steps alternated with Adam ascent on log theta by the restated gradient.  The final ELBO exceeds
    the initial one and theta ends closer to theta* (in log) than it started: the GPU test's conditions are attainable."""
    star = Z.THETA_STAR[lik]
    X, y, Zi = Z.problem(lik, star)
    thetas, elbos = Z.learn(X, y, Zi, Z.ELL, Z.JITTER, lik, 3.0 * star, Z.K_VAR, rho=Z.RHO.get(lik, 1.0))
    print("%s: theta %.4f -> %.4f (theta* %.4f), ELBO %.3f -> %.3f" % (Z.NAMES[lik], thetas[0], thetas[-1], star, elbos[0], elbos[-1]))
    assert elbos[-1] > elbos[0]
    assert abs(math.log(thetas[-1] / star)) < abs(math.log(thetas[0] / star))
