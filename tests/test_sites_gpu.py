"""Natural-gradient fit of q(u) for non-conjugate likelihoods on the GPU, against the numpy restatement tests/sites_ref.py
(itself pinned on the host by tests/test_sites_cpu.py).

fp64 bounds are fixed (1e-10 of max|Phi| for the statistics, 1e-12 for the sites, 1e-8 end to end).  fp32 bounds are not
constants: the statistics and the end-to-end prediction are held to 4 x the error the float32 restatement makes against
float64 on the same inputs (as tests/test_optimal_q_gpu.py does); the sites compute in double whatever the storage type
and are held to 2 float32 ulps of the reference value.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd import graph as G
from henbun_amd import hip_ops as H
from henbun_amd.models import SVGP, SVGPLik
from henbun_amd.param import tri_pack

import optimal_q_ref as R
import sites_ref as SR
from parity import tile_err

pytestmark = pytest.mark.gpu
tf = hb.tf

KSPLIT = 432          # columns per float32 block of the restatement (tests/test_optimal_q_gpu.py)
FMAX = float(np.finfo(np.float32).max)


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


# ------------------------------------------------------------------------------------------------ 1. hb_sgp_wstats
@pytest.mark.parametrize("M", [32, 160])
@pytest.mark.parametrize("N", [1, 97, 4096, 40001])
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_sgp_wstats_against_the_restatement(dtype, d, N, M):
    """hb_sgp_wstats_f64 / _f32 with a mixed-sign w that holds exact zeros: Phi_w, b, tr; Phi_w bitwise symmetric; two
    runs bitwise equal; with w == 1 and r = Y[:, 0] the bits of hb_sgp_stats.  N crosses a chunk (32768) and K-split
    boundaries and leaves ragged tails; M = 32 uses part of one tile, 160 three tiles (one off the diagonal, ragged rows).
    Observed on MI355X: see DESIGN.md 3, "Natural-gradient fit"."""
    dt = torch.float64 if dtype == "float64" else torch.float32
    npdt = np.float64 if dtype == "float64" else np.float32
    X, w, r, Y, z, ell, W = (a.astype(npdt) for a in SR.stats_case(N, M, d, seed=N + M + d))
    Xd, wd, rd, Yd, zd, elld, Wd = (dev(a, dt) for a in (X, w, r, Y, z, ell, W))
    out = H.sgp_wstats(Xd, wd, rd, zd, elld, Wd)
    out2 = H.sgp_wstats(Xd, wd, rd, zd, elld, Wd)
    one = H.sgp_wstats(Xd, torch.ones_like(wd), Yd[:, 0].contiguous(), zd, elld, Wd)
    plain = H.sgp_stats(Xd, Yd, zd, elld, Wd)
    torch.cuda.synchronize()
    for a, c in zip(out, out2):
        assert a.dtype == torch.float64 and torch.equal(a, c)
    assert torch.equal(one[0], plain[0]) and torch.equal(one[1], plain[1]) and torch.equal(one[2], plain[3])
    Phi, b, tr = (o.cpu().numpy() for o in out)
    assert Phi.shape == (M, M) and b.shape == (1, M) and tr.shape == (1,)
    assert np.array_equal(Phi, Phi.T)
    assert tr[0] == pytest.approx(np.trace(Phi), rel=1e-12, abs=1e-12 * np.abs(np.diag(Phi)).sum())
    rPhi, rb, _ = SR.wstats_from_W(X, w, r, z, ell, W)         # float64 arithmetic on the SAME (already rounded) inputs
    sc, scb = np.abs(rPhi).max(), np.abs(rb).max()
    ePhi, eb = np.abs(Phi - rPhi), np.abs(b - rb)
    print("sgp_wstats %s N=%d M=%d d=%d: dPhi/max|Phi|=%.3e db/max|b|=%.3e" % (dtype, N, M, d, ePhi.max() / sc, eb.max() / scb))
    if dtype == "float64":
        assert ePhi.max() <= 1e-10 * sc
        assert eb.max() <= 1e-10 * scb
        return
    qPhi, qb, _ = SR.wstats_from_W(X, w, r, z, ell, W, dtype=np.float32, ksplit=KSPLIT)
    gotPhi, refPhi = tile_err(Phi, rPhi), tile_err(qPhi, rPhi)
    gotb, refb = tile_err(b, rb), tile_err(qb, rb)
    print("   fp32 worst tile: Phi device %.3e, restatement %.3e (%.2f x); b %.3e vs %.3e (%.2f x)"
          % (gotPhi, refPhi, gotPhi / refPhi, gotb, refb, gotb / refb))
    assert gotPhi <= 4.0 * refPhi
    assert gotb <= 4.0 * refb


# ------------------------------------------------------------------------------------------------ 2. the sites
def _site_inputs(lik, N, seed):
    """mu, v with the corners mu = +-30, v in {1e-12, 25} in front (as many as fit), Poisson y up to 1000."""
    rng = np.random.RandomState(seed)
    mu, v = 2.0 * rng.randn(N), np.exp(rng.uniform(-6, 1, N))
    corners = [(30.0, 25.0), (-30.0, 1e-12), (30.0, 1e-12), (-30.0, 25.0)][:N]
    for i, (a, c) in enumerate(corners):
        mu[i], v[i] = a, c
    if lik == SR.BERNOULLI:
        y = (rng.uniform(size=N) < 0.5).astype(np.float64)
    elif lik == SR.POISSON:
        y = rng.poisson(np.exp(np.clip(mu, -3, 3))).astype(np.float64)
        y[-1] = 1000.0
    else:
        y = mu + rng.randn(N)
    return y, mu, v


def _ulps32(got, ref):
    """|got - ref| in units of the float32 spacing at ref (ref saturated to the float32 range, as the kernel does)."""
    ref = np.clip(ref, -FMAX, FMAX)
    a32 = np.maximum(np.abs(ref.astype(np.float32)), np.finfo(np.float32).tiny)
    with np.errstate(over="ignore"):
        up = np.nextafter(a32, np.float32(np.inf)) - a32
    ulp = np.where(np.isfinite(up), up, a32 - np.nextafter(a32, np.float32(0)))
    return np.abs(got.astype(np.float64) - ref) / ulp.astype(np.float64)


@pytest.mark.parametrize("N", [1, 255, 1500])
@pytest.mark.parametrize("lik", [SR.GAUSSIAN, SR.BERNOULLI, SR.POISSON])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_lik_sites_and_predict_against_the_restatement(dtype, lik, N):
    """hb_lik_sites / hb_lik_predict: one element, one block minus one, several blocks with a ragged tail; the corners
    mu = +-30, v in {1e-12, 25}; Poisson y up to 1000.  Everything finite; two runs of the sum bitwise equal.
    float64 storage: 1e-12 relative per element -- beta = g + lam mu is measured against |g| + |lam mu|, the size of
    the terms it is the sum of (the two cancel where the site's pseudo-observation crosses zero), and sum_j l_j against
    sum_j |l_j|.  float32 storage: 2 float32 ulps of the reference value (double arithmetic, one rounding on output;
    the Poisson predictive variance at mu = 30, v = 25 is 6e47 and saturates to the largest float)."""
    dt = torch.float64 if dtype == "float64" else torch.float32
    npdt = np.float64 if dtype == "float64" else np.float32
    param, ms, vs = 0.7, 1.25, 0.8
    y, mu, v = (a.astype(npdt) for a in _site_inputs(lik, N, seed=7 * N + lik))
    yd, mud, vd = dev(y, dt), dev(mu, dt), dev(v, dt)
    lam, beta, lsum = H.lik_sites(lik, yd, mud, vd, param=param, mscale=ms, vscale=vs)
    _, _, lsum2 = H.lik_sites(lik, yd, mud, vd, param=param, mscale=ms, vscale=vs)
    ym, yv = H.lik_predict(lik, mud, vd, param=param)
    torch.cuda.synchronize()
    assert torch.equal(lsum, lsum2) and lsum.dtype == torch.float64
    lam, beta, ym, yv = (t.cpu().numpy() for t in (lam, beta, ym, yv))
    lsum = float(lsum.cpu()[0])
    m64, v64 = ms * mu.astype(np.float64), vs * v.astype(np.float64)
    rl, rlam, rbeta, rg = SR.sites(lik, y, m64, v64, param)
    rym, ryv = SR.predict_y(lik, mu.astype(np.float64), v.astype(np.float64), param)
    assert all(np.all(np.isfinite(a)) for a in (lam, beta, ym, yv)) and np.isfinite(lsum)
    e_sum = abs(lsum - rl.sum()) / np.abs(rl).sum()
    if dtype == "float64":
        e_lam = np.abs(lam / rlam - 1).max()
        e_beta = (np.abs(beta - rbeta) / (np.abs(rg) + np.abs(rlam * m64))).max()
        e_ym, e_yv = np.abs(ym / rym - 1).max(), np.abs(yv / ryv - 1).max()
        print("lik %d float64 N=%d: lam %.2e beta %.2e sum %.2e; predict mean %.2e var %.2e" % (lik, N, e_lam, e_beta, e_sum, e_ym, e_yv))
        assert max(e_lam, e_beta, e_sum, e_ym, e_yv) <= 1e-12
        return
    u = [float(_ulps32(a, b).max()) for a, b in ((lam, rlam), (beta, rbeta), (ym, rym), (yv, ryv))]
    print("lik %d float32 N=%d: ulps lam %.2f beta %.2f predict mean %.2f var %.2f; sum %.2e" % (lik, N, *u, e_sum))
    assert max(u) <= 2.0
    assert e_sum <= 1e-12


# ------------------------------------------------------------------------------------------------ 3. natgrad_q, fp64
LIKS = {SR.BERNOULLI: hb.likelihoods.Bernoulli, SR.POISSON: hb.likelihoods.Poisson}


def _model(lik, dtype, residual="diagonal", likelihood=None):
    X, y, Z = SR.problem(lik)
    m = SVGPLik(X=X, Y=y, Z=Z, likelihood=likelihood or LIKS[lik](), residual=residual, dtype=dtype)
    m.gp.kern.lengthscales = SR.ELL.copy()
    m.k_var = np.ones(1) * SR.K_VAR
    m.initialize()
    return m, X, y, Z


_REF = {}


def _ref(lik, rho, steps=8):
    """The float64 restatement, computed once per (likelihood, rho) and shared."""
    key = (lik, rho, steps)
    if key not in _REF:
        X, y, Z = SR.problem(lik)
        _REF[key] = SR.natgrad(X, y, Z, SR.ELL, hb.settings.numerics.jitter_level, lik, 1.0, SR.K_VAR, steps=steps, rho=rho,
                               tol=0.0)
    return _REF[key]


@pytest.mark.parametrize("rho", [1.0, 0.5])
@pytest.mark.parametrize("lik", [SR.BERNOULLI, SR.POISSON])
def test_natgrad_q_fp64_follows_the_restatement(lik, rho):
    """8 steps from the prior in a float64 session: the ELBO trace to 1e-8 relative, the residual trace to 1e-8 (it is
    already relative to max|Lambda~|, and at the fixed point it IS round-off: 5e-9 on the host), m and S S^T to 1e-8 of
    their largest entry.  rho = 1: the ELBO never decreases beyond the round-off of a sum of N terms (N eps |ELBO|), and
    the final residual is <= 1e-6.  Observed on MI355X: see DESIGN.md 3, "Natural-gradient fit"."""
    assert hb.settings.numerics.jitter_level == SR.JITTER
    m, X, y, Z = _model(lik, "float64")
    qm, S, info = m.gp.natgrad_q(X, y, LIKS[lik](), k_var=SR.K_VAR, steps=8, rho=rho, tol=0.0)
    rm, rS, rinfo = _ref(lik, rho)
    assert info["steps"] == 8 and len(info["elbo"]) == 9 and len(info["residual"]) == 9
    assert qm.shape == (1, 32) and S.shape == (32, 32) and np.array_equal(S, np.tril(S)) and np.all(np.diag(S) > 0)
    e_elbo = np.abs(info["elbo"] / rinfo["elbo"] - 1).max()
    e_res = np.abs(info["residual"] - rinfo["residual"]).max()
    e_m = np.abs(qm - rm).max() / np.abs(rm).max()
    e_S = np.abs(S @ S.T - rS @ rS.T).max() / np.abs(rS @ rS.T).max()
    print("natgrad_q fp64 lik %d rho %.1f: elbo %.3f -> %.3f (rel err %.2e), residual -> %.2e (err %.2e), m %.2e S S^T %.2e"
          % (lik, rho, info["elbo"][0], info["elbo"][-1], e_elbo, info["residual"][-1], e_res, e_m, e_S))
    assert e_elbo <= 1e-8 and e_res <= 1e-8 and e_m <= 1e-8 and e_S <= 1e-8
    if rho == 1.0:
        assert np.all(np.diff(info["elbo"]) >= -X.shape[0] * np.finfo(np.float64).eps * np.abs(info["elbo"][-1]))
        assert info["residual"][-1] <= 1e-6
    # a Data of the model and a start from a given q: the restatement's 4th iterate, continued for 4 steps
    m4, S4, _ = _ref(lik, rho, steps=4)
    _, _, info2 = m.gp.natgrad_q(object.__getattribute__(m, "X"), object.__getattribute__(m, "Y"), LIKS[lik](),
                                 k_var=SR.K_VAR, q0=(m4, S4), steps=4, rho=rho, tol=0.0)
    assert np.abs(info2["elbo"] / rinfo["elbo"][4:] - 1).max() <= 1e-8


def test_gaussian_step_is_the_devices_own_optimal_q():
    """One step at rho = 1 from the prior with the Gaussian likelihood against SparseGP.optimal_q / collapsed_bound of
    the same session: 1e-10."""
    X, y, Z = SR.problem(SR.GAUSSIAN)
    m = SVGP(X=X, Y=y, Z=Z, q_shape="fullrank", dtype="float64")
    m.gp.kern.lengthscales = SR.ELL.copy()
    m.initialize()
    qm, S, info = m.gp.natgrad_q(X, y, hb.likelihoods.Gaussian(0.4), k_var=SR.K_VAR, steps=1, tol=0.0)
    om, oS = m.gp.optimal_q(X, y, 0.4, SR.K_VAR)
    bound = m.gp.collapsed_bound(X, y, 0.4, SR.K_VAR)
    e_m, e_S = np.abs(qm - om).max() / np.abs(om).max(), np.abs(S @ S.T - oS @ oS.T).max() / np.abs(oS @ oS.T).max()
    print("Gaussian step: m %.2e S S^T %.2e elbo %.9f bound %.9f residual %.2e" % (e_m, e_S, info["elbo"][1], bound, info["residual"][1]))
    assert e_m <= 1e-10 and e_S <= 1e-10
    assert abs(info["elbo"][1] - bound) <= 1e-10 * abs(bound)


# ------------------------------------------------------------------------------------------------ 4. fp32 session
def _model_factor(Z, ell, jitter):
    """W in float32 as the model's own factor + inverse launches produce it (tests/test_optimal_q_gpu.py)."""
    z = dev(Z, torch.float32)
    _, W, info = H.cholesky_inverse(H.gram_fwd(z, z, dev(ell, torch.float32), diag_add=float(jitter)))
    assert int(info.cpu()[0]) == 0
    return W.cpu().numpy()


@pytest.mark.parametrize("lik", [SR.BERNOULLI, SR.POISSON])
def test_natgrad_q_fp32_session_predicts_within_the_float32_restatements_error(lik):
    """fit_q in a float32 session, then predict_f at X, against the float64 restatement; bound: 4 x the error of the
    float32 restatement (float32 A, marginals and weighted products, lam and beta rounded to float32, float64 tail) on
    the model's own float32 W.
    Observed on MI355X (8 steps from the prior): Bernoulli mean 1.13e-5 against the restatement's 6.75e-6 (1.7 x), var
    2.41e-6 against 2.05e-6 (1.2 x); Poisson mean 1.11e-5 against 1.12e-5 (1.0 x), var 2.46e-6 against 2.09e-6 (1.2 x);
    the ELBO agrees with float64 to 7 digits (-1749.847, -4416.938).
    The test holds only because natgrad_q whitens with z and the lengthscales as the plans transform them on the
    device.  With the host's transform (double, then rounded) the lengthscale 0.9 differed from the plan's softplus in
    its last float32 bit (0x3f666666 against 0x3f666667); W then differs by cond(K(z, z)) times that (|dW| ~ 0.09), q(u)
    was fitted in one whitening and read by predict_f in the other, and the mean erred by 8.83e-5 (13 x) and 1.13e-4
    (10 x), the variance by 5.04e-6 (2.5 x) and 4.30e-6 (2.1 x).  The numpy restatement with a lengthscale one ulp apart
    between fit and prediction reproduces that: 8.3e-5 against 5.3e-6."""
    jitter = hb.settings.numerics.jitter_level
    m, X, y, Z = _model(lik, "float32")
    q, sess = object.__getattribute__(m, "u"), m._session
    sess.write_raw(object.__getattribute__(q, "q_mu"), np.zeros(32))           # fit_q starts at the model's q: the prior,
    sess.write_raw(object.__getattribute__(q, "q_sqrt"), tri_pack(np.eye(32)) if q.packed else np.eye(32))   # as the restatement
    qm, S, info = m.fit_q(steps=8, tol=0.0)
    mu32, v32 = m.predict_f(X)
    rm, rS, _ = _ref(lik, 1.0)
    rmu, rv = R.predict(X, Z, SR.ELL, jitter, rm, rS, SR.K_VAR)
    W32 = _model_factor(Z, SR.ELL, jitter)
    fm, fS, _ = SR.natgrad(X.astype(np.float32), y, Z.astype(np.float32), SR.ELL.astype(np.float32), jitter, lik, 1.0, SR.K_VAR,
                           steps=8, tol=0.0, dtype=np.float32, W=W32, ksplit=KSPLIT)
    A32 = R.A_of(W32, Z.astype(np.float32), X.astype(np.float32), SR.ELL.astype(np.float32))
    qmu, qv = SR.marginals(fm, fS, A32, SR.K_VAR)
    b_mu, b_v = np.abs(qmu - rmu).max(), np.abs(qv - rv).max()
    g_mu, g_v = np.abs(mu32 - rmu).max(), np.abs(v32 - rv).max()
    print("natgrad_q fp32 lik %d: predict_f mean %.3e (float32 restatement %.3e) var %.3e (%.3e); elbo %.3f (fp64 %.3f)"
          % (lik, g_mu, b_mu, g_v, b_v, info["elbo"][-1], _ref(lik, 1.0)[2]["elbo"][-1]))
    assert g_mu <= 4.0 * b_mu
    assert g_v <= 4.0 * b_v


# ------------------------------------------------------------------------------------------------ 5. the model
def _grad_plan(m):
    """(plan, objective, d objective / d q_mu) of the model's own ELBO on ALL rows (tests/test_optimal_q_gpu.py)."""
    opt = m.ELBO()
    opt._ensure_compiled()
    m.initialize()
    obj = opt._trace(None)
    q = object.__getattribute__(m, "u")
    grads = G.gradients(obj, [object.__getattribute__(q, "q_mu")._leaf])
    return m._session.make_plan([obj] + grads, minibatch=None), obj, grads


@pytest.mark.parametrize("lik", [SR.BERNOULLI, SR.POISSON])
def test_svgplik_fit_q_zeroes_the_gradient_of_the_sampled_elbo(lik):
    """After SVGPLik.fit_q() the Monte-Carlo gradient of the model's sampled ELBO (all rows, analytic KL, 128 draws) with
    respect to q_mu is zero within 4 standard errors for >= 99 % of the entries (the initial q's share is printed); the
    Monte-Carlo ELBO equals info['elbo'][-1] within 4 standard errors; predict_y is the restatement's predictive of
    predict_f (1e-12)."""
    K = 128
    cfg = hb.settings.get_settings()
    cfg.numerics.kl_form = "analytic"
    with hb.settings.temp_settings(cfg):
        m, X, y, Z = _model(lik, "float64")
        plan, obj, grads = _grad_plan(m)

        def draws():
            g, o = [], []
            for _ in range(K):
                plan.run()
                plan.check()
                g.append(plan.value(grads[0]).astype(np.float64).reshape(-1))
                o.append(float(np.ravel(plan.value(obj))[0]))
            g, o = np.stack(g), np.asarray(o)
            return g.mean(0), g.std(0, ddof=1) / np.sqrt(K), o.mean(), o.std(ddof=1) / np.sqrt(K)

        g0, se0, _, _ = draws()
        # fit_q starts at the model's q.  A full step (rho = 1) from the RANDOM initial q overshoots (observed: the ELBO
        # falls to -4.7e5 for Bernoulli, exp overflows for Poisson), so the fit starts at the prior, as the restatement does
        q, sess = object.__getattribute__(m, "u"), m._session
        sess.write_raw(object.__getattribute__(q, "q_mu"), np.zeros(32))
        sess.write_raw(object.__getattribute__(q, "q_sqrt"), tri_pack(np.eye(32)) if q.packed else np.eye(32))
        qm, S, info = m.fit_q()
        g1, se1, e1, see1 = draws()
        frac0, frac1 = np.mean(np.abs(g0) <= 4 * se0), np.mean(np.abs(g1) <= 4 * se1)
        print("lik %d: d ELBO / d q_mu within 4 s.e.: initial q %.0f %% (max %.1f s.e.), after fit_q (%d steps) %.0f %% (max "
              "%.2f); Monte-Carlo ELBO %.3f +- %.3f, info %.3f"
              % (lik, 100 * frac0, np.max(np.abs(g0) / se0), info["steps"], 100 * frac1, np.max(np.abs(g1) / se1), e1, see1,
                 info["elbo"][-1]))
        assert np.all(se1 > 0) and see1 > 0
        assert frac1 >= 0.99
        assert abs(e1 - info["elbo"][-1]) <= 4.0 * see1
        q = object.__getattribute__(m, "u")
        assert np.allclose(q.q_mu.value.reshape(1, -1), qm, rtol=0, atol=1e-14)
        assert np.allclose(np.tril(q.q_sqrt.value), S, rtol=0, atol=1e-14)
        xs = np.linspace(-1.0, 17.0, 200)[:, None]
        mu, v = m.predict_f(xs)
        ym, yv = m.predict_y(xs)
        rym, ryv = SR.predict_y(lik, mu, v)
        assert ym.shape == mu.shape and np.abs(ym / rym - 1).max() <= 1e-12 and np.abs(yv / ryv - 1).max() <= 1e-12
        rmu, rv = R.predict(xs, Z, SR.ELL, hb.settings.numerics.jitter_level, qm, S, SR.K_VAR)
        assert np.abs(mu - rmu).max() <= 1e-8 and np.abs(v - rv).max() <= 1e-8


def test_natgrad_q_refuses_what_it_does_not_cover():
    m, X, y, Z = _model(SR.BERNOULLI, "float64")
    lik = hb.likelihoods.Bernoulli()
    with pytest.raises(NotImplementedError, match="fullrank"):
        m.gp.natgrad_q(X, y, lik, residual="fullrank")
    with pytest.raises(NotImplementedError, match="mean-field"):
        m.gp.natgrad_q(X, y, lik, q0=(np.zeros((1, 32)), np.ones(32)))
    with pytest.raises(NotImplementedError, match="one latent function"):
        m.gp.natgrad_q(X, np.concatenate([y, y], 1), lik)
    with pytest.raises(TypeError):
        m.gp.natgrad_q(X, y, "bernoulli")
    S0 = np.eye(32)
    S0[3, 3] = 0.0
    with pytest.raises(G.CholeskyError):
        m.gp.natgrad_q(X, y, lik, q0=(np.zeros((1, 32)), S0))

    class Other(hb.model.Model):
        def setUp(self, Z, kern):
            self.gp = hb.gp.SparseGP(kern=kern, z=Z)

    with pytest.raises(NotImplementedError, match="UnitRBF"):
        Other(Z=Z, kern=hb.gp.kernels.UnitMatern52(np.ones(1)), dtype="float64").gp.natgrad_q(X, y, lik)
    with pytest.raises(NotImplementedError, match="one expert"):
        Other(Z=np.stack([Z, Z]), kern=hb.gp.kernels.UnitRBF(np.ones((2, 1))), dtype="float64").gp.natgrad_q(X, y, lik)
