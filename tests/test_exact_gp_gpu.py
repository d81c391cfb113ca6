"""Exact GP regression by conjugate gradients on the GPU (GP.condition, ExactPosterior, ExactGPR), against the dense
float64 posterior and the numpy restatement tests/exact_gp_ref.py (pinned on the host by tests/test_exact_gp_cpu.py).

The case is the one the preconditioner's effect was measured on: X ~ U(0, 5)^2, N = 600, ell = 0.5, noise_var = 0.01,
k_var = 1, Y = sin(sum x) + 0.1 noise; cond(K^) = 4e3, |K^^-1| = 100.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd.models import ExactGPR, svgp_data

import exact_gp_ref as E

pytestmark = pytest.mark.gpu

_MODEL, _POST, _DENSE = {}, {}, {}


def _model(dtype):
    if dtype not in _MODEL:
        X, Y, ell, k_var, noise_var = E.plane_case()
        m = ExactGPR(X=X, Y=Y, dtype=dtype)
        m.gp.kern.lengthscales = ell.copy()
        m.k_var = np.ones(1) * k_var
        m.var = np.ones(1) * noise_var
        m.initialize()
        _MODEL[dtype] = m
    return _MODEL[dtype]


def _posterior(dtype, rank=64):
    """GP.condition on the case, once per (dtype, rank), at the default tolerance of the dtype."""
    if (dtype, rank) not in _POST:
        m = _model(dtype)
        g = lambda k: object.__getattribute__(m, k)
        _POST[(dtype, rank)] = g("gp").condition(g("X"), g("Y"), 0.01, k_var=1.0, precond_rank=rank)
    return _POST[(dtype, rank)]


def _dense():
    """(X, Y, ell, Xnew [150, 2], alpha, mean, var, |K^^-1|, |k*_j|, |y|) in float64 from the dense Cholesky, once."""
    if not _DENSE:
        X, Y, ell, k_var, noise_var = E.plane_case()
        Xnew = np.random.default_rng(5).uniform(-0.5, 5.5, (150, 2))
        alpha, mean, var = E.posterior(X, Y, ell, k_var, noise_var, Xnew)
        inv_norm = 1.0 / np.linalg.eigvalsh(E.dense(X, ell, k_var, noise_var))[0]
        ks = np.linalg.norm(k_var * E.rbf(X, Xnew, ell), axis=0)
        _DENSE["v"] = (X, Y, ell, Xnew, alpha, mean, var, inv_norm, ks, float(np.linalg.norm(Y)))
    return _DENSE["v"]


def test_float64_solve_against_the_dense_cholesky():
    """alpha within 1e-5 of max|alpha|, the true residual at most 1e-6, and the iterations fall with the rank as they do
    in the restatement (223 / 56 / 15 there): rank 64 at most half of plain CG, rank 128 no more than rank 64."""
    alpha_ref = _dense()[4]
    it = {}
    for rank in (0, 64, 128):
        post = _posterior("float64", rank)
        info = post.info
        err = np.abs(post.alpha - alpha_ref).max() / np.abs(alpha_ref).max()
        it[rank] = info["iterations"]
        print("float64 rank %d (used %d): %d iterations, residual %.3e, alpha error %.3e of max|alpha|"
              % (rank, info["precond_rank"], info["iterations"], info["residual"][0], err))
        assert info["converged"] and info["precond_rank"] == rank and info["residual"].shape == (1,)
        assert info["residual"][0] <= 1e-6 and err <= 1e-5
    assert it[64] <= it[0] / 2 and it[128] <= it[64]


def test_float32_solve_converges_at_1e_3():
    post = _posterior("float32")
    info = post.info
    alpha_ref = _dense()[4]
    print("float32 rank 64, tol 1e-3: %d iterations, %d restarts, residual %.3e, alpha error %.3e of max|alpha|"
          % (info["iterations"], info["restarts"], info["residual"][0], np.abs(post.alpha - alpha_ref).max() / np.abs(alpha_ref).max()))
    assert info["converged"] and post.tol == 1e-3 and post.alpha.dtype == np.float32
    assert info["residual"][0] <= 1e-3


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_predict_f_against_the_dense_posterior(dtype):
    """150 test points: three variance blocks, the last of 22.  float64: mean and variance within 1e-5 (absolute).
    float32: mean and variance within tol |k*_j| |K^^-1|, evaluated from the dense matrices.  (A solve with right-hand
    side b leaves |b - K^ x| <= tol |b|, so k*^T x is off by at most tol |k*| |K^^-1| |b|, b = y for the mean and k* for
    the variance; |y| = 18 and |k*| <= 5.2 here, so the bound asserted is the tighter one, without |b|.)"""
    X, Y, ell, Xnew, alpha, mean, var, inv_norm, ks, ynorm = _dense()
    post = _posterior(dtype)
    m, v = post.predict_f(Xnew)
    m_only, none = post.predict_f(Xnew, var=False)
    my, vy = post.predict_y(Xnew)
    assert m.shape == (1, 150) and v.shape == (150,) and none is None
    assert np.array_equal(m, m_only) and np.array_equal(my, m)
    em, ev = np.abs(m - mean)[0], np.abs(v - var)
    if dtype == "float64":
        bm = bv = np.full(150, 1e-5)
    else:
        bm = bv = post.tol * ks * inv_norm
    print("%s predict_f: mean error %.3e (%.3e of its bound), variance error %.3e (%.3e of its bound); var in [%.3g, %.3g]"
          % (dtype, em.max(), (em / bm).max(), ev.max(), (ev / bv).max(), var.min(), var.max()))
    assert np.all(em <= bm) and np.all(ev <= bv)
    assert np.abs(vy - v - 0.01).max() <= 1e-6


def test_sample_function_coefficients_against_the_restatement():
    """Injected omega, w, eps (float64): coef = [w / sqrt(L) | v] with v within 1e-5 of max|v| of the dense solve (the
    solves stop at 1e-6, as alpha's does), S = 70 draws: two blocks of lockstep solves.  Two evaluations are bitwise equal,
    and pieces of X carry the bits of the whole."""
    X, Y, ell = _dense()[:3]
    post = _posterior("float64")
    rng = np.random.default_rng(7)
    S, L, N = 70, 64, X.shape[0]
    noise = dict(omega=rng.standard_normal((L, 2)), w=rng.standard_normal((S, 2 * L)), eps=rng.standard_normal((S, N)))
    draws = post.sample_functions(S, num_features=L, noise=noise)
    Kh = E.dense(X, ell, 1.0, 0.01)
    ref = E.pathwise_coefficients(X, Y[:, 0], ell, 1.0, 0.01, noise["omega"], noise["w"], noise["eps"],
                                  lambda B: np.linalg.solve(Kh, B.T).T)
    coef = draws.coef
    ew = np.abs(coef[:, :2 * L] - ref[:, :2 * L]).max()
    ev = np.abs(coef[:, 2 * L:] - ref[:, 2 * L:]).max() / np.abs(ref[:, 2 * L:]).max()
    print("exact pathwise coefficients: w part %.3e, v part %.3e of max|v| = %.3g" % (ew, ev, np.abs(ref[:, 2 * L:]).max()))
    assert coef.shape == (S, 2 * L + N) and draws.num_samples == S and draws.scale == 1.0
    assert ew <= 1e-15 and ev <= 1e-5
    xs = np.random.default_rng(8).uniform(0, 5, (200, 2))
    a, b = draws(xs), draws(xs)
    assert np.array_equal(a, b)
    assert np.array_equal(np.concatenate([draws(xs[:77]), draws(xs[77:])], axis=1), a)
    for bad in (dict(omega=noise["omega"], w=noise["w"]), dict(noise, eps=noise["eps"][:, 1:])):
        with pytest.raises(ValueError, match="noise"):
            post.sample_functions(S, num_features=L, noise=bad)


def test_device_rng_draws_have_the_posterior_moments():
    """S = 512 draws with L = 1024 features at 16 points, float64: 12 among the data (v_j about 1e-2) and 4 well outside
    them, where v_j is the prior's k_var = 1 and the bound below has power -- draws without variance would miss it.  The
    mean of a draw is the posterior mean whatever the frequencies; its variance is the posterior variance v_j up to the
    random-feature error of the prior covariance, at most 8 k_var / sqrt(L) (tests/test_pathwise_cpu.py).  With
    u_j = v_j + 8 / sqrt(L): the sample mean within 6 sqrt(u_j / S) + 1e-5 of the mean, the sample variance within
    6 u_j sqrt(2 / (S - 1)) + 8 / sqrt(L) of v_j."""
    post = _posterior("float64")
    S, L = 512, 1024
    x = np.concatenate([np.random.default_rng(9).uniform(0.0, 5.0, (12, 2)), np.array([[9.0, 9.0], [-4.0, 2.0], [2.0, 11.0], [12.0, -3.0]])])
    mean, v = post.predict_f(x)
    assert np.all(v[12:] > 0.999)
    draws = post.sample_functions(S, num_features=L, seed=3)
    f = draws(x)
    bias = 8.0 / np.sqrt(L)
    u = v + bias
    em = np.abs(f.mean(0) - mean[0]) / (6.0 * np.sqrt(u / S) + 1e-5)
    ev = np.abs(f.var(0, ddof=1) - v) / (6.0 * u * np.sqrt(2.0 / (S - 1)) + bias)
    print("device RNG: sample mean at %.2f of its bound, sample variance at %.2f; v in [%.3g, %.3g], sample variance in "
          "[%.3g, %.3g]" % (em.max(), ev.max(), v.min(), v.max(), f.var(0, ddof=1).min(), f.var(0, ddof=1).max()))
    assert f.shape == (S, 16) and em.max() <= 1.0 and ev.max() <= 1.0
    again = post.sample_functions(S, num_features=L, seed=3)
    assert np.array_equal(again.coef, draws.coef) and np.array_equal(again(x), f)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_one_step_of_the_iteration_against_the_restatement(dtype):
    """hb_pcg_dot, hb_pcg_update and hb_pcg_direction on random vectors [4, 3001] with row 1 converged (rr <= thr: both
    steps must leave it alone), with and without the preconditioner's w, first and later steps.  The scalars are double:
    alpha, beta, rz, rr within 1e-12 relative (float64) of numpy on the same inputs; the vectors to the rounding of their
    dtype, 4 ulps of max|.|."""
    from henbun_amd import hip_ops as H

    dt, npdt = (torch.float64, np.float64) if dtype == "float64" else (torch.float32, np.float32)
    rng = np.random.default_rng(11)
    S, N = 4, 3001
    x, r, p, Ap, w = (rng.standard_normal((S, N)).astype(npdt) for _ in range(5))
    Ap = (Ap + 3.0 * p).astype(npdt)                       # p . Ap > 0
    rz, thr = rng.uniform(1.0, 2.0, S), np.full(S, 10.0)
    rr = (r.astype(np.float64) ** 2).sum(1)
    thr[1] = 2.0 * rr[1]
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    f64 = lambda a: a.astype(np.float64)
    ulp = 4.0 * np.finfo(npdt).eps
    dot = H.pcg_dot(up(p), up(Ap)).cpu().numpy()
    assert np.abs(dot - (f64(p) * f64(Ap)).sum(1)).max() <= 1e-12 * (np.abs(f64(p)) * np.abs(f64(Ap))).sum(1).max()
    xd, rd, rrd = up(x), up(r), up(rr)
    H.pcg_update(xd, rd, up(p), up(Ap), up(rz), rrd, up(thr))
    xr, rref, rrr = E.pcg_update(f64(x), f64(r), f64(p), f64(Ap), rz, rr, thr)
    gx, gr, grr = xd.cpu().numpy(), rd.cpu().numpy(), rrd.cpu().numpy()
    print("%s update: x %.2e, r %.2e, rr %.2e" % (dtype, np.abs(gx - xr).max(), np.abs(gr - rref).max(), np.abs(grr / rrr - 1).max()))
    assert np.array_equal(gx[1], x[1]) and np.array_equal(gr[1], r[1]) and grr[1] == rr[1]
    assert np.abs(gx - xr).max() <= ulp * np.abs(xr).max() and np.abs(gr - rref).max() <= ulp * np.abs(rref).max()
    assert np.abs(grr / rrr - 1).max() <= (1e-12 if dtype == "float64" else 8 * ulp)   # rr is |r|^2 of the ROUNDED r
    for wv, first in ((None, True), (w, False), (w, True), (None, False)):
        pd, rzd = up(p), up(rz)
        H.pcg_direction(up(r), None if wv is None else up(wv), pd, rzd, up(rr), up(thr), wscale=1.3, zscale=0.7, first=first)
        pr, rzr = E.pcg_direction(f64(r), None if wv is None else f64(wv), f64(p), rz, rr, thr, 1.3, 0.7, first)
        gp, grz = pd.cpu().numpy(), rzd.cpu().numpy()
        assert np.array_equal(gp[1], p[1]) and grz[1] == rz[1]
        mag = (np.abs(f64(r)) * (np.abs(f64(r)) + 1.3 * np.abs(f64(w)))).sum(1).max()      # sum_i |r_i| |z_i| at most
        assert np.abs(grz - rzr).max() <= 1e-12 * mag
        assert np.abs(gp - pr).max() <= ulp * np.abs(pr).max()


def test_three_iterations_are_not_enough():
    m = _model("float64")
    g = lambda k: object.__getattribute__(m, k)
    with pytest.raises(hb.gp.NotConverged) as ei:
        g("gp").condition(g("X"), g("Y"), 0.01, k_var=1.0, precond_rank=64, max_iter=3)
    info = ei.value.info
    print("max_iter=3: %r" % (info,))
    assert info["converged"] is False and info["iterations"] == 3 and info["residual"][0] > 1e-6


def test_condition_refuses_what_it_does_not_cover():
    class Host(hb.model.Model):
        def setUp(self, kern):
            self.gp = hb.gp.GP(kern=kern)

    X, Y = _dense()[:2]
    with pytest.raises(NotImplementedError, match="UnitRBF"):
        Host(kern=hb.gp.kernels.UnitMatern32(np.ones(1)), dtype="float64").gp.condition(X, Y, 0.01)
    with pytest.raises(NotImplementedError, match="one expert"):
        Host(kern=hb.gp.kernels.UnitRBF(np.ones((2, 1))), dtype="float64").gp.condition(X, Y, 0.01)
    host = Host(kern=hb.gp.kernels.UnitRBF(np.ones(1)), dtype="float64")
    with pytest.raises(NotImplementedError, match="64"):
        host.gp.condition(X, np.zeros((X.shape[0], 65)), 0.01)
    with pytest.raises(ValueError):
        host.gp.condition(X, Y[:-1], 0.01)
    with pytest.raises(NotImplementedError, match="one latent function"):
        host.gp.condition(X[:50], np.concatenate([Y[:50], -Y[:50]], axis=1), 0.01).sample_functions(2, num_features=8)
    with pytest.raises(ValueError, match="fit"):
        ExactGPR(X=X, Y=Y, dtype="float64").predict_f(X[:3])


def test_two_output_columns_are_two_solves():
    """Y [N, 2] in lockstep, the second column smooth and free of noise (its alpha is the more sensitive one): both true
    residuals at most 1e-6, and each column of alpha within |K^^-1| |b - K^ x| of its dense solve -- the bound its own
    residual gives (2-norms; |K^^-1| = 100 here)."""
    X, Y, ell, _, _, _, _, inv_norm = _dense()[:8]
    m = _model("float64")
    Y2 = np.concatenate([Y, np.cos(X[:, :1])], axis=1)
    post = object.__getattribute__(m, "gp").condition(X, Y2, 0.01, k_var=1.0)
    ref = np.linalg.solve(E.dense(X, ell, 1.0, 0.01), Y2).T
    err = np.linalg.norm(post.alpha - ref, axis=1)
    bound = inv_norm * post.info["residual"] * np.linalg.norm(Y2, axis=0)
    print("two columns: %d iterations, residuals %r, alpha errors %r of their bounds"
          % (post.info["iterations"], post.info["residual"], err / bound))
    assert post.alpha.shape == (2, 600) and np.all(post.info["residual"] <= 1e-6) and np.all(err <= bound * (1 + 1e-6))
    mean, var = post.predict_f(X[:5])
    assert mean.shape == (2, 5) and var.shape == (5,)


def test_exact_gpr_predicts_in_data_units():
    """ExactGPR.fit().predict_y on svgp_data(400, ...) with ell = 1.2, k_var = 0.8, var = 0.09 against the dense formula:
    mean and variance within 1e-5, float64."""
    X, Y, _ = svgp_data(400, 32, 0)
    m = ExactGPR(X=X, Y=Y, dtype="float64")
    m.gp.kern.lengthscales = np.ones(1) * 1.2
    m.k_var = np.ones(1) * 0.8
    m.var = np.ones(1) * 0.09
    xs = np.linspace(-1.0, 17.0, 70)[:, None]
    mean, var = m.fit().predict_y(xs)
    _, rm, rv = E.posterior(X, Y, np.array([1.2]), 0.8, 0.09, xs)
    fm, fv = m.predict_f(xs)
    print("ExactGPR: %d iterations at rank %d; mean error %.3e, variance error %.3e"
          % (m.posterior.info["iterations"], m.posterior.info["precond_rank"], np.abs(mean - rm).max(), np.abs(var - rv - 0.09).max()))
    assert mean.shape == (1, 70) and var.shape == (70,)
    assert np.abs(mean - rm).max() <= 1e-5 and np.abs(var - (rv + 0.09)).max() <= 1e-5
    assert np.array_equal(fm, mean) and np.abs(fv + 0.09 - var).max() <= 1e-12
    draws = m.sample_functions(4, num_features=32)
    assert draws(xs).shape == (4, 70)
