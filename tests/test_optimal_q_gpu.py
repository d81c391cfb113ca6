"""Closed-form optimal q(u) and the collapsed bound on the GPU, against the numpy restatement tests/optimal_q_ref.py
(itself pinned on the host by tests/test_optimal_q_cpu.py).

fp64 bounds are fixed (1e-10 of max|Phi| for the statistics, 1e-8 end to end).  fp32 bounds are NOT constants: each is
4 x the error the float32 numpy restatement (float32 A, float32 products over column blocks, float64 sum) makes against
float64 on the same inputs -- per 32 x 32 tile for the statistics, as test_fp32_parity_gpu.py measures products -- the
factor covering the different summation order inside a block.  Every figure is printed before it is asserted.

Observed on MI355X: in the docstrings of the tests; profiles/sgp_stats_errors.txt holds the full list."""
import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd import graph as G
from henbun_amd import hip_ops as H
from henbun_amd.models import SVGP, svgp_data

import optimal_q_ref as R
from parity import tile_err

pytestmark = pytest.mark.gpu
tf = hb.tf

KSPLIT = 432          # columns per float32 block of the restatement: the K-split of a full chunk at M = 512


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def _stats_case(N, M, d, P, seed):
    rng = np.random.RandomState(seed)
    dom = 0.5 * M if d == 1 else 4.0
    X = rng.uniform(0, dom, (N, d))
    Y = np.sin(X.sum(1, keepdims=True) + np.arange(P)[None, :]) + 0.3 * rng.randn(N, P)
    z = np.linspace(0, dom, M)[:, None] if d == 1 else rng.uniform(0, dom, (M, d))
    ell = np.ones(1) if d == 1 else np.array([0.9, 1.1, 1.3])
    _, W = R.chol_factor(z, ell, 1e-5 if d == 1 else 1e-3)
    return X, Y, z, ell, W


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("M", [32, 96, 512])
@pytest.mark.parametrize("N", [1, 97, 4096, 40001])
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_sgp_stats_against_the_restatement(dtype, d, P, N, M):
    """hb_sgp_stats_f64 / _f32: Phi, b, yy, a2sum; Phi bitwise symmetric; two runs bitwise equal.  N crosses a chunk
    (32768) and K-split boundaries and leaves ragged tails; M = 32, 96 use part of one tile, 512 ten tiles.
    Observed on MI355X: fp64 max|dPhi| / max|Phi| <= 5.2e-14; fp32 worst tile of Phi at 0.15 .. 2.31 x the restatement's
    error, of b at <= 2.28 x."""
    dt = torch.float64 if dtype == "float64" else torch.float32
    npdt = np.float64 if dtype == "float64" else np.float32
    X, Y, z, ell, W = (a.astype(npdt) for a in _stats_case(N, M, d, P, seed=N + M + d + P))
    args = [dev(a, dt) for a in (X, Y, z, ell, W)]
    out = H.sgp_stats(*args)
    out2 = H.sgp_stats(*args)
    torch.cuda.synchronize()
    for a, c in zip(out, out2):
        assert a.dtype == torch.float64 and torch.equal(a, c)
    Phi, b, yy, a2 = (o.cpu().numpy() for o in out)
    assert Phi.shape == (M, M) and b.shape == (P, M) and yy.shape == (P,) and a2.shape == (1,)
    assert np.array_equal(Phi, Phi.T)
    assert a2[0] == pytest.approx(np.trace(Phi), rel=1e-14)
    # reference: float64 arithmetic on the SAME (already rounded) inputs
    rPhi, rb, ryy, ra2 = R.stats_from_W(X, Y, z, ell, W)
    sc, scb = np.abs(rPhi).max(), np.abs(rb).max()
    ePhi, eb = np.abs(Phi - rPhi), np.abs(b - rb)
    print("sgp_stats %s N=%d M=%d d=%d P=%d: dPhi/max|Phi|=%.3e db/max|b|=%.3e dyy=%.3e da2sum=%.3e"
          % (dtype, N, M, d, P, ePhi.max() / sc, eb.max() / scb, np.abs(yy / ryy - 1).max(), abs(a2[0] / ra2 - 1)))
    assert np.abs(yy - ryy).max() <= 1e-12 * ryy.max()
    if dtype == "float64":
        assert ePhi.max() <= 1e-10 * sc
        assert eb.max() <= 1e-10 * scb
        assert abs(a2[0] - ra2) <= 1e-10 * ra2
        return
    # fp32: 4 x the float32 restatement's own error, both measured by the suite's tile measure (parity.tile_err: per
    # 32 x 32 tile ||a - b||_F / max(||b||_F, floor), the worst tile; tiles of Phi between inducing points many
    # lengthscales apart hold ~0 and are measured against the floor -- compared pairwise they are rounding against rounding)
    qPhi, qb, _, qa2 = R.stats_from_W(X, Y, z, ell, W, dtype=np.float32, ksplit=KSPLIT)
    gotPhi, refPhi = tile_err(Phi, rPhi), tile_err(qPhi, rPhi)
    gotb, refb = tile_err(b, rb), tile_err(qb, rb)
    print("   fp32 worst tile: Phi device %.3e, restatement %.3e (%.2f x); b %.3e vs %.3e (%.2f x); a2sum %.3e vs %.3e"
          % (gotPhi, refPhi, gotPhi / refPhi, gotb, refb, gotb / refb, abs(a2[0] - ra2) / ra2, abs(qa2 - ra2) / ra2))
    assert gotPhi <= 4.0 * refPhi
    assert gotb <= 4.0 * refb


# ------------------------------------------------------------------------------------------------ 2. end to end, fp64
def _model(N, M, q_shape, dtype, residual="diagonal", seed=0, **kw):
    X, Y, Z = svgp_data(N, M, seed)
    m = SVGP(X=X, Y=Y, Z=Z, q_shape=q_shape, residual=residual, dtype=dtype, **kw)
    m.gp.kern.lengthscales = np.ones(1) * 0.9
    m.k_var = np.ones(1) * 1.3
    m.var = np.ones(1) * 0.4
    m.initialize()
    return m, X, Y, Z


def _ref_fit(X, Y, Z, ell, noise_var, k_var, jitter=None):
    jitter = hb.settings.numerics.jitter_level if jitter is None else jitter
    st = R.stats(X, Y, Z, ell, jitter)
    m, S, s, _ = R.optimal_q(st[0], st[1], noise_var, k_var)
    return st, m, S, s


def test_optimal_q_and_collapsed_bound_fp64():
    """Observed on MI355X: m 5.4e-12, S S^T 1.7e-11, bound 1e-13 (relative)."""
    m, X, Y, Z = _model(20000, 64, "fullrank", "float64")
    st, rm, rS, rs = _ref_fit(X, Y, Z, np.array([0.9]), 0.4, 1.3)
    stats = m.gp.statistics(X, Y)
    assert all(t.dtype == torch.float64 and t.is_cuda for t in stats)
    qm, S = m.gp.optimal_q(X, Y, 0.4, 1.3, stats=stats)
    assert qm.shape == (1, 64) and S.shape == (64, 64) and qm.dtype == np.float64
    assert np.array_equal(S, np.tril(S)) and np.all(np.diag(S) > 0)
    em = np.abs(qm - rm).max() / np.abs(rm).max()
    eS = np.abs(S @ S.T - rS @ rS.T).max() / np.abs(rS @ rS.T).max()
    print("optimal_q fp64: m %.3e  S S^T %.3e" % (em, eS))
    assert em <= 1e-8 and eS <= 1e-8
    _, s = m.gp.optimal_q(X, Y, 0.4, 1.3, q_shape="diagonal", stats=stats)
    Lam = np.eye(64) + (1.3 / 0.4) * st[0]
    assert s.shape == (64,) and np.abs(s - np.diag(Lam) ** -0.5).max() <= 1e-8 * s.max()
    for residual in ("diagonal", "neglected"):
        got = m.gp.collapsed_bound(X, Y, 0.4, 1.3, residual=residual, stats=stats)
        ref = R.collapsed_bound(*st, 20000, 0.4, 1.3, residual)
        print("collapsed_bound fp64 %s: %.9f ref %.9f" % (residual, got, ref))
        assert abs(got - ref) <= 1e-8 * abs(ref)
    # residual does not change q*; the data may come from the model's own device buffers
    qm2, S2 = m.gp.optimal_q(object.__getattribute__(m, "X"), object.__getattribute__(m, "Y"), 0.4, 1.3, residual="neglected")
    assert np.array_equal(qm2, qm) and np.array_equal(S2, S)
    assert abs(m.collapsed_bound() - R.collapsed_bound(*st, 20000, 0.4, 1.3)) <= 1e-8 * abs(m.collapsed_bound())


def test_closed_form_refuses_what_it_does_not_cover():
    X, Y, Z = svgp_data(200, 32, 0)
    m, _, _, _ = _model(200, 32, "diagonal", "float64")
    with pytest.raises(NotImplementedError, match="fullrank"):
        m.gp.optimal_q(X, Y, 0.4, residual="fullrank")
    with pytest.raises(NotImplementedError, match="fullrank"):
        m.gp.collapsed_bound(X, Y, 0.4, residual="fullrank")
    with pytest.raises(ValueError):
        m.gp.optimal_q(X, Y, -1.0)

    class Other(hb.model.Model):
        def setUp(self, Z, kern):
            self.gp = hb.gp.SparseGP(kern=kern, z=Z)

    with pytest.raises(NotImplementedError, match="UnitRBF"):
        Other(Z=Z, kern=hb.gp.kernels.UnitMatern52(np.ones(1)), dtype="float64").gp.statistics(X, Y)
    with pytest.raises(NotImplementedError, match="one expert"):
        Other(Z=np.stack([Z, Z]), kern=hb.gp.kernels.UnitRBF(np.ones((2, 1))), dtype="float64").gp.statistics(X, Y)
    cfg = hb.settings.get_settings()
    cfg.numerics.jitter_level = 0.0
    with hb.settings.temp_settings(cfg):
        bad = Other(Z=np.zeros((32, 1)), kern=hb.gp.kernels.UnitRBF(np.ones(1)), dtype="float64")
        with pytest.raises(G.CholeskyError):
            bad.gp.statistics(X, Y)


# ------------------------------------------------------------------------------------------------ 3. the property
def _grad_plan(m):
    """(plan, objective, [d objective / d q_mu, d objective / d q_sqrt]) of the model's own ELBO on ALL rows."""
    opt = m.ELBO()
    opt._ensure_compiled()
    m.initialize()
    obj = opt._trace(None)
    q = object.__getattribute__(m, "u")
    leaves = [object.__getattribute__(q, "q_mu")._leaf, object.__getattribute__(q, "q_sqrt")._leaf]
    grads = G.gradients(obj, leaves)
    plan = m._session.make_plan([obj] + grads, minibatch=None)
    return plan, obj, grads


def _grad_draws(plan, grads, K, M):
    """[K, M + M(M+1)/2]: the gradient w.r.t. q_mu and the lower triangle of q_sqrt, one row per noise draw."""
    il = np.tril_indices(M)
    rows = []
    for _ in range(K):
        plan.run()
        plan.check()
        g_mu = plan.value(grads[0]).astype(np.float64).reshape(-1)
        g_sq = plan.value(grads[1]).astype(np.float64).reshape(M, M)
        rows.append(np.concatenate([g_mu, g_sq[il]]))
    return np.stack(rows)


def _frac_within(draws, k=4.0):
    mean = draws.mean(0)
    se = draws.std(0, ddof=1) / np.sqrt(draws.shape[0])
    return float(np.mean(np.abs(mean) <= k * se)), mean, se


def _model_factor(Z, ell, jitter):
    """W = chol(K(z, z) + jitter I)^-1 in float32 as the model's own (existing) factor + inverse launches produce it --
    the calls SparseGP.statistics makes.  hb_sgp_stats takes W as an INPUT (test 1 hands the device and the restatement
    the same W); the float32 restatement of fit_q + predict_f takes it the same way."""
    z = dev(Z, torch.float32)
    _, W, info = H.cholesky_inverse(H.gram_fwd(z, z, dev(ell, torch.float32), diag_add=float(jitter)))
    assert int(info.cpu()[0]) == 0
    return W.cpu().numpy()


def _float32_pipeline_prediction(X, Y, Z, ell, noise_var, k_var, xs, W32):
    """The float32 restatement of fit_q + predict_f for a given float32 W: float32 A, float32 block products summed in
    float64, q* from those statistics in float64, the prediction through the float32 A."""
    f = np.float32
    z32, ell32 = Z.astype(f), np.asarray(ell, f)
    st = R.stats_from_W(X, Y, z32, ell32, W32, dtype=f, ksplit=KSPLIT)
    m, S, _, _ = R.optimal_q(st[0], st[1], noise_var, k_var)
    A = R.A_of(W32, z32, xs.astype(f), ell32).astype(np.float64)
    mean = np.sqrt(k_var) * (m @ A)
    var = k_var * (((S.T @ A) ** 2).sum(0) + np.abs(1.0 - (A * A).sum(0)))
    return mean, np.broadcast_to(var, mean.shape)


def test_fit_q_zeroes_the_gradient_of_the_existing_elbo_and_predicts_the_exact_posterior():
    """After SVGP.fit_q() the Monte-Carlo gradient of the EXISTING ELBO objective w.r.t. q_mu and q_sqrt (all 4096 rows,
    analytic KL) is zero within 4 standard errors for >= 99 % of the entries; at the initial q it is not.  predict_f then
    is the restatement's sparse posterior (1e-8, fp64); fp32 against the fp64 run within 4 x the float32 restatement's
    error, the restatement taking the model's own float32 W as its input the way test 1 hands W to both sides.
    Observed on MI355X: 100 % of 560 entries within 4 s.e. after fit_q (largest 3.18 s.e.), 93 % at the initial q (6.3);
    fp64 predict_f 1.1e-13; fp32 mean 5.9e-5 (restatement 5.5e-5), var 2.8e-5 (restatement 9.4e-6: 3.0 x).  A restatement
    that factorises K(z, z) itself with LAPACK in float32 errs by 3.3e-5 / 4.0e-6: against THAT the variance reads 7.1 x --
    the model's existing fp32 factor + inverse is about twice as far from float64 as LAPACK's on this z (|dW| 0.18 against
    0.08 at max|W| = 37), and that error, not the statistics', is what the prediction at the extrapolating points carries."""
    N, M, K = 4096, 32, 128
    cfg = hb.settings.get_settings()
    cfg.numerics.kl_form = "analytic"
    xs = np.linspace(-1.0, 0.5 * M + 1.0, 200)[:, None]
    with hb.settings.temp_settings(cfg):
        m, X, Y, Z = _model(N, M, "fullrank", "float64")
        plan, obj, grads = _grad_plan(m)
        d0 = _grad_draws(plan, grads, K, M)
        frac0, mean0, se0 = _frac_within(d0)
        qm, S = m.fit_q()
        d1 = _grad_draws(plan, grads, K, M)            # the same plan: it reads the parameters fit_q wrote
        frac1, mean1, se1 = _frac_within(d1)
        print("gradient of ELBO w.r.t. q: initial q %.1f %% of %d entries within 4 s.e. (max |g| / s.e. %.1f); after fit_q "
              "%.2f %% (max %.2f)" % (100 * frac0, d0.shape[1], np.max(np.abs(mean0) / se0), 100 * frac1,
                                      np.max(np.abs(mean1) / np.maximum(se1, 1e-300))))
        assert np.all(se1 > 0)
        assert frac1 >= 0.99
        assert frac0 < 0.99
        # the parameters hold q* in their own parametrisation
        q = object.__getattribute__(m, "u")
        assert np.allclose(q.q_mu.value.reshape(1, M), qm, rtol=0, atol=1e-14)
        assert np.allclose(np.tril(q.q_sqrt.value), S, rtol=0, atol=1e-14)
        mu64, v64 = m.predict_f(xs)
        st, rm, rS, _ = _ref_fit(X, Y, Z, np.array([0.9]), 0.4, 1.3)
        rmu, rv = R.predict(xs, Z, np.array([0.9]), hb.settings.numerics.jitter_level, rm, rS, 1.3)
        e_mu, e_v = np.abs(mu64 - rmu).max(), np.abs(v64 - rv).max()
        print("predict_f after fit_q, fp64: mean %.3e var %.3e" % (e_mu, e_v))
        assert e_mu <= 1e-8 and e_v <= 1e-8
        # fp32
        m32, _, _, _ = _model(N, M, "fullrank", "float32")
        m32.fit_q()
        mu32, v32 = m32.predict_f(xs)
        jitter = hb.settings.numerics.jitter_level
        qmu, qv = _float32_pipeline_prediction(X, Y, Z, [0.9], 0.4, 1.3, xs, _model_factor(Z, [0.9], jitter))
        b_mu, b_v = np.abs(qmu - rmu).max(), np.abs(qv - rv).max()
        g_mu, g_v = np.abs(mu32 - mu64).max(), np.abs(v32 - v64).max()
        print("predict_f after fit_q, fp32 vs fp64: mean %.3e (float32 restatement %.3e) var %.3e (%.3e)"
              % (g_mu, b_mu, g_v, b_v))
        # for the record, not asserted: the restatement on a float32 LAPACK factor of its own instead of the model's W
        lmu, lv = _float32_pipeline_prediction(X, Y, Z, [0.9], 0.4, 1.3, xs,
                                               R.chol_factor(Z.astype(np.float32), np.float32([0.9]), np.float32(jitter))[1])
        print("   (restatement on numpy's own float32 factor: mean %.3e var %.3e)"
              % (np.abs(lmu - rmu).max(), np.abs(lv - rv).max()))
        assert g_mu <= 4.0 * b_mu
        assert g_v <= 4.0 * b_v


def test_fit_q_diagonal_writes_log_standard_deviations():
    m, X, Y, Z = _model(4096, 32, "diagonal", "float64")
    qm, s = m.fit_q()
    q = object.__getattribute__(m, "u")
    st, rm, _, rs = _ref_fit(X, Y, Z, np.array([0.9]), 0.4, 1.3)
    assert np.abs(s - rs).max() <= 1e-8 * rs.max() and np.abs(qm - rm).max() <= 1e-8 * np.abs(rm).max()
    assert np.allclose(q.q_sqrt.value.reshape(-1), np.log(s), rtol=0, atol=1e-14)
    xs = np.linspace(0, 16, 50)[:, None]
    mu, v = m.predict_f(xs)
    rmu, rv = R.predict(xs, Z, np.array([0.9]), hb.settings.numerics.jitter_level, rm, rs, 1.3)
    assert np.abs(mu - rmu).max() <= 1e-8 and np.abs(v - rv).max() <= 1e-8


# ------------------------------------------------------------------------------------------------ 4. the envelope
def test_collapsed_bound_is_the_envelope_of_what_adam_reaches():
    """collapsed_bound() at the hyper-parameters a 200-step Adam run ended with >= the mean of 64 evaluations of the
    existing Monte-Carlo ELBO (all rows) at the q it reached, minus 4 of their standard errors."""
    np.random.seed(0)
    m, X, Y, Z = _model(2000, 32, "fullrank", "float64")
    opt = m.ELBO()
    opt.compile(optimizer=tf.train.AdamOptimizer(1e-2))
    opt.optimize(maxiter=200, minibatch_size=256)
    vals = np.array([opt.run() for _ in range(64)])
    bound = m.collapsed_bound()
    mean, se = vals.mean(), vals.std(ddof=1) / 8.0
    print("collapsed bound %.4f; Monte-Carlo ELBO after 200 Adam steps %.4f +- %.4f" % (bound, mean, se))
    assert np.isfinite(bound) and se > 0
    assert bound >= mean - 4.0 * se
    # and fit_q() lifts the Monte-Carlo ELBO to the bound
    m.fit_q()
    vals = np.array([opt.run() for _ in range(64)])
    mean, se = vals.mean(), vals.std(ddof=1) / 8.0
    print("   after fit_q: Monte-Carlo ELBO %.4f +- %.4f" % (mean, se))
    assert abs(bound - mean) <= 4.0 * se


# ------------------------------------------------------------------------------------------------ 5. full size
def test_fullsize_fit_q_N1e6_M512_fp32():
    """cfg 2 size: N = 1e6, M = 512, fp32.  fit_q() then predict_f on 1000 points against the float64 posterior computed
    on the host in chunks; bound: 4 x the error of the float32 restatement of the same pipeline (max over the points).
    The workspace does not depend on N.  Observed on MI355X: mean 1.6e-5 (restatement 1.5e-5), var 2.9e-6 (2.9e-6), the
    bound -215609.886 against -215611.012 (5e-6 relative; about 2e-7 of the sum of its terms' magnitudes)."""
    N, M = 1000000, 512
    assert H.sgp_stats_ws_elems(torch.float32, 100000, M, 1, 1) == H.sgp_stats_ws_elems(torch.float32, N, M, 1, 1)
    X, Y, Z = svgp_data(N, M, 0)
    m = SVGP(X=X, Y=Y, Z=Z, q_shape="diagonal", dtype="float32")
    m.gp.kern.lengthscales = np.ones(1)
    m.k_var = np.ones(1)
    m.var = np.ones(1) * 0.09
    m.initialize()
    qm, s = m.fit_q()
    xs = np.linspace(0.0, 0.5 * M, 1000)[:, None]
    mu, v = m.predict_f(xs)
    bound = m.collapsed_bound()
    # host: float64 and float32 statistics in chunks
    jitter = hb.settings.numerics.jitter_level
    ell = np.ones(1)
    _, W64 = R.chol_factor(Z, ell, jitter)
    z32, ell32 = Z.astype(np.float32), ell.astype(np.float32)
    W32 = _model_factor(Z, ell, jitter)
    Phi, b = np.zeros((M, M)), np.zeros((1, M))
    Phi32, b32 = np.zeros((M, M)), np.zeros((1, M))
    X32, Y32 = X.astype(np.float32), Y.astype(np.float32)
    for j0 in range(0, N, 32768):
        A = R.A_of(W64, Z, X[j0:j0 + 32768], ell)
        Phi += A @ A.T
        b += (A @ Y[j0:j0 + 32768]).T
        A = R.A_of(W32, z32, X32[j0:j0 + 32768], ell32)
        for k0 in range(0, A.shape[1], KSPLIT):
            Ak = A[:, k0:k0 + KSPLIT]
            Phi32 += (Ak @ Ak.T).astype(np.float64)
            b32 += (Ak @ Y32[j0 + k0:j0 + k0 + Ak.shape[1]]).T.astype(np.float64)
    yy = (Y ** 2).sum(0)
    rm, _, rs, _ = R.optimal_q(Phi, b, 0.09, 1.0)
    rmu, rv = R.predict(xs, Z, ell, jitter, rm, rs, 1.0, W=W64)
    qm32, _, qs32, _ = R.optimal_q(Phi32, b32, 0.09, 1.0)
    A = R.A_of(W32, z32, xs.astype(np.float32), ell32).astype(np.float64)
    qmu = qm32 @ A
    qv = ((qs32[:, None] * A) ** 2).sum(0) + np.abs(1.0 - (A * A).sum(0))
    b_mu, b_v = np.abs(qmu - rmu).max(), np.abs(qv - rv).max()
    g_mu, g_v = np.abs(mu - rmu).max(), np.abs(v - rv).max()
    rbound = R.collapsed_bound(Phi, b, yy, float(np.trace(Phi)), N, 0.09, 1.0)
    print("full size fp32: predict_f mean %.3e (float32 restatement %.3e) var %.3e (%.3e); bound %.3f ref %.3f (rel %.2e)"
          % (g_mu, b_mu, g_v, b_v, bound, rbound, abs(bound - rbound) / abs(rbound)))
    assert g_mu <= 4.0 * b_mu
    assert g_v <= 4.0 * b_v
    # the bound: every term of it to fp32-level relative accuracy (16 x 2^-24 ~ 1e-6 of the sum of the terms' magnitudes;
    # the terms are of order N / noise_var and cancel to a value an order of magnitude smaller)
    Lam = np.eye(M) + Phi / 0.09
    c = b / 0.09
    terms = (0.5 * N * abs(np.log(2 * np.pi * 0.09)) + yy.sum() / 0.18 + 0.5 * float((c @ np.linalg.solve(Lam, c.T))[0, 0])
             + 0.5 * np.linalg.slogdet(Lam)[1] + (N - np.trace(Phi)) / 0.18)
    assert abs(bound - rbound) <= 1e-6 * terms
