"""Psi statistics (uncertain inputs) on the GPU against the numpy restatement tests/psi_ref.py (itself pinned on the host by
tests/test_psi_cpu.py): the raw kernels hb_sgp_psi_stats_* / hb_sgp_psi_predict_* in both storage types, then
SparseGP.psi_statistics, SparsePosterior.predict_uncertain and the SVGP methods on top of them.

Bounds.  Psi2 and C elementwise: |got - ref| <= (8192 + 2 N) 2^-52 |ref| + 1e-280 -- every term of the sums is positive (the
raw cases use positive Y), a term's relative error is its exponent (at most 745 before underflow) times a few roundings,
a sequential sum adds N roundings, and the factor 2 covers the reference's own error.  The whitened tuple: 1e-10 of the
largest entry, at jitter_level = 1e-3 (at 1e-5 the float64 restatement ITSELF errs by up to 5e-10 of max|Phi| against
80-bit arithmetic: Phi = W Psi2 W^T amplifies by |W|^2 ~ 1 / jitter).  End to end: 1e-8.  Every figure is printed before
it is asserted.

The split of N by the statistics kernel (csrc/sgp_psi.hip), restated here so that the cases below can be seen to cross it:
tiles T = nt (nt + 1) / 2 with nt = ceil(M / PSI_BT); at most S = max(1, PSI_TARGET_WG // T) splits; points per split
ks = ceil(N / S) rounded up to PSI_PB; splits = ceil(N / ks).  N = 5000 at M = 33: T = 1, ks = 64, 79 splits, the last of 8
points; at M = 128: T = 3, S = 1365, ks = 64, 79 splits; N = 257 crosses the staging step of PSI_PB points four times with
one point left over.

Observed on MI355X: see the docstrings of the tests and profiles/sgp_psi.txt."""
import functools

import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd import hip_ops as H
from henbun_amd.models import SVGP, svgp_data

import optimal_q_ref as R
import psi_ref as PR

pytestmark = pytest.mark.gpu

PSI_BT = 64            # tile of pairs
PSI_PB = 64            # points staged per step = the granule of a split
PSI_TARGET_WG = 4096   # tiles x splits aimed at

DT = {"float64": (torch.float64, np.float64), "float32": (torch.float32, np.float32)}
DIMS = [(1, 1), (3, 1), (3, 3), (5, 1), (5, 5)]      # (d, dl): dl in {1, d}


def splits_of(N, M):
    nt = -(-M // PSI_BT)
    S = max(1, PSI_TARGET_WG // (nt * (nt + 1) // 2))
    ks = -(-(-(-N // S)) // PSI_PB) * PSI_PB
    return -(-N // ks), ks


def test_the_cases_cross_the_split_rule():
    assert splits_of(5000, 33) == (79, 64) and 5000 - 78 * 64 == 8
    assert splits_of(5000, 128) == (79, 64) and splits_of(257, 64) == (5, 64) and splits_of(2, 1) == (1, 64)


def dev(a, dt):
    return torch.as_tensor(np.array(a), dtype=dt).cuda().contiguous()      # (a copy: the cached cases are read-only)


def _inputs(n, M, d, dl, npdt, seed):
    """Storage-rounded (mu, s, z, ell) with variances in [0, 0.36] l^2, every 7th row exactly zero, one row at 100 l^2 and one
    point 60 lengthscales from every z (its terms underflow to 0) -- as far as n has the rows."""
    rng = np.random.RandomState(seed)
    ell = rng.uniform(0.7, 1.4, dl)
    lf = np.broadcast_to(ell, (d,))
    z = rng.uniform(0.0, 4.0, (M, d)) * lf
    mu = rng.uniform(-0.5, 4.5, (n, d)) * lf
    s = rng.uniform(0.0, 0.36, (n, d)) * lf ** 2
    if n > 3:
        s[2, 0] = 0.0                                   # a zero in one dimension only
        s[3] = 100.0 * lf ** 2
    elif n == 2:
        s[1] = 100.0 * lf ** 2
    if n > 5:
        mu[5] = z.max(0) + 60.0 * lf
    s[::7] = 0.0
    return tuple(np.ascontiguousarray(a.astype(npdt)) for a in (mu, s, z, ell))


@functools.lru_cache(maxsize=None)
def _stats_case(dtype, N, M, d, dl):
    """inputs (three POSITIVE columns of Y) and the float64 reference on the rounded inputs, computed once per shape"""
    npdt = DT[dtype][1]
    mu, s, z, ell = _inputs(N, M, d, dl, npdt, seed=N + 7 * M + 31 * d + dl)
    Y = np.random.RandomState(N + M).uniform(0.5, 1.5, (N, 3)).astype(npdt)
    ref = PR.stats_raw(mu, s, Y, z, ell)
    for a in (mu, s, z, ell, Y) + ref:
        a.flags.writeable = False
    return (mu, s, Y, z, ell), ref


# ------------------------------------------------------------------------------------------------ 1. the raw kernels
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("d, dl", DIMS)
@pytest.mark.parametrize("N", [1, 2, 257, 5000])
@pytest.mark.parametrize("M", [1, 33, 64, 128])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_psi_stats_against_the_restatement(dtype, M, N, d, dl, P):
    """hb_sgp_psi_stats_f64 / _f32: Psi2 and C elementwise, yy; Psi2 bitwise symmetric; two calls bitwise equal.  M: one
    pair, a ragged tile, a full tile, three tiles (one off the diagonal); N: below, across and far beyond one staging step
    and one split; d = 5 takes the loop over the dimensions, d <= 4 the register forms.
    Observed on MI355X over the 320 cases: worst |dPsi2| at 0.008 of its bound, worst |dC| at 0.004, yy 1.2e-14."""
    dt = DT[dtype][0]
    (mu, s, Y3, z, ell), (rPsi2, rC3, ryy3) = _stats_case(dtype, N, M, d, dl)
    Y, rC, ryy = np.ascontiguousarray(Y3[:, :P]), rC3[:P], ryy3[:P]
    args = [dev(a, dt) for a in (mu, s, Y, z, ell)]
    out = H.sgp_psi_stats(*args)
    out2 = H.sgp_psi_stats(*args)
    torch.cuda.synchronize()
    for a, c in zip(out, out2):
        assert a.dtype == torch.float64 and torch.equal(a, c)
    Psi2, C, yy = (o.cpu().numpy() for o in out)
    assert Psi2.shape == (M, M) and C.shape == (P, M) and yy.shape == (P,)
    assert np.array_equal(Psi2, Psi2.T)
    assert np.all(np.isfinite(Psi2)) and np.all(np.isfinite(C)) and np.all(Psi2 >= 0)
    eps = (8192 + 2 * N) * 2.0 ** -52
    r2 = np.abs(Psi2 - rPsi2) / (eps * np.abs(rPsi2) + 1e-280)
    rc = np.abs(C - rC) / (eps * np.abs(rC) + 1e-280)
    print("psi_stats %s M=%d N=%d d=%d dl=%d P=%d: worst |dPsi2| / bound %.3f, |dC| / bound %.3f, dyy %.2e"
          % (dtype, M, N, d, dl, P, r2.max(), rc.max(), np.abs(yy / ryy - 1).max()))
    assert r2.max() <= 1.0
    assert rc.max() <= 1.0
    assert np.abs(yy - ryy).max() <= 1e-12 * ryy.max()


def test_psi_stats_far_point_adds_nothing_and_zero_variance_is_the_kernel():
    """The point 60 lengthscales away contributes exact zeros (never NaN): dropping it leaves Psi2 and C bitwise unchanged
    when it is the last point of its split; and with Xvar = 0 everywhere Psi2 is sum_n k k^T."""
    rng = np.random.RandomState(0)
    M, d = 33, 2
    ell = np.array([0.9, 1.2])
    z = rng.uniform(0, 4, (M, d))
    mu = rng.uniform(0, 4, (40, d))
    s = rng.uniform(0, 0.3, (40, d))
    Y = rng.uniform(0.5, 1.5, (40, 1))
    mu[-1] = z.max(0) + 60.0 * ell
    full = H.sgp_psi_stats(*[dev(a, torch.float64) for a in (mu, s, Y, z, ell)])
    part = H.sgp_psi_stats(*[dev(a, torch.float64) for a in (mu[:-1], s[:-1], Y[:-1], z, ell)])
    assert torch.equal(full[0], part[0]) and torch.equal(full[1], part[1])
    cert = H.sgp_psi_stats(*[dev(a, torch.float64) for a in (mu, np.zeros_like(s), Y, z, ell)])[0].cpu().numpy()
    K = R.rbf(z, mu, ell)
    err = np.abs(cert - K @ K.T).max() / np.abs(K @ K.T).max()
    print("psi_stats at zero variance against K K^T: %.2e" % err)
    assert err <= 1e-13


def test_psi_stats_more_columns_of_Y_than_one_pass_carries():
    """P = 6: psi1_stats_kernel carries 4 columns of Y per pass over the points, so this takes two; same bound on C."""
    N, M, d, P = 300, 70, 2, 6
    mu, s, z, ell = _inputs(N, M, d, d, np.float64, seed=11)
    Y = np.random.RandomState(12).uniform(0.5, 1.5, (N, P))
    _, rC, ryy = PR.stats_raw(mu, s, Y, z, ell)
    _, C, yy = (o.cpu().numpy() for o in H.sgp_psi_stats(*[dev(a, torch.float64) for a in (mu, s, Y, z, ell)]))
    rc = np.abs(C - rC) / ((8192 + 2 * N) * 2.0 ** -52 * np.abs(rC) + 1e-280)
    print("psi_stats P=6: worst |dC| / bound %.3f" % rc.max())
    assert C.shape == (P, M) and rc.max() <= 1.0 and np.abs(yy - ryy).max() <= 1e-12 * ryy.max()


@pytest.mark.parametrize("d, dl", [(1, 1), (3, 3), (5, 1)])
@pytest.mark.parametrize("n", [1, 300])
@pytest.mark.parametrize("M", [33, 128])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_psi_predict_against_the_restatement(dtype, M, n, d, dl):
    """hb_sgp_psi_predict_*: e1 within 1e-12 sum|beta|, e2 within 1e-12 sum|Q| (psi1, psi2 <= 1, so these are the scales of
    the sums), random beta and a random symmetric Q; each point alone returns the bits it has in the batch.  M = 33 is one
    workgroup per point, M = 128 three.  Observed on MI355X: e1 <= 7.9e-17 sum|beta|, e2 <= 5.2e-17 sum|Q|."""
    dt, npdt = DT[dtype]
    mu, s, z, ell = _inputs(n, M, d, dl, npdt, seed=n + M + d)
    rng = np.random.RandomState(M + d)
    beta = rng.randn(M)
    Q = rng.randn(M, M)
    Q = Q + Q.T
    args = [dev(a, dt) for a in (mu, s, z, ell)] + [dev(beta, torch.float64), dev(Q, torch.float64)]
    e1, e2 = H.sgp_psi_predict(*args)
    r1, r2 = PR.contractions(mu, s, z, ell, beta, Q)
    g1, g2 = e1.cpu().numpy(), e2.cpu().numpy()
    err1, err2 = np.abs(g1 - r1).max() / np.abs(beta).sum(), np.abs(g2 - r2).max() / np.abs(Q).sum()
    print("psi_predict %s M=%d n=%d d=%d dl=%d: e1 %.2e of sum|beta|, e2 %.2e of sum|Q|" % (dtype, M, n, d, dl, err1, err2))
    assert g1.shape == (n,) and g2.shape == (n,) and e1.dtype == torch.float64
    assert err1 <= 1e-12 and err2 <= 1e-12
    for j in sorted({0, n // 2, n - 1}):
        a1, a2 = H.sgp_psi_predict(args[0][j:j + 1].contiguous(), args[1][j:j + 1].contiguous(), *args[2:])
        assert torch.equal(a1, e1[j:j + 1]) and torch.equal(a2, e2[j:j + 1])


# ------------------------------------------------------------------------------------------------ 2. SparseGP.psi_statistics
JITTER = 1e-3


def _settings():
    cfg = hb.settings.get_settings()
    cfg.numerics.jitter_level = JITTER
    return hb.settings.temp_settings(cfg)


def _model(N, M, q_shape, dtype, residual="diagonal", seed=0):
    X, Y, Z = svgp_data(N, M, seed)
    m = SVGP(X=X, Y=Y, Z=Z, q_shape=q_shape, residual=residual, dtype=dtype)
    m.gp.kern.lengthscales = np.ones(1) * 0.9
    m.k_var = np.ones(1) * 1.3
    m.var = np.ones(1) * 0.4
    m.initialize()
    return m, X, Y, Z


def _variances(N, seed=1):
    s = np.random.RandomState(seed).uniform(0.0, 0.36, (N, 1)) * 0.81
    s[::7] = 0.0
    return s


@functools.lru_cache(maxsize=None)
def _session_reference(N, M):
    """(X, Y, Z, s, the restatement's whitened tuple) for the float64 session tests"""
    X, Y, Z = svgp_data(N, M, 0)
    s = _variances(N)
    return X, Y, Z, s, PR.stats(X, s, Y, Z, np.array([0.9]), JITTER)


def test_psi_statistics_optimal_q_and_collapsed_bound_fp64():
    """SparseGP.psi_statistics in a float64 session at jitter_level 1e-3: Phi and b within 1e-10 of their largest entries,
    optimal_q(stats=) and collapsed_bound(stats=) within 1e-8 of the restatement; X_var = 0 against statistics(); the [d]
    and scalar forms of X_var.  Observed on MI355X: Phi 8.8e-13, b 4.2e-14, a2sum 5.9e-14; m 1.7e-11, S S^T 3.3e-10; the
    bound equal to the restatement's in all 9 printed decimals; X_var = 0 against statistics() 1.5e-13."""
    N, M = 1500, 48
    X, Y, Z, s, ref = _session_reference(N, M)
    with _settings():
        m, _, _, _ = _model(N, M, "fullrank", "float64")
        stats = m.gp.psi_statistics(X, s, Y)
        assert all(t.dtype == torch.float64 and t.is_cuda for t in stats)
        Phi, b, yy, a2 = (t.cpu().numpy() for t in stats)
        assert Phi.shape == (M, M) and b.shape == (1, M) and yy.shape == (1,) and a2.shape == (1,)
        assert np.array_equal(Phi, Phi.T)
        ePhi, eb = np.abs(Phi - ref[0]).max() / np.abs(ref[0]).max(), np.abs(b - ref[1]).max() / np.abs(ref[1]).max()
        print("psi_statistics fp64: Phi %.3e b %.3e yy %.1e a2sum %.3e" % (ePhi, eb, abs(yy[0] / ref[2][0] - 1), abs(a2[0] / ref[3] - 1)))
        assert ePhi <= 1e-10 and eb <= 1e-10 and abs(a2[0] - ref[3]) <= 1e-10 * ref[3]
        assert abs(yy[0] - ref[2][0]) <= 1e-12 * ref[2][0]
        rm, rS, rs, _ = R.optimal_q(ref[0], ref[1], 0.4, 1.3)
        qm, S = m.gp.optimal_q(X, Y, 0.4, 1.3, stats=stats)
        em = np.abs(qm - rm).max() / np.abs(rm).max()
        eS = np.abs(S @ S.T - rS @ rS.T).max() / np.abs(rS @ rS.T).max()
        print("optimal_q(stats=psi) fp64: m %.3e  S S^T %.3e" % (em, eS))
        assert em <= 1e-8 and eS <= 1e-8
        for residual in ("diagonal", "neglected"):
            got = m.gp.collapsed_bound(X, Y, 0.4, 1.3, residual=residual, stats=stats)
            want = R.collapsed_bound(*ref, N, 0.4, 1.3, residual)
            print("collapsed_bound(stats=psi) fp64 %s: %.9f ref %.9f" % (residual, got, want))
            assert abs(got - want) <= 1e-8 * abs(want)
        # zero variance: the certain-input statistics
        cert = [t.cpu().numpy() for t in m.gp.statistics(X, Y)]
        for form in (0.0, np.zeros(1), np.zeros((N, 1))):
            zero = [t.cpu().numpy() for t in m.gp.psi_statistics(X, form, Y)]
            e0 = np.abs(zero[0] - cert[0]).max() / np.abs(cert[0]).max()
            print("psi_statistics(X, 0, Y) against statistics(X, Y): Phi %.3e" % e0)
            assert e0 <= 1e-10 and np.abs(zero[1] - cert[1]).max() <= 1e-10 * np.abs(cert[1]).max()
        # a shared variance in its three forms: the same bits
        a = m.gp.psi_statistics(X, 0.2, Y)
        for form in (np.array([0.2]), np.full((N, 1), 0.2)):
            assert all(torch.equal(p, q) for p, q in zip(a, m.gp.psi_statistics(X, form, Y)))


def test_psi_statistics_fp32_session():
    """The same calls in a float32 session against the restatement on the float32-rounded inputs and the DEVICE's W (the
    float32 factor + inverse of the session, read back): the arithmetic after W is double, so the bound stays 1e-10.
    Observed on MI355X: Phi 7.2e-13, b 1.5e-14, a2sum 1.0e-13; m 1.2e-11, S S^T 2.6e-10: 1e-10 is attained, no wider bound."""
    N, M = 1500, 48
    X, Y, Z, s, _ = _session_reference(N, M)
    f = np.float32
    with _settings():
        m, _, _, _ = _model(N, M, "fullrank", "float32")
        Phi, b, yy, a2 = (t.cpu().numpy() for t in m.gp.psi_statistics(X, s, Y))
        # z, the lengthscale and W exactly as psi_statistics takes them (the lengthscale is the transform of a float32 raw
        # parameter: not float32(0.9) to the last bit, and W moves by cond(K(z, z)) times that)
        gp = object.__getattribute__(m, "gp")
        z32, ell32, W, _ = gp._whitening(*gp._stats_session("test"), None, None, "test")
        ref = PR.stats(X.astype(f), s.astype(f), Y.astype(f), z32.cpu().numpy(), ell32.cpu().numpy(), W=W.cpu().numpy())
        ePhi, eb = np.abs(Phi - ref[0]).max() / np.abs(ref[0]).max(), np.abs(b - ref[1]).max() / np.abs(ref[1]).max()
        print("psi_statistics fp32 session: Phi %.3e b %.3e a2sum %.3e" % (ePhi, eb, abs(a2[0] / ref[3] - 1)))
        assert np.array_equal(Phi, Phi.T)
        assert ePhi <= 1e-10 and eb <= 1e-10 and abs(a2[0] - ref[3]) <= 1e-10 * ref[3]
        rm, rS, _, _ = R.optimal_q(ref[0], ref[1], 0.4, 1.3)
        stats = m.gp.psi_statistics(X, s, Y)
        qm, S = m.gp.optimal_q(X, Y, 0.4, 1.3, stats=stats)
        em = np.abs(qm - rm).max() / np.abs(rm).max()
        eS = np.abs(S @ S.T - rS @ rS.T).max() / np.abs(rS @ rS.T).max()
        got, want = m.gp.collapsed_bound(X, Y, 0.4, 1.3, stats=stats), R.collapsed_bound(*ref, N, 0.4, 1.3)
        print("   optimal_q m %.3e S S^T %.3e; bound %.9f ref %.9f" % (em, eS, got, want))
        assert em <= 1e-8 and eS <= 1e-8 and abs(got - want) <= 1e-8 * abs(want)


# ------------------------------------------------------------------------------------------------ 3. predict_uncertain
@pytest.mark.parametrize("residual", ["diagonal", "neglected"])
@pytest.mark.parametrize("q_shape", ["fullrank", "diagonal"])
def test_predict_uncertain_against_the_restatement(q_shape, residual):
    """SparsePosterior.predict_uncertain (float64 session, jitter_level 1e-3: Q = W^T (..) W carries |W|^2 ~ 1 / jitter, the
    amplification the statistics have) against the restatement within 1e-8, for full-rank and mean-field q and both
    residual modes; X_var = 0 against predict(); the variance is non-negative.  Observed on MI355X: mean <= 9.1e-15, var <=
    9.5e-13; X_var = 0 against predict: mean 2.3e-15, var <= 5.8e-13; smallest variance 1.0e-2."""
    N, M, n = 600, 32, 200
    rng = np.random.RandomState(3)
    xs = rng.uniform(-1.0, 0.5 * M + 1.0, (n, 1))
    sv = rng.uniform(0.0, 0.36, (n, 1)) * 0.81
    sv[::7] = 0.0
    with _settings():
        m, X, Y, Z = _model(N, M, q_shape, "float64", residual)
        qm, S = m.fit_q()
        post = m.posterior()
        mean, var = post.predict_uncertain(xs, sv)
        _, W = R.chol_factor(Z, np.array([0.9]), JITTER)
        rmean, rvar = PR.predict_uncertain(xs, sv, Z, np.array([0.9]), W, qm, S, 1.3, residual)
        e_m, e_v = np.abs(mean - rmean).max(), np.abs(var - rvar).max()
        print("predict_uncertain %s %s: mean %.3e var %.3e (min var %.3e)" % (q_shape, residual, e_m, e_v, var.min()))
        assert mean.shape == (n,) and var.shape == (n,) and mean.dtype == np.float64
        assert e_m <= 1e-8 and e_v <= 1e-8
        assert np.all(var >= 0.0)
        m0, v0 = post.predict_uncertain(xs, 0.0)
        pm, pv = post.predict(xs)
        print("   X_var = 0 against predict: mean %.3e var %.3e" % (np.abs(m0 - pm).max(), np.abs(v0 - pv).max()))
        assert np.abs(m0 - pm).max() <= 1e-8 and np.abs(v0 - pv).max() <= 1e-8
        # the model's methods are the posterior's numbers in the shapes of predict_f / predict_y
        fm, fv = m.predict_f_uncertain(xs, sv)
        ym, yv = m.predict_y_uncertain(xs, sv)
        assert fm.shape == (1, n) and np.array_equal(fm[0], mean) and np.array_equal(fv[0], var)
        assert np.array_equal(ym, fm) and np.allclose(yv, fv + 0.4, rtol=0, atol=1e-14)


# ------------------------------------------------------------------------------------------------ 4. SVGP
def test_svgp_fit_q_and_collapsed_bound_with_input_variances():
    """SVGP.fit_q(X_var=) writes the (m, S) optimal_q(stats=psi_statistics(..)) returns, collapsed_bound(X_var=) is
    collapsed_bound(stats=..), and without X_var both take the certain-input path."""
    N, M = 600, 32
    s = _variances(N, seed=5)
    with _settings():
        m, _, _, _ = _model(N, M, "fullrank", "float64")
        X, Y, var, k_var = m._closed_form_inputs()              # the model's own device data and scalars
        stats = m.gp.psi_statistics(X, s, Y)
        want_m, want_S = m.gp.optimal_q(X, Y, var, k_var, stats=stats)
        qm, S = m.fit_q(X_var=s)
        assert np.array_equal(qm, want_m) and np.array_equal(S, want_S)
        q = object.__getattribute__(m, "u")
        assert np.allclose(q.q_mu.value.reshape(1, M), qm, rtol=0, atol=1e-14)
        assert np.allclose(np.tril(q.q_sqrt.value), S, rtol=0, atol=1e-14)
        assert m.collapsed_bound(X_var=s) == m.gp.collapsed_bound(X, Y, var, k_var, stats=stats)
        assert m.collapsed_bound() == m.gp.collapsed_bound(X, Y, var, k_var)
        cm, cS = m.fit_q()
        wm, wS = m.gp.optimal_q(X, Y, var, k_var)
        assert np.array_equal(cm, wm) and np.array_equal(cS, wS)
        assert np.abs(cm - qm).max() > 1e-6                     # the input noise moved the optimum


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_uncertain_input_routes_refuse_what_they_do_not_cover():
    X, Y, Z = svgp_data(200, 32, 0)
    m, _, _, _ = _model(200, 32, "diagonal", "float64")
    post = m.posterior()
    xs = X[:10]
    for bad in (-0.1, np.full((200, 1), -1e-3), np.array([np.nan]), np.array([np.inf])):
        with pytest.raises(ValueError, match="X_var"):
            m.gp.psi_statistics(X, bad, Y)
    with pytest.raises(ValueError, match="X_var"):
        post.predict_uncertain(xs, -1.0)
    for bad in (np.zeros((200, 2)), np.zeros(2), np.zeros((199, 1)), np.zeros((1, 1, 1))):
        with pytest.raises(ValueError, match="X_var"):
            m.gp.psi_statistics(X, bad, Y)
    with pytest.raises(ValueError, match="X_var"):
        post.predict_uncertain(xs, np.zeros((10, 2)))
    with pytest.raises(ValueError):
        m.gp.psi_statistics(X, 0.1, Y[:-1])
    with pytest.raises(ValueError):
        m.gp.psi_statistics(np.zeros((200, 2)), 0.1, Y)
    with pytest.raises(ValueError):
        post.predict_uncertain(np.zeros((10, 2)), 0.1)
    with pytest.raises(ValueError, match="X_var"):
        m.fit_q(X_var=-1.0)

    class Other(hb.model.Model):
        def setUp(self, Z, kern):
            self.gp = hb.gp.SparseGP(kern=kern, z=Z)

    with pytest.raises(NotImplementedError, match="UnitRBF"):
        Other(Z=Z, kern=hb.gp.kernels.UnitMatern52(np.ones(1)), dtype="float64").gp.psi_statistics(X, 0.1, Y)
