"""Psi statistics (uncertain inputs) on the host: the new C entries exist and are bound, both entry families validate their
arguments before any launch, the workspace of the statistics does not grow with N, and the numpy restatement the GPU tests
lean on (tests/psi_ref.py) is pinned by what defines it -- the expectations by 60-node tensor Gauss-Hermite quadrature, the
zero-variance limit by the certain-input statistics, the shared-variance case by its product identity, and the whitened
tuple by the property that the collapsed bound is the ELBO at optimal_q's q(u).  No HIP kernel runs here.

Observed (printed by the tests): quadrature psi1 6.7e-16, psi2 6.7e-16, mean 2.1e-15, var 2.1e-14; zero variance Psi2
1.8e-16, C 4.0e-16, Phi 3.7e-15, b 1.5e-15; shared variance 8.0e-16; ELBO against the collapsed bound <= 1.6e-15 relative."""
import numpy as np
import pytest

import optimal_q_ref as R
import psi_ref as PR

ENTRIES = ("hb_sgp_psi_stats_f32", "hb_sgp_psi_stats_f64", "hb_sgp_psi_stats_ws_elems",
           "hb_sgp_psi_predict_f32", "hb_sgp_psi_predict_f64", "hb_sgp_psi_predict_ws_elems")


# ---------------------------------------------------------------- C ABI
def test_psi_symbols_are_declared_exported_and_bound():
    from henbun_amd import _lib
    from henbun_amd import hip_ops as H

    names = _lib.declared_symbols()
    lib = _lib.lib()
    for n in ENTRIES:
        assert n in names
        assert lib.raw(n) is not None
    for w in ("sgp_psi_stats", "sgp_psi_predict", "sgp_psi_stats_ws_elems", "sgp_psi_predict_ws_elems"):
        assert callable(getattr(H, w))
    assert lib.raw("hb_version")() == 2


def _stats_call(lib, suffix, **kw):
    a = dict(kind=0, Xm=1, Xv=1, Y=1, z=1, ell=1, dl=1, Psi2=1, C=1, yy=1, N=100, M=64, d=1, P=1, ws=None)
    a.update(kw)
    return lib.raw("hb_sgp_psi_stats" + suffix)(a["kind"], a["Xm"], a["Xv"], a["Y"], a["z"], a["ell"], a["dl"], a["Psi2"],
                                                a["C"], a["yy"], a["N"], a["M"], a["d"], a["P"], a["ws"], None)


def _predict_call(lib, suffix, **kw):
    a = dict(kind=0, Xm=1, Xv=1, z=1, ell=1, dl=1, beta=1, Q=1, e1=1, e2=1, n=100, M=64, d=1, ws=None)
    a.update(kw)
    return lib.raw("hb_sgp_psi_predict" + suffix)(a["kind"], a["Xm"], a["Xv"], a["z"], a["ell"], a["dl"], a["beta"], a["Q"],
                                                  a["e1"], a["e2"], a["n"], a["M"], a["d"], a["ws"], None)


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
@pytest.mark.parametrize("bad, word", [
    (dict(kind=1), "UnitRBF"),
    (dict(kind=7), "UnitRBF"),
    (dict(N=0), "extents"),
    (dict(N=-3), "extents"),
    (dict(M=0), "extents"),
    (dict(d=0), "extents"),
    (dict(P=0), "extents"),
    (dict(dl=2, d=3), "lengthscales"),
    (dict(Xm=None), "NULL input"),
    (dict(Xv=None), "NULL input"),
    (dict(Y=None), "NULL input"),
    (dict(z=None), "NULL input"),
    (dict(ell=None), "NULL input"),
    (dict(Psi2=None), "NULL output"),
    (dict(C=None), "NULL output"),
    (dict(yy=None), "NULL output"),
    (dict(ws=None), "workspace"),
    (dict(M=46341, ws=16), "too large"),
])
def test_psi_stats_rejects_bad_arguments(suffix, bad, word):
    """(the pointers are the integer 1: any launch would fault -- every case must return before one)"""
    from henbun_amd import _lib

    lib = _lib.lib()
    rc = _stats_call(lib, suffix, **bad)
    assert rc < 0 and word in lib.last_error(), (rc, lib.last_error())


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
@pytest.mark.parametrize("bad, word", [
    (dict(kind=1), "UnitRBF"),
    (dict(n=-1), "extents"),
    (dict(M=0), "extents"),
    (dict(d=0), "extents"),
    (dict(dl=2, d=3), "lengthscales"),
    (dict(Xm=None), "NULL input"),
    (dict(Xv=None), "NULL input"),
    (dict(z=None), "NULL input"),
    (dict(ell=None), "NULL input"),
    (dict(beta=None), "NULL input"),
    (dict(Q=None), "NULL input"),
    (dict(e1=None), "NULL output"),
    (dict(e2=None), "NULL output"),
    (dict(ws=None), "workspace"),
    (dict(M=46341, ws=16), "too large"),
])
def test_psi_predict_rejects_bad_arguments(suffix, bad, word):
    from henbun_amd import _lib

    lib = _lib.lib()
    assert lib.raw("hb_sgp_psi_predict_ws_elems")(100, 64, 1, 4) > 0       # so a NULL workspace is refused
    rc = _predict_call(lib, suffix, **bad)
    assert rc < 0 and word in lib.last_error(), (rc, lib.last_error())


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
def test_psi_predict_of_no_points_returns_without_a_launch(suffix):
    from henbun_amd import _lib

    assert _predict_call(_lib.lib(), suffix, n=0) == 0
    assert _lib.lib().raw("hb_sgp_psi_predict_ws_elems")(0, 64, 1, 4) == 0


def test_psi_stats_workspace_does_not_grow_with_N():
    from henbun_amd import _lib

    f = _lib.lib().raw("hb_sgp_psi_stats_ws_elems")
    for M, P, b in [(512, 1, 4), (1024, 2, 4), (512, 1, 8), (33, 3, 4), (1, 1, 8), (128, 5, 4)]:
        w = [f(N, M, 2, P, b) for N in (100000, 1000000, 10000000)]
        assert w[0] > 0 and w[0] == w[1] == w[2]
        # the partial tiles of at most 4096 workgroups, in elements of the storage type, and the partials of C
        assert w[0] <= (8 // b) * (4096 * 4096 + 4096 * P * M + 128)
        assert f(1, M, 2, P, b) == w[0]
    assert f(0, 512, 1, 1, 4) == 0
    assert f(100000, 512, 1, 1, 4) == 2 * f(100000, 512, 1, 1, 8)


# ---------------------------------------------------------------- the restatement against what defines it
def _small(seed=5, N=6, M=5, d=2):
    rng = np.random.RandomState(seed)
    ell = np.array([0.8, 1.3])[:d]
    z = rng.uniform(-1.5, 1.5, (M, d))
    mu = rng.uniform(-2.0, 2.0, (N, d))
    s = rng.uniform(0.0, 0.36, (N, d)) * ell ** 2
    s[0] = 0.0                       # exact zeros: a whole row, and one dimension of another
    s[1, 0] = 0.0
    s[2, 1] = 0.0
    s[3] = 0.36 * ell ** 2           # the widest input the 60-node rule resolves to 1e-12: its error falls as (c / (1 + c))^60, c = 2 s / l^2
    return mu, s, z, ell, rng


def test_restatement_agrees_with_gauss_hermite_quadrature():
    """psi1, psi2 and the predictive mean / variance against 60-node tensor Gauss-Hermite quadrature, d = 2, M = 5, within
    1e-12; the variances include exact zeros (a whole point, and single dimensions)."""
    mu, s, z, ell, rng = _small()
    M = z.shape[0]
    jitter = 1e-3
    _, W = R.chol_factor(z, ell, jitter)
    m = rng.randn(M)
    S = np.tril(0.3 * rng.randn(M, M)) + np.eye(M)
    p1, p2 = PR.psi1(mu, s, z, ell), PR.psi2(mu, s, z, ell)
    worst = dict(psi1=0.0, psi2=0.0, mean=0.0, var=0.0)
    for residual, Sq in (("diagonal", S), ("neglected", S), ("diagonal", np.abs(np.diag(S)))):
        mean, var = PR.predict_uncertain(mu, s, z, ell, W, m, Sq, 1.7, residual)
        Sm = np.diag(Sq) if Sq.ndim == 1 else Sq
        rho = 1.0 if residual == "diagonal" else 0.0
        for n in range(mu.shape[0]):
            k = lambda x: R.rbf(z, x, ell).T                                            # [K, M]
            q1 = PR.gauss_hermite_expect(k, mu[n], s[n])
            q2 = PR.gauss_hermite_expect(lambda x: k(x)[:, :, None] * k(x)[:, None, :], mu[n], s[n])

            def moments(x):
                A = W @ R.rbf(z, x, ell)                                                # [M, K]
                cm = np.sqrt(1.7) * (m @ A)
                cv = 1.7 * (rho * (1.0 - (A * A).sum(0)) + ((Sm.T @ A) ** 2).sum(0))
                return np.stack([cm, cv + cm * cm], 1)

            qm, qsecond = PR.gauss_hermite_expect(moments, mu[n], s[n])
            worst["psi1"] = max(worst["psi1"], np.abs(p1[n] - q1).max())
            worst["psi2"] = max(worst["psi2"], np.abs(p2[n] - q2).max())
            worst["mean"] = max(worst["mean"], abs(mean[n] - qm))
            worst["var"] = max(worst["var"], abs(var[n] - (qsecond - qm * qm)))
    print("restatement against quadrature:", worst)
    assert all(v <= 1e-12 for v in worst.values()), worst


def test_zero_variance_is_the_certain_input_statistics():
    """X_var = 0: Psi2 = K K^T, C = (K Y)^T, and the whitened tuple that of optimal_q_ref, within 1e-13 of the largest
    entry (inducing points one lengthscale apart, jitter 1e-3: W has entries of order 10)."""
    rng = np.random.RandomState(2)
    N, M, P = 200, 12, 2
    z = np.linspace(0.0, 11.0, M)[:, None]
    ell = np.array([1.0])
    X = rng.uniform(0.0, 11.0, (N, 1))
    Y = rng.randn(N, P)
    Psi2, C, yy = PR.stats_raw(X, np.zeros_like(X), Y, z, ell)
    K = R.rbf(z, X, ell)
    e2, eC = np.abs(Psi2 - K @ K.T).max() / np.abs(K @ K.T).max(), np.abs(C - (K @ Y).T).max() / np.abs(K @ Y).max()
    got, ref = PR.stats(X, np.zeros_like(X), Y, z, ell, 1e-3), R.stats(X, Y, z, ell, 1e-3)
    ePhi, eb = np.abs(got[0] - ref[0]).max() / np.abs(ref[0]).max(), np.abs(got[1] - ref[1]).max() / np.abs(ref[1]).max()
    print("zero variance: Psi2 %.2e C %.2e Phi %.2e b %.2e a2sum %.2e" % (e2, eC, ePhi, eb, abs(got[3] / ref[3] - 1)))
    assert max(e2, eC, ePhi, eb) <= 1e-13 and abs(got[3] - ref[3]) <= 1e-13 * ref[3]
    assert np.allclose(got[2], ref[2], rtol=1e-15, atol=0)


def test_shared_variance_identity():
    """One variance for all points: Psi2 = c H o (K' K'^T) with l'^2 = l^2 + 2 s, c = prod (1 + 2 s / l^2)^-1/2 and
    H = exp(-1/4 sum dz^2 (1 / l^2 - 1 / l'^2)), within 1e-13 of the largest entry."""
    rng = np.random.RandomState(4)
    N, M, d = 150, 9, 3
    ell = np.array([0.7, 1.0, 1.6])
    z = rng.uniform(-2, 2, (M, d))
    mu = rng.uniform(-3, 3, (N, d))
    s = np.array([0.2, 0.0, 0.9])
    Psi2, _, _ = PR.stats_raw(mu, np.broadcast_to(s, (N, d)), np.zeros((N, 1)), z, ell)
    l2p = ell ** 2 + 2.0 * s
    Kp = R.rbf(z, mu, np.sqrt(l2p))
    dz2 = (z[:, None, :] - z[None, :, :]) ** 2
    Hm = np.exp(-0.25 * (dz2 * (1.0 / ell ** 2 - 1.0 / l2p)).sum(-1))
    ref = np.prod(1.0 + 2.0 * s / ell ** 2) ** -0.5 * Hm * (Kp @ Kp.T)
    err = np.abs(Psi2 - ref).max() / np.abs(ref).max()
    print("shared variance identity: %.2e" % err)
    assert err <= 1e-13


@pytest.mark.parametrize("residual", ["diagonal", "neglected"])
@pytest.mark.parametrize("noise_var, k_var", [(0.09, 1.0), (0.7, 2.3)])
def test_collapsed_bound_with_psi_statistics_is_the_elbo_at_optimal_q(residual, noise_var, k_var):
    """With the psi statistics in the tuple, optimal_q's (m, S) maximises the ELBO under uncertain inputs written out
    term by term from the per-point psi1_n, psi2_n, and its value there is the collapsed bound."""
    rng = np.random.RandomState(7)
    N, M, P, d = 120, 8, 2, 2
    ell = np.array([0.9, 1.2])
    z = rng.uniform(-2, 2, (M, d))
    mu = rng.uniform(-2.5, 2.5, (N, d))
    s = rng.uniform(0.0, 0.36, (N, d)) * ell ** 2
    s[::7] = 0.0
    Y = np.stack([np.sin(mu.sum(1) + p) for p in range(P)], 1) + 0.3 * rng.randn(N, P)
    jitter = 1e-3
    _, W = R.chol_factor(z, ell, jitter)
    Phi, b, yy, a2sum = PR.stats(mu, s, Y, z, ell, W=W)
    assert N - a2sum > 0
    m, S, s_diag, _ = R.optimal_q(Phi, b, noise_var, k_var)
    bound = R.collapsed_bound(Phi, b, yy, a2sum, N, noise_var, k_var, residual)
    best = PR.elbo_direct(m, S, mu, s, Y, z, ell, W, noise_var, k_var, residual)
    print("ELBO at optimal_q %.12f, collapsed bound %.12f (%.1e relative)" % (best, bound, abs(best / bound - 1)))
    assert abs(best - bound) <= 1e-9 * abs(bound)
    for _ in range(10):
        dm = 0.05 * rng.randn(*m.shape)
        S2 = S + np.tril(0.02 * rng.randn(M, M))
        S2[np.diag_indices(M)] = np.abs(np.diag(S2)) + 1e-12
        assert PR.elbo_direct(m + dm, S2, mu, s, Y, z, ell, W, noise_var, k_var, residual) < best
    assert PR.elbo_direct(m, np.diag(s_diag), mu, s, Y, z, ell, W, noise_var, k_var, residual) <= best
