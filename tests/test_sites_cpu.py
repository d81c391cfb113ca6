"""Natural-gradient fit of q(u) on the host: the new C entries exist, are bound and validate their arguments before any
launch, and the numpy restatement the GPU tests lean on (tests/sites_ref.py) is pinned three ways -- the Gaussian step is
optimal_q, the converged q is a stationary point of the ELBO written out term by term, and the 20-node rule has converged
at the marginals the iteration meets.  No HIP kernel runs here."""
import numpy as np
import pytest

import optimal_q_ref as R
import sites_ref as SR

NEW = ("hb_sgp_wstats_f32", "hb_sgp_wstats_f64", "hb_sgp_wstats_ws_elems", "hb_lik_sites_f32", "hb_lik_sites_f64",
       "hb_lik_sites_ws_elems", "hb_lik_predict_f32", "hb_lik_predict_f64")


# ---------------------------------------------------------------- C ABI
def test_site_symbols_are_exported_and_bound():
    from henbun_amd import _lib

    names = _lib.declared_symbols()
    lib = _lib.lib()
    for n in NEW:
        assert n in names
        assert lib.raw(n) is not None
    assert lib.raw("hb_version")() == 2


def test_likelihood_classes_carry_the_abi_ids():
    import henbun_amd as hb
    from henbun_amd import hip_ops as H

    L = hb.likelihoods
    assert (L.Gaussian(0.3).lik_id, L.Bernoulli().lik_id, L.Poisson().lik_id) == (0, 1, 2)
    assert (H.LIK_GAUSSIAN, H.LIK_BERNOULLI, H.LIK_POISSON) == (SR.GAUSSIAN, SR.BERNOULLI, SR.POISSON) == (0, 1, 2)
    assert L.Gaussian(0.3).param == 0.3
    with pytest.raises(ValueError):
        L.Gaussian(0.0)


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
@pytest.mark.parametrize("bad, word", [
    (dict(lik=3), "unknown likelihood"),
    (dict(lik=-1), "unknown likelihood"),
    (dict(N=-1), "negative N"),
    (dict(lik=0, param=0.0), "variance"),
    (dict(lik=0, param=-2.0), "variance"),
])
def test_lik_entry_points_reject_bad_arguments(suffix, bad, word):
    """(the pointers are the integer 1: any launch would fault -- every case must return before one)"""
    from henbun_amd import _lib

    lib = _lib.lib()
    a = dict(lik=1, N=10, param=1.0)
    a.update(bad)
    rc = lib.raw("hb_lik_sites" + suffix)(a["lik"], 1, 1, 1, 1.0, 1.0, a["param"], 1, 1, 1, a["N"], 1, None)
    assert rc < 0 and word in lib.last_error(), (rc, lib.last_error())
    rc = lib.raw("hb_lik_predict" + suffix)(a["lik"], 1, 1, a["param"], 1, 1, a["N"], None)
    assert rc < 0 and word in lib.last_error(), (rc, lib.last_error())


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
@pytest.mark.parametrize("bad, word", [
    (dict(kind=1), "UnitRBF"),
    (dict(N=0), "extents"),
    (dict(M=0), "extents"),
    (dict(dl=2, d=3), "lengthscales"),
    (dict(w=None), "NULL input"),
    (dict(r=None), "NULL input"),
    (dict(Phi=None), "NULL output"),
    (dict(tr=None), "NULL output"),
    (dict(w=4), "alignment"),
    (dict(ws=None), "workspace"),
])
def test_wstats_entry_points_reject_bad_arguments(suffix, bad, word):
    from henbun_amd import _lib

    lib = _lib.lib()
    a = dict(kind=0, X=16, w=16, r=16, z=16, ell=16, dl=1, W=16, Wf=None, Phi=16, b=16, tr=16, N=100, M=64, d=1, ws=None)
    a.update(bad)
    rc = lib.raw("hb_sgp_wstats" + suffix)(a["kind"], a["X"], a["w"], a["r"], a["z"], a["ell"], a["dl"], a["W"], a["Wf"],
                                           a["Phi"], a["b"], a["tr"], a["N"], a["M"], a["d"], a["ws"], None)
    assert rc < 0 and word in lib.last_error() and "hb_sgp_wstats" in lib.last_error(), (rc, lib.last_error())


def test_workspaces_do_not_grow_with_N():
    from henbun_amd import _lib

    f, g, h = (_lib.lib().raw(n) for n in ("hb_sgp_wstats_ws_elems", "hb_sgp_stats_ws_elems", "hb_lik_sites_ws_elems"))
    for M, b in [(512, 4), (160, 4), (100, 8)]:
        w = [f(N, M, 1, b) for N in (100000, 1000000, 10000000)]
        assert w[0] > 0 and w[0] == w[1] == w[2] == g(1000000, M, 1, 1, b)
    assert h(1) == 1 and h(257) == 2 and h(10 ** 6) == h(10 ** 8) <= 1024


# ---------------------------------------------------------------- the restatement
def test_gaussian_step_from_the_prior_is_optimal_q_and_attains_the_collapsed_bound():
    X, y, Z = SR.problem(SR.GAUSSIAN)
    s2 = 0.4
    for residual in ("diagonal", "neglected"):
        m, S, info = SR.natgrad(X, y, Z, SR.ELL, SR.JITTER, SR.GAUSSIAN, s2, SR.K_VAR, residual, steps=1, tol=0.0)
        Phi, b, yy, a2 = R.stats(X, y, Z, SR.ELL, SR.JITTER)
        rm, rS, _, _ = R.optimal_q(Phi, b, s2, SR.K_VAR)
        assert info["steps"] == 1 and len(info["elbo"]) == 2
        assert np.abs(m - rm).max() <= 1e-10 * np.abs(rm).max()
        assert np.abs(S @ S.T - rS @ rS.T).max() <= 1e-10 * np.abs(rS @ rS.T).max()
        _, W = R.chol_factor(Z, SR.ELL, SR.JITTER)
        A = R.A_of(W, Z, X, SR.ELL)
        a2 = a2 if residual == "neglected" else X.shape[0] - np.abs(1.0 - (A * A).sum(0)).sum()   # sum_j |1 - a2_j|
        bound = R.collapsed_bound(Phi, b, yy, a2, X.shape[0], s2, SR.K_VAR, residual)
        assert abs(info["elbo"][1] - bound) <= 1e-10 * abs(bound), (info["elbo"], bound)
        assert info["residual"][1] <= 1e-12                       # a fixed point after one step


@pytest.fixture(scope="module", params=[SR.BERNOULLI, SR.POISSON])
def converged(request):
    lik = request.param
    X, y, Z = SR.problem(lik)
    _, W = R.chol_factor(Z, SR.ELL, SR.JITTER)
    A = R.A_of(W, Z, X, SR.ELL)
    m, S, info = SR.natgrad(X, y, Z, SR.ELL, SR.JITTER, lik, 1.0, SR.K_VAR, steps=40, tol=0.0)
    return lik, X, y, Z, A, m, S, info


def _fd_gradient(fun, m, S, entries, h=1e-4):
    gm = np.zeros(m.size)
    for i in range(m.size):
        d = np.zeros_like(m)
        d.reshape(-1)[i] = h
        gm[i] = (fun(m + d, S) - fun(m - d, S)) / (2 * h)
    gS = []
    for (i, j) in entries:
        d = np.zeros_like(S)
        d[i, j] = h
        gS.append((fun(m, S + d) - fun(m, S - d)) / (2 * h))
    return gm, np.asarray(gS)


def test_converged_q_is_a_stationary_point_of_the_elbo(converged):
    """Central finite differences of the ELBO written out term by term (sites_ref.elbo, no Lambda anywhere) with respect
    to every m_i and a dozen entries of S at the converged q: <= 1e-5 of the largest gradient entry at the prior."""
    lik, X, y, Z, A, m, S, info = converged
    M = Z.shape[0]
    fun = lambda mm, SS: SR.elbo(mm, SS, A, y, lik, 1.0, SR.K_VAR)
    entries = [(0, 0), (5, 5), (17, 17), (31, 31), (1, 0), (6, 5), (16, 15), (31, 30), (9, 3), (20, 12), (31, 0), (25, 24)]
    g0m, g0S = _fd_gradient(fun, np.zeros((1, M)), np.eye(M), entries)
    gm, gS = _fd_gradient(fun, m, S, entries)
    scale = max(np.abs(g0m).max(), np.abs(g0S).max())
    print("lik %d: |grad| at the prior %.3e; at the converged q: m %.3e S %.3e; residual %.2e; elbo %.3f -> %.3f"
          % (lik, scale, np.abs(gm).max(), np.abs(gS).max(), info["residual"][-1], info["elbo"][0], info["elbo"][-1]))
    assert abs(fun(m, S) - info["elbo"][-1]) <= 1e-10 * abs(info["elbo"][-1])
    assert np.abs(gm).max() <= 1e-5 * scale
    assert np.abs(gS).max() <= 1e-5 * scale
    assert info["residual"][-1] <= 1e-6       # its floor is the round trip Lambda -> S -> marginals, about 5e-9 here
    assert np.all(np.diff(info["elbo"]) >= -1e-9 * np.abs(info["elbo"][-1]))      # monotone at rho = 1


def test_twenty_nodes_have_converged_at_the_marginals_of_the_iteration(converged):
    lik, X, y, Z, A, m, S, info = converged
    worst = 0.0
    for mu, v in info["marginals"][1:9]:      # after the first step (the prior's v = k_var is not met again)
        a, b = SR.sites(lik, y, mu, v, nodes=20), SR.sites(lik, y, mu, v, nodes=200)
        for p, q in zip(a, b):
            worst = max(worst, float(np.abs(p - q).max() / max(np.abs(q).max(), 1.0)))
        pa, pb = SR.predict_y(lik, mu, v, nodes=20), SR.predict_y(lik, mu, v, nodes=200)
        worst = max(worst, float(np.abs(pa[0] - pb[0]).max()))
    vs = np.concatenate([v for _, v in info["marginals"][1:9]])
    print("lik %d: 20 against 200 nodes %.2e; v in [%.3g, %.3g] after the first step" % (lik, worst, vs.min(), vs.max()))
    assert worst <= 1e-10


def test_damped_iteration_reaches_the_same_elbo(converged):
    """(the ELBO is flat to second order at the fixed point, so it is the quantity two routes agree on to round-off)"""
    lik, X, y, Z, A, m, S, info = converged
    m2, S2, info2 = SR.natgrad(X, y, Z, SR.ELL, SR.JITTER, lik, 1.0, SR.K_VAR, steps=60, rho=0.5, tol=0.0)
    assert abs(info2["elbo"][-1] - info["elbo"][-1]) <= 1e-10 * abs(info["elbo"][-1])
