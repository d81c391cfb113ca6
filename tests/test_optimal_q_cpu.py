"""Closed-form optimal q(u) / collapsed bound on the host: the new C entries exist and are bound, hb_sgp_stats_* validates
its arguments before any launch, and the numpy restatement the GPU tests lean on (tests/optimal_q_ref.py) is pinned by
the property that defines it -- q* maximises the ELBO written out term by term, and its value there is the collapsed
bound.  No HIP kernel runs here."""
import numpy as np
import pytest

import optimal_q_ref as R


# ---------------------------------------------------------------- C ABI
def test_stats_symbols_are_exported_and_bound():
    from henbun_amd import _lib

    names = _lib.declared_symbols()
    lib = _lib.lib()
    for n in ("hb_sgp_stats_f32", "hb_sgp_stats_f64", "hb_sgp_stats_ws_elems"):
        assert n in names
        assert lib.raw(n) is not None
    assert lib.raw("hb_version")() == 2


def _call(lib, suffix, **kw):
    a = dict(kind=0, X=1, Y=1, z=1, ell=1, dl=1, W=1, Wf=None, Phi=1, b=1, yy=1, a2sum=1, N=100, M=64, d=1, P=1, ws=None)
    a.update(kw)
    return lib.raw("hb_sgp_stats" + suffix)(a["kind"], a["X"], a["Y"], a["z"], a["ell"], a["dl"], a["W"], a["Wf"], a["Phi"],
                                            a["b"], a["yy"], a["a2sum"], a["N"], a["M"], a["d"], a["P"], a["ws"], None)


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
    (dict(X=None), "NULL input"),
    (dict(Y=None), "NULL input"),
    (dict(W=None), "NULL input"),
    (dict(Phi=None), "NULL output"),
    (dict(b=None), "NULL output"),
    (dict(yy=None), "NULL output"),
    (dict(a2sum=None), "NULL output"),
    (dict(ws=None), "workspace"),
])
def test_stats_entry_points_reject_bad_arguments(suffix, bad, word):
    """(the pointers are the integer 1: any launch would fault -- every case must return before one)"""
    from henbun_amd import _lib

    lib = _lib.lib()
    rc = _call(lib, suffix, **bad)
    assert rc < 0 and word in lib.last_error(), (rc, lib.last_error())


def test_stats_workspace_does_not_grow_with_N():
    from henbun_amd import _lib

    f = _lib.lib().raw("hb_sgp_stats_ws_elems")
    for M, P, b in [(512, 1, 4), (1024, 2, 4), (512, 1, 8), (96, 2, 4), (100, 1, 4), (512, 5, 4)]:
        w = [f(N, M, 1, P, b) for N in (100000, 1000000, 10000000)]
        assert w[0] > 0 and w[0] == w[1] == w[2]
        assert w[0] >= M * min(32768, (1 << 24) // M)          # one chunk of A
        assert w[0] < 2 * M * 32768 + (1 << 24)                # and a bounded set of partial tiles
        assert f(1, M, 1, P, b) < w[0]
    assert f(0, 512, 1, 1, 4) == 0


# ---------------------------------------------------------------- the algebra
def _problem(N=300, M=16, P=2, seed=3):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 8, (N, 1))
    Y = np.concatenate([np.sin(X + p) + 0.3 * rng.randn(N, 1) for p in range(P)], 1)
    z = np.linspace(0, 8, M)[:, None]
    ell = np.array([1.1])
    return X, Y, z, ell, rng


@pytest.mark.parametrize("residual", ["diagonal", "neglected"])
@pytest.mark.parametrize("noise_var, k_var", [(0.09, 1.0), (0.7, 2.3)])
def test_optimal_q_maximises_the_elbo_and_attains_the_collapsed_bound(residual, noise_var, k_var):
    X, Y, z, ell, rng = _problem()
    jitter = 1e-5
    N, M = X.shape[0], z.shape[0]
    Phi, b, yy, a2sum = R.stats(X, Y, z, ell, jitter)
    _, W = R.chol_factor(z, ell, jitter)
    A = R.A_of(W, z, X, ell)
    assert np.all(1.0 - (A * A).sum(0) >= 0.0)                 # so sum_j |1 - a2_j| == N - a2sum here
    m, S, s_diag, Lam = R.optimal_q(Phi, b, noise_var, k_var)
    assert np.all(np.diag(S) > 0) and np.array_equal(S, np.tril(S))
    bound = R.collapsed_bound(Phi, b, yy, a2sum, N, noise_var, k_var, residual)
    best = R.elbo_direct(m, S, A, Y, noise_var, k_var, residual)
    assert abs(best - bound) <= 1e-9 * abs(bound), (best, bound)
    for _ in range(20):
        dm = 0.05 * rng.randn(*m.shape)
        dS = np.tril(0.02 * rng.randn(M, M))
        S2 = S + dS
        S2[np.diag_indices(M)] = np.abs(np.diag(S2)) + 1e-12
        assert R.elbo_direct(m + dm, S2, A, Y, noise_var, k_var, residual) < best
    # the mean-field optimum: the best diagonal S, and below the full-rank optimum
    mf = R.elbo_direct(m, np.diag(s_diag), A, Y, noise_var, k_var, residual)
    assert mf <= best
    for _ in range(20):
        s2 = s_diag * np.exp(0.05 * rng.randn(M))
        assert R.elbo_direct(m, np.diag(s2), A, Y, noise_var, k_var, residual) < mf


def test_float32_restatement_is_close_to_float64():
    """(inducing points half a lengthscale apart, as in svgp_data: the float32 error of A = W K grows with |W| |K|)"""
    X, Y, z, _, _ = _problem(N=5000, M=16, P=1)
    ell = np.ones(1)
    _, W = R.chol_factor(z.astype(np.float32), ell.astype(np.float32), np.float32(1e-5))
    X32, Y32 = X.astype(np.float32), Y.astype(np.float32)
    s64 = R.stats_from_W(X32, Y32, z.astype(np.float32), ell.astype(np.float32), W)
    s32 = R.stats_from_W(X32, Y32, z, ell, W, dtype=np.float32, ksplit=512)
    assert np.abs(s32[0] - s64[0]).max() <= 1e-5 * np.abs(s64[0]).max()
    assert np.abs(s32[1] - s64[1]).max() <= 1e-5 * np.abs(s64[1]).max()
    assert np.array_equal(s32[0], s32[0].T)
