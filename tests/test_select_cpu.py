"""Greedy selection of inducing points on the host: the numpy restatement the GPU tests lean on (tests/greedy_ref.py) is
pinned by identities it does not use, the new C entries exist and validate their arguments before any launch, and the
workspace promise covers the history.  No HIP kernel runs here."""
import numpy as np
import pytest

import greedy_ref as GR
import optimal_q_ref as R


# ---------------------------------------------------------------- the restatement
def _problem(N=400, d=2, seed=5):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 6, (N, d))
    Y = np.sin(X.sum(1, keepdims=True)) + 0.3 * rng.randn(N, 1)
    ell = np.array([1.0]) if d == 1 else np.array([0.9, 1.2])
    return X, Y, ell


@pytest.mark.parametrize("d, M", [(1, 8), (2, 24)])
def test_restatement_meets_the_identities_of_a_pivoted_cholesky(d, M):
    X, Y, ell = _problem(d=d)
    N = X.shape[0]
    idx, pivots, count, trace = GR.select(X, M, ell, 0.0)
    assert count == M and idx[0] == 0 and pivots[0] == 1.0
    assert len(set(idx.tolist())) == M and idx.min() >= 0 and idx.max() < N
    assert np.all(np.diff(pivots) <= 0)
    Z = X[idx]
    # prod_j pivots_j = det K(Z, Z): the pivots are the squared diagonal of the Cholesky factor of the pivoted matrix
    sign, logdet = np.linalg.slogdet(R.rbf(Z, Z, ell))
    assert sign > 0 and abs(np.log(pivots).sum() - logdet) <= 1e-8 * max(1.0, abs(logdet))
    # trace = N - a2sum of the sufficient statistics at zero jitter: tr(K_XX - K_XZ K_ZZ^-1 K_ZX)
    a2sum = R.stats(X, Y, Z, ell, 0.0)[3]
    assert abs(trace - (N - a2sum)) <= 1e-7 * N
    # the replay of the chosen sequence is the selection itself, and it was greedy at every step
    rp, rmax, rtrace = GR.replay(X, idx, ell)
    assert np.array_equal(rp, pivots) and np.array_equal(rp, rmax) and rtrace == trace
    rp2, _, rtrace2 = GR.replay(X, idx, ell, order="reversed")
    assert np.abs(rp2 - rp).max() <= 1e-10 and abs(rtrace2 - rtrace) <= 1e-8


def test_restatement_tie_rule_and_early_stop():
    rng = np.random.RandomState(0)
    base = np.arange(8)[:, None] * 6.0
    X = np.repeat(base, 50, axis=0)[rng.permutation(400)]
    idx, pivots, count, trace = GR.select(X, 16, np.ones(1), 1e-3)
    assert count == 8 and np.all(idx[8:] == -1) and np.all(pivots[8:] == 0) and np.all(idx[:8] >= 0)
    assert idx[0] == 0
    assert sorted(X[idx[:8], 0].tolist()) == base[:, 0].tolist()
    # each chosen point is the FIRST row holding its value
    for i in idx[:8]:
        assert i == np.flatnonzero(X[:, 0] == X[i, 0])[0]
    assert trace < 1e-6 * 400
    assert GR.select(X, 4, np.ones(1), 1.0)[2] == 0          # kdiag = 1 <= threshold: nothing is chosen
    assert GR.select(X, 4, np.ones(1), 1.0)[3] == 400.0


def test_float32_restatement_parts_from_float64_but_reaches_a_similar_trace():
    """Why the GPU tests replay the device's choice instead of comparing indices with a reference."""
    X, _ = GR.clustered()
    i64, _, c64, t64 = GR.select(X, 64, np.ones(1), 0.0)
    i32, _, c32, t32 = GR.select(X, 64, np.ones(1), 0.0, dtype=np.float32)
    assert c64 == c32 == 64
    first = int(np.flatnonzero(i64 != i32)[0]) if np.any(i64 != i32) else 64
    print("clustered 1-D: float32 and float64 selections differ first at step %d; traces %.4g / %.4g" % (first, t32, t64))
    assert t64 < 1e-2 and t32 < 1e-2


# ---------------------------------------------------------------- C ABI
def test_select_symbols_are_exported_and_bound():
    from henbun_amd import _lib

    names = _lib.declared_symbols()
    lib = _lib.lib()
    for n in ("hb_sgp_select_f32", "hb_sgp_select_f64", "hb_sgp_select_ws_elems"):
        assert n in names
        assert lib.raw(n) is not None
    assert lib.raw("hb_version")() == 2


def _call(lib, suffix, **kw):
    a = dict(kind=0, X=1, ell=1, dl=1, N=100, M=16, d=1, threshold=0.0, idx=1, pivots=1, count=1, trace=1, ws=16)
    a.update(kw)
    return lib.raw("hb_sgp_select" + suffix)(a["kind"], a["X"], a["ell"], a["dl"], a["N"], a["M"], a["d"], a["threshold"],
                                             a["idx"], a["pivots"], a["count"], a["trace"], a["ws"], None)


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
@pytest.mark.parametrize("bad, word", [
    (dict(kind=1), "UnitRBF"),
    (dict(kind=2), "UnitRBF"),
    (dict(N=0), "extents"),
    (dict(N=-5), "extents"),
    (dict(M=0), "extents"),
    (dict(M=101), "extents"),
    (dict(d=0), "extents"),
    (dict(dl=2, d=3), "lengthscales"),
    (dict(dl=0), "lengthscales"),
    (dict(threshold=-1e-9), "threshold"),
    (dict(threshold=float("nan")), "threshold"),
    (dict(X=None), "NULL input"),
    (dict(ell=None), "NULL input"),
    (dict(idx=None), "NULL output"),
    (dict(pivots=None), "NULL output"),
    (dict(count=None), "NULL output"),
    (dict(trace=None), "NULL output"),
    (dict(ws=None), "workspace"),
    (dict(ws=20), "workspace"),
])
def test_select_entry_points_reject_bad_arguments(suffix, bad, word):
    """(the pointers are small integers: any launch would fault -- every case must return before one)"""
    from henbun_amd import _lib

    lib = _lib.lib()
    rc = _call(lib, suffix, **bad)
    assert rc < 0 and word in lib.last_error(), (rc, lib.last_error())


def test_select_workspace_holds_the_history():
    from henbun_amd import _lib

    f = _lib.lib().raw("hb_sgp_select_ws_elems")
    for N, M, b in [(1, 1, 4), (100, 16, 4), (4096, 128, 8), (1000000, 512, 4), (1000001, 1024, 8)]:
        w = f(N, M, 1, b)
        assert w >= M * N + N                                    # the history and dvar
        assert w <= (M + 1) * (N + 63) + 3 * 4096                # and no more than padding and the arg-max partials
        assert f(N, M, 3, b) == w
    assert f(0, 16, 1, 4) == 0 and f(100, 0, 1, 4) == 0
