"""Exact GP regression by conjugate gradients on the host: the new C entries exist, are bound and validate their arguments
before any launch, and the numpy restatement the GPU tests lean on (tests/exact_gp_ref.py) is pinned against dense linear
algebra.  No HIP kernel runs here."""
import numpy as np
import pytest

import exact_gp_ref as E

NEW = ("hb_gram_matvec_f32", "hb_gram_matvec_f64", "hb_gram_matvec_chunk", "hb_gram_matvec_ws_elems", "hb_pcg_dot_f32",
       "hb_pcg_dot_f64", "hb_pcg_update_f32", "hb_pcg_update_f64", "hb_pcg_direction_f32", "hb_pcg_direction_f64")


# ---------------------------------------------------------------- C ABI
def test_exact_gp_symbols_are_exported_and_bound():
    import os

    import henbun_amd as hb
    from henbun_amd import _lib, hip_ops as H
    from henbun_amd.models import ExactGPR

    names = _lib.declared_symbols()
    lib = _lib.lib()
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "henbun_hip.h")).read()
    for n in NEW:
        assert n in names and n + "(" in header
        assert lib.raw(n) is not None
    assert lib.raw("hb_version")() == 2
    assert callable(H.gram_matvec) and callable(hb.gp.GP.condition) and callable(hb.gp.pcg_solve)
    assert issubclass(hb.gp.NotConverged, RuntimeError) and hasattr(hb.gp, "ExactPosterior")
    assert all(callable(getattr(ExactGPR, k)) for k in ("fit", "predict_f", "predict_y", "sample_functions"))


def test_chunk_and_workspace_size():
    """The chunk is a constant of the library; one chunk needs no workspace, up to 16 need chunks x S x n elements, more
    need 16 S n plus S n doubles: O(S n) whatever N."""
    from henbun_amd import _lib

    lib = _lib.lib()
    chunk = lib.raw("hb_gram_matvec_chunk")()
    ws = lib.raw("hb_gram_matvec_ws_elems")
    assert chunk >= 32 and chunk % 32 == 0
    for nbytes in (4, 8):
        assert ws(300, chunk, 17, nbytes) == 0 and ws(0, 10 * chunk, 3, nbytes) == 0
        assert ws(300, chunk + 1, 17, nbytes) == 2 * 17 * 300
        assert ws(300, 16 * chunk, 17, nbytes) == 16 * 17 * 300
        assert ws(300, 16 * chunk + 1, 17, nbytes) == (16 + 8 // nbytes) * 17 * 300
        assert ws(100000, 100000, 64, nbytes) == ws(100000, 10 ** 9, 64, nbytes) == (16 + 8 // nbytes) * 64 * 100000


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
@pytest.mark.parametrize("bad, word", [
    (dict(kind=1), "UnitRBF"),
    (dict(S=0), "extents"),
    (dict(d=0), "extents"),
    (dict(n=-1), "extents"),
    (dict(dl=2, d=3), "lengthscales"),
    (dict(x2=None, N=99), "symmetric"),
    (dict(shift=0.5), "shift"),
    (dict(V=None), "NULL"),
    (dict(out=None), "NULL"),
    (dict(N=5000, ws=None), "workspace"),
])
def test_gram_matvec_rejects_bad_arguments(suffix, bad, word):
    """(the pointers are the integer 1: any launch would fault -- every case must return before one)"""
    from henbun_amd import _lib

    lib = _lib.lib()
    a = dict(kind=0, x=1, x2=1, ell=1, dl=1, V=1, scale=1.0, shift=0.0, out=1, n=100, N=40, d=1, S=2, ws=1)
    a.update(bad)
    rc = lib.raw("hb_gram_matvec" + suffix)(a["kind"], a["x"], a["x2"], a["ell"], a["dl"], a["V"], a["scale"], a["shift"], a["out"],
                                            a["n"], a["N"], a["d"], a["S"], a["ws"], None)
    assert rc < 0 and word in lib.last_error() and "hb_gram_matvec" in lib.last_error(), (rc, lib.last_error())


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
def test_no_columns_is_not_an_error_and_not_a_launch(suffix):
    from henbun_amd import _lib

    rc = _lib.lib().raw("hb_gram_matvec" + suffix)(0, None, 1, 1, 1, 1, 1.0, 0.0, 1, 0, 40, 1, 2, None, None)
    assert rc == 0


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
def test_pcg_steps_reject_bad_arguments(suffix):
    from henbun_amd import _lib

    lib = _lib.lib()
    assert lib.raw("hb_pcg_dot" + suffix)(1, 1, None, 2, 10, None) < 0 and "hb_pcg_dot" in lib.last_error()
    assert lib.raw("hb_pcg_dot" + suffix)(1, 1, 1, 0, 10, None) < 0 and "extents" in lib.last_error()
    assert lib.raw("hb_pcg_update" + suffix)(1, 1, 1, None, 1, 1, 1, 2, 10, None) < 0 and "hb_pcg_update" in lib.last_error()
    assert lib.raw("hb_pcg_update" + suffix)(1, 1, 1, 1, 1, 1, 1, 2, 0, None) < 0 and "extents" in lib.last_error()
    assert lib.raw("hb_pcg_direction" + suffix)(1, None, None, 1, 1, 1, 1.0, 1.0, 1, 2, 10, None) < 0
    assert "hb_pcg_direction" in lib.last_error()


# ---------------------------------------------------------------- the restatement
@pytest.fixture(scope="module")
def case():
    X, Y, ell, k_var, noise_var = E.plane_case()
    solves = {}
    for rank in (0, 64, 128):
        C = E.factor(X, ell, rank) if rank else None
        solves[rank] = (C,) + E.pcg(X, ell, k_var, noise_var, Y.T, C, tol=1e-6)
    return X, Y, ell, k_var, noise_var, solves


def test_chunked_product_is_the_dense_product():
    rng = np.random.default_rng(1)
    x, x2 = rng.uniform(0, 3, (37, 3)), rng.uniform(0, 3, (150, 3))
    ell, V = np.array([0.7, 0.9, 1.1]), rng.standard_normal((5, 150))
    ref = 1.5 * V @ E.rbf(x2, x, ell)
    for chunk in (32, 64, 150, 2048):
        assert np.abs(E.matvec(x, x2, ell, V, 1.5, 0.0, chunk) - ref).max() <= 1e-12 * np.abs(V).sum(1).max()
    Vs = rng.standard_normal((5, 37))
    ref = 0.5 * Vs @ E.rbf(x, x, ell) + 0.01 * Vs
    assert np.abs(E.matvec(x, None, ell, Vs, 0.5, 0.01, 16) - ref).max() <= 1e-12 * np.abs(Vs).sum(1).max()


def test_pcg_solution_against_the_dense_cholesky(case):
    """|x - K^^-1 b| <= |K^^-1| |b - K^ x|: the error of the solution is within the bound its own true residual gives, at
    every rank, and the residual the solve reports is the true one."""
    from scipy.linalg import cho_factor, cho_solve

    X, Y, ell, k_var, noise_var, solves = case
    Kh = E.dense(X, ell, k_var, noise_var)
    ref = cho_solve(cho_factor(Kh, lower=True), Y).T
    inv_norm = 1.0 / np.linalg.eigvalsh(Kh)[0]
    for rank, (C, x, info) in solves.items():
        res = np.linalg.norm(Y.T - x @ Kh, axis=1)
        err = np.linalg.norm(x - ref, axis=1)
        print("rank %d: %d iterations, residual %.3e, error %.3e <= %.3e" % (rank, info["iterations"], info["residual"][0],
                                                                            err[0], inv_norm * res[0]))
        assert info["converged"] and info["residual"][0] <= 1e-6 * 1.0000001
        assert abs(info["residual"][0] - res[0] / np.linalg.norm(Y)) <= 1e-12
        assert err[0] <= inv_norm * res[0] * (1 + 1e-6) + 1e-12 * np.linalg.norm(ref)


def test_woodbury_inverse_is_the_inverse_of_the_dense_preconditioner(case):
    X, Y, ell, k_var, noise_var, solves = case
    rng = np.random.default_rng(2)
    r = rng.standard_normal((3, X.shape[0]))
    for k_v in (k_var, 2.5):
        for rank in (64, 128):
            C = solves[rank][0]
            assert C.shape == (rank, X.shape[0])
            P = k_v * C.T @ C + noise_var * np.eye(X.shape[0])
            ref = r @ np.linalg.inv(P)
            got = E.precond_apply(C, k_v, noise_var, r)
            assert np.abs(got - ref).max() <= 1e-9 * np.abs(ref).max()
    assert np.array_equal(E.precond_apply(None, k_var, noise_var, r), r)


def test_the_factor_is_a_pivoted_incomplete_cholesky(case):
    """K - C^T C is positive semi-definite with a zero diagonal at the pivots and a trace that falls with the rank."""
    X, Y, ell, k_var, noise_var, solves = case
    K = E.rbf(X, X, ell)
    tr = []
    for rank in (64, 128):
        C = solves[rank][0]
        D = K - C.T @ C
        tr.append(np.trace(D))
        assert np.linalg.eigvalsh(D)[0] >= -1e-10 and np.sort(np.abs(np.diag(D)))[rank - 1] <= 1e-12
    assert tr[1] < tr[0] < X.shape[0]


def test_the_preconditioner_cuts_the_iterations(case):
    """Measured with this restatement (numpy, float64, tol 1e-6): plain CG 223 iterations, rank 64: 56, rank 128: 15.
    Asserted: rank 64 at most half of plain CG, rank 128 no more than rank 64."""
    solves = case[-1]
    it = {rank: solves[rank][2]["iterations"] for rank in solves}
    print("iterations: plain %d, rank 64: %d, rank 128: %d" % (it[0], it[64], it[128]))
    assert it[64] <= it[0] / 2 and it[128] <= it[64]


def test_lockstep_rows_are_independent_solves(case):
    """Three right-hand sides in lockstep, one of them zero and one a multiple of another: each row is the solve it would
    be alone (a converged row stops moving; numpy's matrix products round differently for one row and for three, hence
    1e-9), the zero row stays zero."""
    X, Y, ell, k_var, noise_var, solves = case
    C, x1, info1 = solves[128]
    B = np.concatenate([Y.T, np.zeros((1, X.shape[0])), 3.0 * Y.T])
    x, info = E.pcg(X, ell, k_var, noise_var, B, C, tol=1e-6)
    assert info["converged"] and info["iterations"] == info1["iterations"]
    scale = np.abs(x1[0]).max()
    assert np.abs(x[0] - x1[0]).max() <= 1e-9 * scale and not np.any(x[1]) and np.abs(x[2] - 3.0 * x1[0]).max() <= 3e-9 * scale


def test_exact_pathwise_draws_interpolate_as_the_algebra_says():
    """With v = sqrt(k) K^^-1 (y - sqrt(k) g(X) - sqrt(s2) eps), the draw at the data plus its own noise draw is
    f(X) + sqrt(s2) eps = y - s2 K^^-1 (y - sqrt(k) g(X) - sqrt(s2) eps): K^ K^^-1 = I written out.  And with w = 0,
    eps = 0 every draw is the posterior mean."""
    X, Y, ell, k_var, noise_var = E.plane_case(200)
    k_var = 1.7
    rng = np.random.default_rng(3)
    S, L, N = 4, 32, X.shape[0]
    omega, w, eps = rng.standard_normal((L, 2)), rng.standard_normal((S, 2 * L)), rng.standard_normal((S, N))
    Kh = E.dense(X, ell, k_var, noise_var)
    solve = lambda B: np.linalg.solve(Kh, B.T).T
    import pathwise_ref as PR

    coef = E.pathwise_coefficients(X, Y[:, 0], ell, k_var, noise_var, omega, w, eps, solve)
    assert coef.shape == (S, 2 * L + N) and np.array_equal(coef[:, :2 * L], w / np.sqrt(L))
    f = PR.evaluate(X, omega, X, ell, coef, np.sqrt(k_var))
    prior = np.sqrt(k_var) * PR.evaluate(X, omega, None, ell, coef[:, :2 * L])
    want = Y.T - noise_var * solve(Y.T - prior - np.sqrt(noise_var) * eps)
    assert np.abs(f + np.sqrt(noise_var) * eps - want).max() <= 1e-9 * np.abs(want).max()
    coef0 = E.pathwise_coefficients(X, Y[:, 0], ell, k_var, noise_var, omega, 0 * w, 0 * eps, solve)
    xs = rng.uniform(0, 5, (50, 2))
    _, mean, _ = E.posterior(X, Y, ell, k_var, noise_var, xs)
    assert np.abs(PR.evaluate(xs, omega, X, ell, coef0, np.sqrt(k_var)) - mean).max() <= 1e-9 * np.abs(mean).max()
