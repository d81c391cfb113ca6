"""Pathwise posterior function draws on the host: the new C entries exist, are bound and validate their arguments before
any launch, and the numpy restatement the GPU tests lean on (tests/pathwise_ref.py) is pinned twice -- its mean is
predict_f's mean, and its covariance at fixed frequencies tends to the exact conditional at the 1 / sqrt(L) rate.  No HIP
kernel runs here."""
import numpy as np
import pytest

import optimal_q_ref as R
import pathwise_ref as PR
import sites_ref as SR

NEW = ("hb_sgp_pathwise_f32", "hb_sgp_pathwise_f64")


# ---------------------------------------------------------------- C ABI
def test_pathwise_symbols_are_exported_and_bound():
    import os

    import henbun_amd as hb
    from henbun_amd import _lib, hip_ops as H

    names = _lib.declared_symbols()
    lib = _lib.lib()
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "henbun_hip.h")).read()
    for n in NEW:
        assert n in names and n + "(" in header
        assert lib.raw(n) is not None
    assert lib.raw("hb_version")() == 2
    assert callable(H.sgp_pathwise) and hasattr(hb.gp, "PathwiseDraws")
    assert callable(hb.gp.SparseGP.pathwise_draws)
    from henbun_amd.models import SVGP, SVGPLik

    assert SVGPLik.sample_functions is SVGP.sample_functions


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
@pytest.mark.parametrize("bad, word", [
    (dict(kind=1), "UnitRBF"),
    (dict(L=0), "extents"),
    (dict(S=0), "extents"),
    (dict(n=-1), "extents"),
    (dict(dl=2, d=3), "lengthscales"),
    (dict(coef=None), "NULL"),
    (dict(out=None), "NULL"),
])
def test_pathwise_entry_points_reject_bad_arguments(suffix, bad, word):
    """(the pointers are the integer 1: any launch would fault -- every case must return before one)"""
    from henbun_amd import _lib

    lib = _lib.lib()
    a = dict(kind=0, x=1, omega=1, z=1, ell=1, dl=1, coef=1, scale=1.0, out=1, n=100, L=8, M=4, d=1, S=2)
    a.update(bad)
    rc = lib.raw("hb_sgp_pathwise" + suffix)(a["kind"], a["x"], a["omega"], a["z"], a["ell"], a["dl"], a["coef"], a["scale"],
                                             a["out"], a["n"], a["L"], a["M"], a["d"], a["S"], None)
    assert rc < 0 and word in lib.last_error() and "hb_sgp_pathwise" in lib.last_error(), (rc, lib.last_error())


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
def test_no_points_is_not_an_error_and_not_a_launch(suffix):
    from henbun_amd import _lib

    rc = _lib.lib().raw("hb_sgp_pathwise" + suffix)(0, 1, 1, None, 1, 1, 1, 1.0, 1, 0, 8, 0, 1, 2, None)
    assert rc == 0


# ---------------------------------------------------------------- the restatement
def test_the_mean_of_the_restatement_is_predict_fs_mean():
    """With w = 0 and eps = 0 every draw is the mean: sqrt(k_var) m A(x), A = W K formed in float64.  The v form and the A
    form differ by cond(K(z, z)) 2^-53: 1e-8 of max|mean|."""
    X, _, Z = SR.problem(SR.BERNOULLI)
    rng = np.random.default_rng(0)
    M, L, S = Z.shape[0], 64, 3
    _, W = R.chol_factor(Z, SR.ELL, SR.JITTER)
    m = rng.standard_normal((1, M))
    Sq = 0.3 * np.eye(M) + 0.05 * np.tril(rng.standard_normal((M, M)))
    omega = rng.standard_normal((L, 1))
    x = np.concatenate([X[:200], np.array([[-1.0], [17.0]])])
    mean = np.sqrt(SR.K_VAR) * m @ R.A_of(W, Z, x, SR.ELL)
    for q in (Sq, np.abs(np.diag(Sq))):
        coef = PR.coefficients(m, q, W, Z, SR.ELL, omega, np.zeros((S, 2 * L)), np.zeros((S, M)))
        assert coef.shape == (S, 2 * L + M) and not np.any(coef[:, :2 * L])
        f = PR.evaluate(x, omega, Z, SR.ELL, coef, np.sqrt(SR.K_VAR))
        err = np.abs(f - mean).max()
        print("mean of the restatement against m A: %.3e of max|mean| %.3f" % (err / np.abs(mean).max(), np.abs(mean).max()))
        assert f.shape == (S, x.shape[0]) and err <= 1e-8 * np.abs(mean).max()


def test_coefficients_reproduce_u_at_the_inducing_points():
    """coef = [w / sqrt(L) | (u - g(z) W^T) W] with g written out from the basis, and the draw at the inducing points is
    g(z) + t A(z) = g(z) + t W (Lm Lm^T - jitter I): whitened back, (f(z) - g(z)) W^T = t (I - jitter W W^T)."""
    rng = np.random.default_rng(1)
    _, omega, z, ell, W, Sq = PR.cov_case(2, 64, 3)
    M, S, L, jitter = 32, 4, 64, 1e-5
    m, w, eps = rng.standard_normal((1, M)), rng.standard_normal((S, 2 * L)), rng.standard_normal((S, M))
    coef = PR.coefficients(m, Sq, W, z, ell, omega, w, eps)
    assert np.array_equal(coef[:, :2 * L], w / np.sqrt(L))
    g = (w / np.sqrt(L)) @ PR.basis(z, omega, None, ell)
    t = (m + eps @ Sq.T) - g @ W.T
    assert np.abs(coef[:, 2 * L:] - t @ W).max() <= 1e-12 * np.abs(coef[:, 2 * L:]).max()
    fz = PR.evaluate(z, omega, z, ell, coef)
    back = (fz - g) @ W.T
    want = t - jitter * (t @ W) @ W.T
    assert np.abs(back - want).max() <= 1e-8 * np.abs(want).max()


@pytest.mark.parametrize("L", [256, 1024, 4096])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_the_covariance_of_the_restatement_tends_to_the_exact_conditional(d, L):
    """max |covariance - (K - A^T A + A^T S S^T A)| <= 8 / sqrt(L) over seeds 0..9: M = 32, ell = 0.8, jitter 1e-5, z and
    300 points x uniform on [0, 16] (d = 1) or [0, 4]^d.  Observed worst over the seeds, times sqrt(L): d = 1: 2.4, 3.1,
    5.1 for L = 256, 1024, 4096; d = 2: 2.8, 4.0, 2.2; d = 3: 3.5, 2.8, 2.9."""
    worst = 0.0
    for seed in range(10):
        x, omega, z, ell, W, Sq = PR.cov_case(d, L, seed)
        cov = PR.covariance(x, omega, z, ell, W, Sq)
        assert np.abs(cov - cov.T).max() <= 1e-12
        worst = max(worst, float(np.abs(cov - PR.exact_covariance(x, z, ell, W, Sq)).max()))
    print("d=%d L=%d: worst error %.3e = %.2f / sqrt(L)" % (d, L, worst, worst * np.sqrt(L)))
    assert worst <= 8.0 / np.sqrt(L)
