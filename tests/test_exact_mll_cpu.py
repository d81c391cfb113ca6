"""The exact GP's log marginal likelihood on the host: the new C entries exist, are bound and validate their arguments
before any launch, and the numpy restatement the GPU tests lean on (tests/exact_mll_ref.py) is pinned against dense linear
algebra.  No HIP kernel runs here.

The case of the pins is the 2-D set of exact_gp_ref.plane_case with ell = (0.5, 0.7), k_var = 1.3, noise_var = 0.05.  With
the orthogonal probes Z = sqrt(N) chol(P_)^T (T = N) the probes' second moment is P_ exactly, so the estimator equals the
exact value and gradient up to the solve's tolerance.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import exact_gp_ref as E
import exact_mll_ref as R

NEW = ("hb_gram_bilinear_grad_f32", "hb_gram_bilinear_grad_f64", "hb_gram_bilinear_grad_ws_elems", "hb_pcg_update_coef_f32",
       "hb_pcg_update_coef_f64", "hb_pcg_direction_coef_f32", "hb_pcg_direction_coef_f64")
ELL, K_VAR, NOISE = np.array([0.5, 0.7]), 1.3, 0.05


# ---------------------------------------------------------------- C ABI
def test_exact_mll_symbols_are_exported_and_bound():
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
    assert callable(H.gram_bilinear_grad) and callable(hb.gp.log_marginal_likelihood)
    assert callable(hb.gp.GP.log_marginal_likelihood) and callable(hb.gp.GP.log_marginal_likelihood_and_grad)
    assert all(callable(getattr(ExactGPR, k)) for k in ("fit_hyper", "log_marginal_likelihood", "log_marginal_likelihood_and_grad"))


def test_workspace_size_does_not_grow_with_the_chunks():
    """min(chunks, 16) x strips of 128 x (1 + dl) doubles: linear in N, whatever S."""
    from henbun_amd import _lib

    ws = _lib.lib().raw("hb_gram_bilinear_grad_ws_elems")
    assert ws(0, 1) == 0 and ws(1, 1) == 2 and ws(128, 3) == 4 and ws(129, 3) == 8
    assert ws(2048, 2) == 16 * 3 and ws(2049, 2) == 2 * 17 * 3
    assert ws(16 * 2048, 1) == 16 * 256 * 2 and ws(16 * 2048 + 1, 1) == 16 * 257 * 2
    assert ws(100000, 2) == 16 * 782 * 3


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
@pytest.mark.parametrize("bad, word", [
    (dict(kind=1), "UnitRBF"),
    (dict(S=0), "extents"),
    (dict(d=0), "extents"),
    (dict(N=-1), "extents"),
    (dict(dl=2, d=3), "lengthscales"),
    (dict(A=None), "NULL"),
    (dict(B=None), "NULL"),
    (dict(w=None), "NULL"),
    (dict(g=None), "NULL"),
    (dict(ell=None), "NULL"),
    (dict(ws=None), "workspace"),
])
def test_gram_bilinear_grad_rejects_bad_arguments(suffix, bad, word):
    """(the pointers are the integer 1: any launch would fault -- every case must return before one)"""
    from henbun_amd import _lib

    lib = _lib.lib()
    a = dict(kind=0, x=1, ell=1, dl=1, A=1, B=1, w=1, g=1, N=100, d=1, S=2, ws=1)
    a.update(bad)
    rc = lib.raw("hb_gram_bilinear_grad" + suffix)(a["kind"], a["x"], a["ell"], a["dl"], a["A"], a["B"], a["w"], a["g"], a["N"],
                                                   a["d"], a["S"], a["ws"], None)
    assert rc < 0 and word in lib.last_error() and "hb_gram_bilinear_grad" in lib.last_error(), (rc, lib.last_error())


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
def test_pcg_coef_steps_reject_bad_arguments(suffix):
    from henbun_amd import _lib

    lib = _lib.lib()
    assert lib.raw("hb_pcg_update_coef" + suffix)(1, 1, 1, None, 1, 1, 1, 2, 10, 1, 0, None) < 0 and "hb_pcg_update" in lib.last_error()
    assert lib.raw("hb_pcg_update_coef" + suffix)(1, 1, 1, 1, 1, 1, 1, 2, 0, 1, 0, None) < 0 and "extents" in lib.last_error()
    assert lib.raw("hb_pcg_update_coef" + suffix)(1, 1, 1, 1, 1, 1, 1, 2, 10, 1, -1, None) < 0 and "iteration" in lib.last_error()
    assert lib.raw("hb_pcg_direction_coef" + suffix)(1, None, None, 1, 1, 1, 1.0, 1.0, 1, 2, 10, 1, 0, None) < 0
    assert "hb_pcg_direction" in lib.last_error()
    assert lib.raw("hb_pcg_direction_coef" + suffix)(1, None, 1, 1, 1, 1, 1.0, 1.0, 1, 2, 10, 1, -1, None) < 0
    assert "iteration" in lib.last_error()


def test_exact_gpr_hyper_variables_are_the_three_named():
    from henbun_amd.models import ExactGPR

    X, Y, _, _, _ = E.plane_case(20)
    m = ExactGPR(X=X, Y=Y, dtype="float64")
    hv = m._hyper_variables()
    assert list(hv) == ["lengthscales", "k_var", "var"]
    g = object.__getattribute__
    assert hv["k_var"] is g(m, "k_var") and hv["var"] is g(m, "var")
    assert hv["lengthscales"] is g(g(g(m, "gp"), "kern"), "lengthscales")


def test_host_quadrature_is_the_restatement():
    """exact.lanczos_logquad (the host tail of the library) against the restatement's tridiagonal on one recurrence."""
    from henbun_amd.gp import exact

    X, Y, _, _, _ = E.plane_case(48)
    _, rec = R.pcg_record(X, ELL, K_VAR, NOISE, Y.T, None, tol=1e-10)
    m = int(rec["lanczos_steps"][0])
    a, b = rec["coef"][:m, 0, 0], rec["coef"][:m, 1, 0]
    T = R.tridiagonal(a, b)
    assert m >= 10 and np.array_equal(T, T.T) and np.count_nonzero(np.triu(T, 2)) == 0
    assert abs(exact.lanczos_logquad(a, b) - R.logquad(a, b)) <= 1e-12 * abs(R.logquad(a, b))
    assert exact.lanczos_logquad(a[:0], b[:0]) == 0.0 and abs(exact.lanczos_logquad(a[:1], b[:0]) + np.log(a[0])) <= 1e-15
    coef = np.array([[[0.5, 0.5], [0.1, np.nan]], [[0.25, np.nan], [np.nan, np.nan]]])
    assert exact._lanczos_steps(coef).tolist() == [2, 1] and exact._lanczos_steps(coef[:0]).tolist() == [0, 0]


@pytest.mark.parametrize("stop_at, iterations", [(None, 3), (None, 4), (None, 10), (3, 10), (4, 10), (4, 4), (0, 6), (7, 8), (8, 13)])
def test_coefficient_log_has_one_row_per_iteration_whatever_was_allocated(stop_at, iterations):
    """exact._CoefLog with blocks of 4 iterations driven as pcg_solve drives it (numpy blocks in place of device tensors):
    iteration i writes alpha to row 2 i and beta to row 2 i + 1 of its slot until the log is closed at `stop_at` (the first
    restart: before a block boundary, on it, after it, at once, never).  Blocks are allocated only while the log is open,
    yet the assembled log is [iterations, 2, S] -- the recorded rows, then NaN -- and the steps count the recorded ones."""
    from henbun_amd.gp import exact

    S = 3
    log = exact._CoefLog(S, lambda: np.full((8, S), np.nan), block=4)
    for i in range(iterations):
        if stop_at is not None and i == stop_at:
            log.stop()
        for half in (0, 1):                                  # the update, then the direction of iteration i
            blk, at = log.slot(i)
            if blk is not None:
                blk[2 * at + half] = 1.0 + i + 0.5 * half
    recorded = iterations if stop_at is None else min(stop_at, iterations)
    assert len(log.blocks) == (recorded + 3) // 4
    coef = log.assemble(iterations, np.concatenate(log.blocks) if log.blocks else None)
    assert coef.shape == (iterations, 2, S)
    assert np.array_equal(coef[:recorded, 0, :], np.repeat(1.0 + np.arange(recorded)[:, None], S, 1))
    assert np.array_equal(coef[:recorded, 1, :], coef[:recorded, 0, :] + 0.5) and np.isnan(coef[recorded:]).all()
    assert exact._lanczos_steps(coef).tolist() == [recorded] * S
    wide = np.full((max(iterations, 5), 2, 2 * S), np.nan)   # the merge of log_marginal_likelihood: by the log's own length
    wide[:coef.shape[0], :, S:] = coef
    assert np.isnan(wide[:, :, :S]).all() and np.array_equal(wide[:recorded, 0, S:], coef[:recorded, 0, :])


# ---------------------------------------------------------------- the restatement
def test_bilinear_grad_is_the_dense_contraction():
    rng = np.random.default_rng(1)
    x = rng.uniform(0, 3, (41, 3))
    A, B, w = rng.standard_normal((5, 41)), rng.standard_normal((5, 41)), rng.standard_normal(5)
    for ell in (np.array([0.7, 0.9, 1.1]), np.array([0.8])):
        K = E.rbf(x, x, ell)
        W = np.einsum("s,si,sj->ij", w, A, B)
        D = [(x[:, k, None] - x[None, :, k]) ** 2 for k in range(3)]
        want = [np.sum(W * K)] + ([np.sum(W * K * D[k]) / ell[k] ** 3 for k in range(3)] if ell.size == 3
                                  else [np.sum(W * K * sum(D)) / ell[0] ** 3])
        for block in (7, 41, 512):
            g, M = R.bilinear_grad(x, ell, A, B, w, block=block, magnitude=True)
            assert g.shape == (1 + ell.size,) and np.all(np.abs(g - want) <= 1e-12 * M) and np.all(M >= np.abs(g))


def test_dense_gradient_against_central_differences():
    X, Y, _, _, _ = E.plane_case(60)
    Y = np.concatenate([Y, np.cos(X[:, :1])], axis=1)
    for ell in (ELL, np.array([0.6])):
        value, grad, mag = R.mll_dense(X, Y, ell, K_VAR, NOISE)
        h = 1e-5
        f = lambda e, k, s: R.mll_dense(X, Y, e, k, s)[0]
        fd = dict(k_var=(f(ell, K_VAR + h, NOISE) - f(ell, K_VAR - h, NOISE)) / (2 * h),
                  noise_var=(f(ell, K_VAR, NOISE + h) - f(ell, K_VAR, NOISE - h)) / (2 * h),
                  lengthscales=np.array([(f(ell + h * np.eye(ell.size)[k], K_VAR, NOISE)
                                          - f(ell - h * np.eye(ell.size)[k], K_VAR, NOISE)) / (2 * h) for k in range(ell.size)]))
        for name in fd:
            err = np.abs(grad[name] - fd[name]).max() / np.max(mag[name])
            print("mll_dense d/d%s (dl = %d): %.3e of the terms' magnitude" % (name, ell.size, err))
            assert err <= 1e-6
        assert mag["value"] >= abs(value)


@pytest.mark.parametrize("rank", [0, 16])
def test_orthogonal_probes_make_the_estimator_exact(rank):
    """N = 48, tol 1e-10: value within 1e-10 relative, every gradient component within 1e-9 relative of mll_dense (seen:
    at most 1e-14 and 7e-12)."""
    X, Y, _, _, _ = E.plane_case(48)
    C = E.factor(X, ELL, rank) if rank else None
    Z = R.orthogonal_probes(R.precond_dense(X, C, K_VAR, NOISE))
    assert np.abs(Z.T @ Z / 48 - R.precond_dense(X, C, K_VAR, NOISE)).max() <= 1e-12
    value, grad, info = R.mll_estimate(X, Y, ELL, K_VAR, NOISE, Z, C, tol=1e-10)
    ref, gref, _ = R.mll_dense(X, Y, ELL, K_VAR, NOISE)
    ev = abs(value - ref) / abs(ref)
    eg = max(np.abs(np.asarray(grad[k]) - gref[k]).max() / np.abs(gref[k]).min() for k in gref)
    print("rank %d: %d iterations, value %.3e relative, gradient %.3e relative, logdet %.6f (precond %.6f)"
          % (rank, info["iterations"], ev, eg, info["logdet"], info["logdet_precond"]))
    assert ev <= 1e-10 and eg <= 1e-9


@pytest.mark.parametrize("rank", [0, 16])
def test_tridiagonal_quadrature_is_the_dense_log_quadratic_form(rank):
    """16 Gaussian probes with covariance P_: the quadrature built from the PCG coefficients equals the dense same-probe
    1/T sum q^T log(P_^-1/2 K^ P_^-1/2) q to 1e-9 (seen 2e-11).  Its distance from the true logdet is the estimator's
    variance, which is printed, not asserted."""
    X, Y, _, _, _ = E.plane_case(48)
    N = 48
    C = E.factor(X, ELL, rank) if rank else None
    rng = np.random.default_rng(4)
    Z = rng.standard_normal((16, N)) @ np.linalg.cholesky(R.precond_dense(X, C, K_VAR, NOISE)).T
    _, _, info = R.mll_estimate(X, Y, ELL, K_VAR, NOISE, Z, C, tol=1e-10)
    got = info["logdet"] - info["logdet_precond"]
    want = R.logquad_dense(X, ELL, K_VAR, NOISE, Z, C)
    true = np.linalg.slogdet(E.dense(X, ELL, K_VAR, NOISE))[1]
    print("rank %d: quadrature %.9f, dense same-probe form %.9f (difference %.3e); logdet estimate %.4f, true %.4f"
          % (rank, got, want, abs(got - want), info["logdet"], true))
    assert abs(got - want) <= 1e-9 * max(1.0, abs(want))
    assert abs(info["logdet_precond"] - np.linalg.slogdet(R.precond_dense(X, C, K_VAR, NOISE))[1]) <= 1e-10 * N
