"""Gradient of the collapsed bound on the host: the numpy restatement the GPU tests lean on
(tests/collapsed_grad_ref.py) against torch.autograd in float64 and against central differences of
optimal_q_ref.collapsed_bound; Transform.dforward against differences of forward; the new C entries exist, are bound and
validate their arguments before any launch.  No HIP kernel runs here.

Bounds.  Restatement against autograd: both are float64 evaluations of the same function.  The z and lengthscale
gradients are differences of two terms (through K(z, X) and through K(z, z)) whose weights carry W = Lm^-1 twice; the
rounding error of W is of relative order eps cond(Kmm) <= eps M / jitter (lambda_max <= tr Kmm = M (1 + jitter)) and
enters each term at the term's own size, so the error scales with the cancelling scale max|streamed part| + max|Kmm
part|, not with the result.  Bound: 8 eps (M / jitter) x that scale -- two evaluations, and the factor 4 the GPU tests
use for the order of summation; 8.5e-9 of the scale at M = 48, jitter 1e-5.  Observed: <= 1.2e-9 of the scale
('neglected', d = 1), 1e-14 .. 1e-11 elsewhere.  The scalars do not cancel: 1e-9 relative (observed <= 2.2e-12).
Central differences: the bound is 4 x (the truncation error estimated from two step sizes, |fd(2h) - fd(h)| / 3, plus the
rounding error 1e-12 |F| / h of two evaluations of F), every figure printed."""
import numpy as np
import pytest

import collapsed_grad_ref as C
import optimal_q_ref as R

JITTER = 1e-5
CASES = [(residual, P, d, scalar) for residual in ("diagonal", "neglected") for P in (1, 2)
         for d, scalar in ((1, True), (3, False), (3, True))]


@pytest.mark.parametrize("residual, P, d, scalar", CASES)
def test_restatement_against_autograd(residual, P, d, scalar):
    X, Y, z, ell = C.case(3000, 48, d, P, seed=P + d, scalar_ell=scalar)
    r = C.bound_and_grad(X, Y, z, ell, JITTER, 0.09, 1.3, residual)
    a = C.bound_autograd(X, Y, z, ell, JITTER, 0.09, 1.3, residual)
    assert r["z"].shape == z.shape and r["lengthscales"].shape == ell.shape
    zs = np.abs(r["z_streamed"]).max() + np.abs(r["z_kmm"]).max()
    es = np.abs(r["ell_streamed"]).max() + np.abs(r["ell_kmm"]).max()
    ez, ee = np.abs(r["z"] - a["z"]).max(), np.abs(r["lengthscales"] - a["lengthscales"]).max()
    print("%s P=%d d=%d dl=%d: value %.3e; z: max|grad| %.3e scale %.3e gap %.3e (%.1e of scale); ell: %.3e scale %.3e gap "
          "%.3e (%.1e); noise_var %.1e k_var %.1e (relative)"
          % (residual, P, d, ell.size, abs(r["value"] / a["value"] - 1), np.abs(a["z"]).max(), zs, ez, ez / zs,
             np.abs(a["lengthscales"]).max(), es, ee, ee / es, abs(r["noise_var"] / a["noise_var"] - 1),
             abs(r["k_var"] / a["k_var"] - 1)))
    assert abs(r["value"] - a["value"]) <= 1e-12 * abs(a["value"])
    cancel = 8.0 * np.finfo(np.float64).eps * z.shape[0] / JITTER
    assert ez <= cancel * zs
    assert ee <= cancel * es
    assert abs(r["noise_var"] - a["noise_var"]) <= 1e-9 * abs(a["noise_var"])
    assert abs(r["k_var"] - a["k_var"]) <= 1e-9 * abs(a["k_var"])


def test_the_z_gradient_is_a_small_difference_of_two_large_parts():
    """The reason the device routine is float64 end to end: at N = 20000, M = 64, jitter 1e-5 the streamed and the Kmm
    parts of the z gradient are more than 100 times the gradient itself."""
    X, Y, z, ell = C.case(20000, 64, 1, 1, seed=0)
    r = C.bound_and_grad(X, Y, z, ell, JITTER, 0.09, 1.0)
    g, s, k = np.abs(r["z"]).max(), np.abs(r["z_streamed"]).max(), np.abs(r["z_kmm"]).max()
    print("max|z gradient| %.3g, max|streamed part| %.3g, max|Kmm part| %.3g" % (g, s, k))
    assert s > 100 * g and k > 100 * g


@pytest.mark.parametrize("residual, P, d, scalar", CASES)
def test_restatement_against_central_differences(residual, P, d, scalar):
    X, Y, z, ell = C.case(2000, 32, d, P, seed=10 + P + d, scalar_ell=scalar)
    s2, k = 0.09, 1.3
    r = C.bound_and_grad(X, Y, z, ell, JITTER, s2, k, residual)
    rng = np.random.RandomState(1)

    def F(z_=z, ell_=ell, s2_=s2, k_=k):
        st = R.stats(X, Y, z_, ell_, JITTER)
        return R.collapsed_bound(*st, X.shape[0], float(s2_), float(k_), residual)

    groups = [("z", z, r["z"], lambda v: F(z_=v)), ("lengthscales", ell, r["lengthscales"], lambda v: F(ell_=v)),
              ("noise_var", np.array(s2), np.array(r["noise_var"]), lambda v: F(s2_=v)),
              ("k_var", np.array(k), np.array(r["k_var"]), lambda v: F(k_=v))]
    for name, x0, g, f in groups:
        u = np.asarray(rng.standard_normal(np.shape(x0)))
        u = u / np.sqrt((u * u).sum())
        h = 1e-4 * max(1e-2, float(np.abs(x0).max()) if name != "z" else 1.0)
        fd1, fd2 = C.directional_fd(f, x0, u, h), C.directional_fd(f, x0, u, 2 * h)
        an = float((g * u).sum())
        tol = 4.0 * (abs(fd2 - fd1) / 3.0 + 1e-12 * abs(r["value"]) / h)
        print("%s P=%d d=%d dl=%d %s: analytic %.9e central difference %.9e (h=%.1e) |gap| %.3e bound %.3e"
              % (residual, P, d, ell.size, name, an, fd1, h, abs(an - fd1), tol))
        assert abs(an - fd1) <= tol


# ---------------------------------------------------------------- transforms
def test_dforward_against_differences_of_forward():
    from henbun_amd import transforms as T

    x = np.array([-30.0, -5.0, -0.7, 0.0, 0.3, 4.0, 25.0])
    h = 1e-6
    for t in (T.Identity(), T.Exp(), T.Log1pe(), T.Logistic(-1.0, 3.0), T.positive):
        d = t.dforward(x)
        fd = (t.forward(x + h) - t.forward(x - h)) / (2 * h)
        assert d.shape == x.shape and d.dtype == np.float64
        # central difference: h^2 / 6 |f'''| <= 2e-13 |f'| for these maps, plus rounding 1e-16 |f| / h
        assert np.all(np.abs(d - fd) <= 1e-8 * np.abs(fd) + 1e-9), (type(t).__name__, d, fd)
    assert T.Log1pe().dforward(np.array([0.0]))[0] == 0.5          # softplus' = sigmoid


# ---------------------------------------------------------------- C ABI
def test_kgrad_symbols_are_declared_exported_and_bound():
    import os

    from henbun_amd import _lib

    names = _lib.declared_symbols()
    lib = _lib.lib()
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "henbun_hip.h")).read()
    for n in ("hb_sgp_kgrad_f32", "hb_sgp_kgrad_f64", "hb_sgp_kgrad_ws_elems"):
        assert n in names and n + "(" in header
        assert lib.raw(n) is not None
    assert lib.raw("hb_version")() == 2


def _call(lib, suffix, **kw):
    a = dict(kind=0, X=1, Y=1, z=1, ell=1, dl=1, Q=1, R=1, zbar=1, ellbar=1, N=100, M=64, d=1, P=1, ws=None)
    a.update(kw)
    return lib.raw("hb_sgp_kgrad" + suffix)(a["kind"], a["X"], a["Y"], a["z"], a["ell"], a["dl"], a["Q"], a["R"], a["zbar"],
                                            a["ellbar"], a["N"], a["M"], a["d"], a["P"], a["ws"], None)


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
@pytest.mark.parametrize("bad, word", [
    (dict(kind=1), "UnitRBF"),
    (dict(N=0), "extents"),
    (dict(M=0), "extents"),
    (dict(d=0), "extents"),
    (dict(P=-1), "extents"),
    (dict(dl=2, d=3), "lengthscales"),
    (dict(X=None), "NULL input"),
    (dict(Y=None), "NULL input"),
    (dict(Q=None), "NULL input"),
    (dict(R=None), "NULL input"),
    (dict(zbar=None), "NULL output"),
    (dict(ellbar=None), "NULL output"),
    (dict(M=9000), "too large"),
    (dict(ws=None), "workspace"),
])
def test_kgrad_entry_points_reject_bad_arguments(suffix, bad, word):
    """(the pointers are the integer 1: any launch would fault -- every case must return before one)"""
    from henbun_amd import _lib

    lib = _lib.lib()
    rc = _call(lib, suffix, **bad)
    assert rc < 0 and word in lib.last_error(), (rc, lib.last_error())


def test_kgrad_workspace_does_not_depend_on_N():
    from henbun_amd import _lib

    f = _lib.lib().raw("hb_sgp_kgrad_ws_elems")
    for M, d, P in [(512, 1, 1), (512, 3, 2), (96, 3, 1), (50, 1, 2), (1024, 1, 1)]:
        w = [f(N, M, d, P) for N in (1, 100000, 10000000)]
        assert w[0] == w[1] == w[2] >= M * M
        assert w[0] <= M * M + 64 + 256 * (2 * M * d + 64)
    assert f(100, 0, 1, 1) == 0
