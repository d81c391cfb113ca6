"""Hyper-parameter gradient of the ELBO at a fixed q(u) on the host: the numpy restatement the GPU tests lean on
(tests/elbo_grad_ref.py) against torch.autograd in float64 and against directional central differences, for the
Gaussian, Poisson and Bernoulli likelihoods; the envelope property against collapsed_grad_ref at q* = optimal_q; the new
C entries exist, are bound and validate their arguments before any launch.  No HIP kernel runs here.

The restatement tests (against autograd, the surrogate, central differences and the collapsed bound) pin the REFERENCE
tests/elbo_grad_ref.py, not the library: they would pass without the feature.  The tests of the C entries at the end and
everything in tests/test_elbo_grad_gpu.py need the feature.

Bounds.  Restatement against autograd: two float64 evaluations of the same function; as in test_collapsed_grad_cpu.py
the z and lengthscale gradients are differences of a streamed and a K(z, z) part whose weights carry W = Lm^-1 twice, so
the error scales with the cancelling scale max|streamed| + max|K(z, z) part| at relative size eps cond(Kmm) <= eps M /
jitter: bound 8 eps (M / jitter) x that scale (8.5e-9 of it at M = 48, jitter 1e-5).  k_var: 1e-9 of the sum of its two
absolute terms.
Bernoulli: the restatement (and the device) DEFINE dl/dv = -lam / 2 (Stein's identity) with lam the 20-node quadrature
of -d2 log p, whereas autograd differentiates the 20-node quadrature of log p.  The two differ by the quadrature error,
not by rounding.  The arithmetic is therefore pinned with the per-point derivatives of the quadrature value in place of
(lam, gamma) -- the restatement is linear in them -- under the bounds above, and the Stein-versus-quadrature gap of the
full gradient is printed (observed: in the docstring of the test) and held under a loose ceiling, 1e-7 of the largest
entry of each gradient: the GPU bounds are 4 x this gap, and a wrong lam in sites_ref.py would otherwise widen them
silently (a 20-node rule integrates these sigmoid integrands at v <= 1.2 to far better than that; observed <= 6e-11
relative)."""
import numpy as np
import pytest

import collapsed_grad_ref as C
import elbo_grad_ref as E
import optimal_q_ref as R
import sites_ref as S_

JITTER = 1e-5
PARAM = {E.GAUSSIAN: 0.09, E.POISSON: 1.0, E.BERNOULLI: 1.0}
NAME = {E.GAUSSIAN: "gaussian", E.POISSON: "poisson", E.BERNOULLI: "bernoulli"}


def _labels(lik, X, seed):
    """y [N] for a latent sin(sum_d x): the generating rule of sites_ref.problem for any d."""
    f = 1.5 * np.sin(X.sum(1))
    rng = np.random.RandomState(77 + seed)
    if lik == E.BERNOULLI:
        return (rng.uniform(size=f.shape) < 1.0 / (1.0 + np.exp(-f))).astype(np.float64)
    if lik == E.POISSON:
        return rng.poisson(np.exp(f)).astype(np.float64)
    return f + 0.3 * rng.randn(*f.shape)


def _quadrature_weights(lik, y, mu, v, param):
    """(w, r) = (-2 dl/dv, dl/dmu) per point from torch.autograd on the VALUE l_j(mu_j, v_j) the sites use."""
    import torch

    t = lambda a: torch.tensor(np.asarray(a, np.float64).reshape(-1))
    y, mu, v = t(y), t(mu).requires_grad_(True), t(v).requires_grad_(True)
    x, wq = S_.gh(20)
    f = mu[:, None] + torch.sqrt(2.0 * v)[:, None] * torch.tensor(x)[None, :]
    l = ((y[:, None] * f - torch.nn.functional.softplus(f)) * torch.tensor(wq)).sum(1)
    l.sum().backward()
    return -2.0 * v.grad.numpy(), mu.grad.numpy()


def _scales(r):
    return (np.abs(r["z_streamed"]).max() + np.abs(r["z_kmm"]).max(),
            np.abs(r["ell_streamed"]).max() + np.abs(r["ell_kmm"]).max())


def _case(lik, d, scalar, N=3000, M=48, seed=0):
    X, _, z, ell = C.case(N, M, d, 1, seed=seed + d, scalar_ell=scalar)
    return X, _labels(lik, X, seed), z, ell, E.q_case(M, seed)


CASES = [(lik, residual, d, scalar) for lik in (E.GAUSSIAN, E.POISSON, E.BERNOULLI) for residual in ("diagonal", "neglected")
         for d, scalar in ((1, True), (3, False), (3, True))]


@pytest.mark.parametrize("lik, residual, d, scalar", CASES)
def test_restatement_against_autograd(lik, residual, d, scalar):
    """Observed: value <= 2.5e-14 relative; z gap <= 5.8e-14 of the cancelling scale, lengthscales <= 2.2e-12, k_var <= 2e-14
    of its absolute terms.  Bernoulli, Stein against the derivative of the 20-node quadrature (k_var 1.3, v up to 1.13):
    max|w - w_q| <= 4.1e-9 at max|w| 0.24; gap of the full gradient: z <= 2.1e-9 (max|z gradient| 41), lengthscales
    <= 4.9e-9 (gradient 47 .. 176), k_var <= 5.3e-9 (gradient 150)."""
    X, y, z, ell, (m, S) = _case(lik, d, scalar)
    k = 1.3
    r = E.elbo_and_grad(X, y, z, ell, JITTER, lik, m, S, PARAM[lik], k, residual)
    a = E.elbo_autograd(X, y, z, ell, JITTER, lik, m, S, PARAM[lik], k, residual)
    assert r["z"].shape == z.shape and r["lengthscales"].shape == ell.shape
    assert abs(r["value"] - a["value"]) <= 1e-12 * abs(a["value"])
    pinned = r
    if lik == E.BERNOULLI:
        A = R.A_of(r["W"], z, X, ell)
        mu, v = E.marginals(m, S, A, k, residual)
        wq, rq = _quadrature_weights(lik, y, mu, v, PARAM[lik])
        pinned = E.grad_from_weights(X, wq, rq, z, ell, JITTER, m, S, k, residual)
        print("bernoulli %s d=%d dl=%d: Stein against the derivative of the quadrature: max|w - w_q| %.3e (max|w| %.3e), "
              "max|r - r_q| %.3e; gradient gap z %.3e (max|grad| %.3e) ell %.3e (%.3e) k_var %.3e (%.3e); max v %.3f"
              % (residual, d, ell.size, np.abs(r["w"] - wq).max(), np.abs(wq).max(), np.abs(r["r"] - rq).max(),
                 np.abs(r["z"] - a["z"]).max(), np.abs(a["z"]).max(), np.abs(r["lengthscales"] - a["lengthscales"]).max(),
                 np.abs(a["lengthscales"]).max(), abs(r["k_var"] - a["k_var"]), abs(a["k_var"]), v.max()))
        assert np.abs(r["z"] - a["z"]).max() <= 1e-7 * np.abs(a["z"]).max()
        assert np.abs(r["lengthscales"] - a["lengthscales"]).max() <= 1e-7 * np.abs(a["lengthscales"]).max()
        assert abs(r["k_var"] - a["k_var"]) <= 1e-7 * abs(a["k_var"])
    zs, es = _scales(pinned)
    ez, ee = np.abs(pinned["z"] - a["z"]).max(), np.abs(pinned["lengthscales"] - a["lengthscales"]).max()
    ek = abs(pinned["k_var"] - a["k_var"])
    print("%s %s d=%d dl=%d: value %.3e; z: max|grad| %.3e scale %.3e gap %.3e (%.1e of scale); ell: %.3e scale %.3e gap "
          "%.3e (%.1e); k_var %.3e gap %.3e (%.1e of its terms)"
          % (NAME[lik], residual, d, ell.size, abs(r["value"] / a["value"] - 1), np.abs(a["z"]).max(), zs, ez, ez / zs,
             np.abs(a["lengthscales"]).max(), es, ee, ee / es, a["k_var"], ek, ek / pinned["k_var_abs"]))
    cancel = 8.0 * np.finfo(np.float64).eps * z.shape[0] / JITTER
    assert ez <= cancel * zs
    assert ee <= cancel * es
    assert ek <= 1e-9 * pinned["k_var_abs"]


@pytest.mark.parametrize("residual, d, scalar", [("diagonal", 1, True), ("diagonal", 3, False), ("neglected", 3, True)])
def test_restatement_with_weights_of_either_sign_against_autograd_of_the_surrogate(residual, d, scalar):
    """What the kernel tests feed hb_sgp_wkgrad: w with both signs and exact zeros.  For fixed w, r the restatement is the
    exact gradient of sum_j (r_j mu_j - w_j v_j / 2).
    Observed: z gap <= 3.8e-14 of the cancelling scale, lengthscales <= 5.7e-13, k_var <= 8.0e-13 of its terms."""
    X, _, z, ell, (m, S) = _case(E.GAUSSIAN, d, scalar, seed=5)
    w, rr = E.weights_case(X.shape[0], 5)
    assert (w == 0).sum() > 0 and (w < 0).sum() > 0 and (w > 0).sum() > 0
    r = E.grad_from_weights(X, w, rr, z, ell, JITTER, m, S, 1.3, residual)
    a = E.surrogate_autograd(X, w, rr, z, ell, JITTER, m, S, 1.3, residual)
    zs, es = _scales(r)
    ez, ee = np.abs(r["z"] - a["z"]).max(), np.abs(r["lengthscales"] - a["lengthscales"]).max()
    print("surrogate %s d=%d dl=%d: z gap %.3e scale %.3e (%.1e); ell gap %.3e scale %.3e (%.1e); k_var gap %.3e (%.1e)"
          % (residual, d, ell.size, ez, zs, ez / zs, ee, es, ee / es, abs(r["k_var"] - a["k_var"]),
             abs(r["k_var"] - a["k_var"]) / r["k_var_abs"]))
    cancel = 8.0 * np.finfo(np.float64).eps * z.shape[0] / JITTER
    assert ez <= cancel * zs and ee <= cancel * es
    assert abs(r["k_var"] - a["k_var"]) <= 1e-9 * r["k_var_abs"]


@pytest.mark.parametrize("lik", [E.GAUSSIAN, E.POISSON, E.BERNOULLI])
@pytest.mark.parametrize("residual, d, scalar", [("diagonal", 1, True), ("neglected", 3, False), ("diagonal", 3, True)])
def test_restatement_against_central_differences(lik, residual, d, scalar):
    """Directional central differences of the restatement's own VALUE at the fixed q.  Bound as in
    test_collapsed_grad_cpu.py: 4 x (|fd(2h) - fd(h)| / 3 + 1e-12 |F| / h).  Bernoulli: the analytic side uses the
    derivatives of the quadrature value (see the module docstring); the Stein form's directional gap is printed."""
    X, y, z, ell, (m, S) = _case(lik, d, scalar, N=2000, M=32, seed=10)
    k = 1.3
    r = E.elbo_and_grad(X, y, z, ell, JITTER, lik, m, S, PARAM[lik], k, residual)
    pinned = r
    if lik == E.BERNOULLI:
        mu, v = E.marginals(m, S, R.A_of(r["W"], z, X, ell), k, residual)
        pinned = E.grad_from_weights(X, *_quadrature_weights(lik, y, mu, v, PARAM[lik]), z, ell, JITTER, m, S, k, residual)
    rng = np.random.RandomState(1)

    def F(z_=z, ell_=ell, k_=k):
        _, W = R.chol_factor(z_, ell_, JITTER)
        mu, v = E.marginals(m, S, R.A_of(W, z_, X, ell_), float(k_), residual)
        return float(S_.sites(lik, y, mu, v, PARAM[lik])[0].sum()) - E.kl(m, S)

    assert abs(F() - r["value"]) <= 1e-13 * abs(r["value"])
    for name, x0, f in [("z", z, lambda v: F(z_=v)), ("lengthscales", ell, lambda v: F(ell_=v)),
                        ("k_var", np.array(k), lambda v: F(k_=v))]:
        u = np.asarray(rng.standard_normal(np.shape(x0)))
        u = u / np.sqrt((u * u).sum())
        h = 1e-4 * max(1e-2, float(np.abs(x0).max()) if name != "z" else 1.0)
        fd1, fd2 = C.directional_fd(f, x0, u, h), C.directional_fd(f, x0, u, 2 * h)
        an, stein = float((np.asarray(pinned[name]) * u).sum()), float((np.asarray(r[name]) * u).sum())
        tol = 4.0 * (abs(fd2 - fd1) / 3.0 + 1e-12 * abs(r["value"]) / h)
        print("%s %s d=%d dl=%d %s: analytic %.9e central difference %.9e (h=%.1e) |gap| %.3e bound %.3e; Stein form %.9e"
              % (NAME[lik], residual, d, ell.size, name, an, fd1, h, abs(an - fd1), tol, stein))
        assert abs(an - fd1) <= tol


@pytest.mark.parametrize("residual", ["diagonal", "neglected"])
def test_envelope_gaussian_at_the_optimal_q_reproduces_the_gradient_of_the_collapsed_bound(residual):
    """At q* = optimal_q the partial gradient at fixed q is the total derivative of the collapsed bound: value and the
    z / lengthscale / k_var gradients against collapsed_grad_ref.bound_and_grad.  Both are float64 evaluations whose
    parts cancel, and q* itself carries the rounding of Lambda^-1 (relative eps cond(Lambda)), so the bound is the one of
    the autograd comparison on the SUM of the two restatements' cancelling scales.  The gap printed here is what the GPU
    test's envelope bound is built from.
    Observed: value <= 3.3e-15 relative; z gap 1.0e-12 of the summed scale ('diagonal'; 1.9e-9 at max|z gradient| 0.23)
    and 5.6e-10 ('neglected'; 4.3e-8 at 0.058); lengthscales <= 4.3e-11; k_var <= 2.6e-15 of its terms."""
    N, M, s2, k = 4096, 32, 0.09, 1.3
    X, Y, z, ell = C.case(N, M, 1, 1, seed=3)
    c = C.bound_and_grad(X, Y, z, ell, JITTER, s2, k, residual)
    m, S, _, _ = R.optimal_q(c["Phi"], c["b"], s2, k)
    r = E.elbo_and_grad(X, Y, z, ell, JITTER, E.GAUSSIAN, m, S, s2, k, residual)
    zs, es = (a + b for a, b in zip(_scales(r), _scales(c)))
    ez, ee = np.abs(r["z"] - c["z"]).max(), np.abs(r["lengthscales"] - c["lengthscales"]).max()
    ek, ks = abs(r["k_var"] - c["k_var"]), r["k_var_abs"] + c["k_var_abs"]
    print("envelope %s: value %.9f collapsed %.9f (rel %.2e); z gap %.3e (max|grad| %.3e, scales %.3e: %.1e); ell gap %.3e "
          "(%.3e, %.3e: %.1e); k_var %.9e against %.9e gap %.3e (%.1e of the terms)"
          % (residual, r["value"], c["value"], abs(r["value"] / c["value"] - 1), ez, np.abs(c["z"]).max(), zs, ez / zs, ee,
             np.abs(c["lengthscales"]).max(), es, ee / es, r["k_var"], c["k_var"], ek, ek / ks))
    assert abs(r["value"] - c["value"]) <= 1e-10 * abs(c["value"])
    cancel = 8.0 * np.finfo(np.float64).eps * M / JITTER
    assert ez <= cancel * zs and ee <= cancel * es
    assert ek <= 1e-9 * ks


# ---------------------------------------------------------------- C ABI
def test_wkgrad_symbols_are_declared_exported_and_bound():
    import os

    from henbun_amd import _lib

    names = _lib.declared_symbols()
    lib = _lib.lib()
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "henbun_hip.h")).read()
    for n in ("hb_sgp_wkgrad_f32", "hb_sgp_wkgrad_f64"):
        assert n in names and n + "(" in header
        assert lib.raw(n) is not None
    assert lib.raw("hb_version")() == 2


def _call(lib, suffix, **kw):
    a = dict(kind=0, X=1, w=1, r=1, z=1, ell=1, dl=1, Q=1, R=1, zbar=1, ellbar=1, N=100, M=64, d=1, ws=None)
    a.update(kw)
    return lib.raw("hb_sgp_wkgrad" + suffix)(a["kind"], a["X"], a["w"], a["r"], a["z"], a["ell"], a["dl"], a["Q"], a["R"],
                                             a["zbar"], a["ellbar"], a["N"], a["M"], a["d"], a["ws"], None)


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
@pytest.mark.parametrize("bad, word", [
    (dict(kind=1), "UnitRBF"),
    (dict(N=0), "extents"),
    (dict(M=0), "extents"),
    (dict(d=0), "extents"),
    (dict(dl=2, d=3), "lengthscales"),
    (dict(X=None), "NULL input"),
    (dict(w=None), "NULL input"),
    (dict(r=None), "NULL input"),
    (dict(Q=None), "NULL input"),
    (dict(R=None), "NULL input"),
    (dict(zbar=None), "NULL output"),
    (dict(ellbar=None), "NULL output"),
    (dict(M=9000), "too large"),
    (dict(ws=None), "workspace"),
])
def test_wkgrad_entry_points_reject_bad_arguments(suffix, bad, word):
    """(the pointers are the integer 1: any launch would fault -- every case must return before one)"""
    from henbun_amd import _lib

    lib = _lib.lib()
    rc = _call(lib, suffix, **bad)
    assert rc < 0 and word in lib.last_error(), (rc, lib.last_error())
