"""Input gradient of the sparse-GP bounds on the GPU: hb_sgp_kgrad_x / hb_sgp_wkgrad_x, SparseGP.collapsed_bound_and_grad
(x_grad=True) and SparseGP.elbo_and_grad(x_grad=True) against the float64 host references of tests/kgrad_x_ref.py
(pinned on the host by tests/test_kgrad_x_cpu.py).

Bounds are not constants.  The rule is the project's: err <= 4 x max(gap, gamma x scale), gap = max|restatement -
torch.autograd| of the two independent float64 CPU evaluations ON THE SAME INPUTS, scale = the largest sum of absolute
terms of an entry of xbar (kgrad_x_ref.abs_scale) and gamma = (2 M + P + 16) 2^-53, the a-priori bound of summing 2 M + P
terms plus 16 ulp for the rounding of K and the products; the factor 4 covers the order of summation.  The ELBO route
uses the tolerance test_elbo_grad_gpu.py applies to its z gradient, 4 x max(gap, 1e-10 x scale), with the scale of xbar.
Every figure is printed before it is asserted.

Observed on MI355X: in the docstrings of the tests; profiles/sgp_kgrad_x.txt holds the timings."""
import functools

import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd import hip_ops as H
from henbun_amd.models import SVGPLik

import collapsed_grad_ref as C
import elbo_grad_ref as E
import kgrad_x_ref as KX
import sites_ref as SR

pytestmark = pytest.mark.gpu

JITTER = 1e-5
LIKS = {SR.BERNOULLI: hb.likelihoods.Bernoulli, SR.POISSON: hb.likelihoods.Poisson}


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


# ------------------------------------------------------------------------------------------------ 1. the kernel
@functools.lru_cache(maxsize=None)
def _kernel_case(dtype, d, P, N, M, scalar_ell=False):
    """Inputs (X, Y rounded to the storage type), the weights Q, R of the bound's tail, drawn column weights, and per
    form (restatement of xbar, gap to autograd, abs-scale) -- computed once and shared."""
    npdt = np.float64 if dtype == "float64" else np.float32
    X, Y, z, ell = C.case(N, M, d, P, seed=N + M + d + P, scalar_ell=scalar_ell)
    X, Y = X.astype(npdt).astype(np.float64), Y.astype(npdt).astype(np.float64)
    r = C.bound_and_grad(X, Y, z, ell, JITTER, 0.09, 1.0)
    Q, Rw = r["Q"], r["R"]
    xb = KX.streamed_x(X, Y, z, ell, Q, Rw)
    plain = (xb, np.abs(xb - KX.bound_autograd_x(X, Y, z, ell, JITTER, 0.09, 1.0)).max(),
             KX.abs_scale(X, Y, z, ell, Q, Rw).max())
    w, rr = E.weights_case(N, N + M + d)
    R1 = np.ascontiguousarray(Rw[:, :1])
    xw = KX.streamed_x_w(X, w, rr, z, ell, Q, R1)
    weighted = (xw, np.abs(xw - KX.surrogate_autograd_x(X, w, rr, z, ell, Q, R1)).max(),
                KX.abs_scale(X, rr[:, None], z, ell, Q, R1, w=w).max())
    return X, Y, z, ell, Q, Rw, R1, w, rr, plain, weighted


def _check_kgrad_x(dtype, d, P, N, M, scalar_ell=False):
    dt = torch.float64 if dtype == "float64" else torch.float32
    X, Y, z, ell, Q, Rw, R1, w, rr, plain, weighted = _kernel_case(dtype, d, P, N, M, scalar_ell)
    assert ell.shape == ((1,) if scalar_ell or d == 1 else (d,))
    f64 = torch.float64
    common = [dev(v, f64) for v in (z, ell, Q)]
    runs = [("sgp_kgrad_x", H.sgp_kgrad, [dev(X, dt), dev(Y, dt)] + common + [dev(Rw, f64)], plain, P),
            ("sgp_wkgrad_x", H.sgp_wkgrad, [dev(X, dt), dev(w, f64), dev(rr, f64)] + common + [dev(R1, f64)], weighted, 1)]
    for name, fn, args, (ref, gap, scale), Pk in runs:
        zb, eb, xb = fn(*args, x_grad=True)
        zb2, eb2, xb2 = fn(*args, x_grad=True)
        z0, e0 = fn(*args)
        torch.cuda.synchronize()
        assert xb.dtype == torch.float64 and tuple(xb.shape) == (N, d)
        assert torch.equal(xb, xb2) and torch.equal(zb, zb2) and torch.equal(eb, eb2)      # two runs: the same bits
        assert torch.equal(zb, z0) and torch.equal(eb, e0)                                  # the bits of the entry without _x
        got = xb.cpu().numpy()
        err, bnd = np.abs(got - ref).max(), KX.bound(gap, scale, M, Pk)
        print("%s %s N=%d M=%d d=%d dl=%d P=%d: device %.3e, CPU gap %.3e, abs-scale %.3e (max|xbar| %.3e), bound %.3e "
              "(%.2g of it)" % (name, dtype, N, M, d, ell.size, Pk, err, gap, scale, np.abs(ref).max(), bnd, err / bnd))
        assert np.all(np.isfinite(got))
        assert err <= bnd


@pytest.mark.parametrize("M", [32, 96, 50])
@pytest.mark.parametrize("N", [1, 97, 4099])
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_sgp_kgrad_x_against_the_restatement(dtype, d, P, N, M):
    """hb_sgp_kgrad_x and hb_sgp_wkgrad_x (the latter with drawn column weights of both signs) against the restatement on
    the same Q, R; two runs bitwise equal; zbar and ellbar the bits of hb_sgp_kgrad / hb_sgp_wkgrad.  M = 32 leaves six
    of the eight waves without a row tile, M = 96 gives two waves a second one, M = 50 takes the plain form; N = 1, 97,
    4099 leave ragged last steps and, at 4099, 129 steps for 129 workgroups.
    Observed on MI355X (72 shapes, both forms): device error <= 0.63 % of the bound (worst: weighted, float32, N = 1,
    M = 32, d = 3: 9.4e-16 against 1.5e-13) and <= 2.3e-16 of the abs-scale.  Worst per M (fraction of the bound,
    unweighted / weighted): 32: 4.5e-3 / 6.3e-3; 96: 1.2e-3 / 9.5e-4; 50 (plain form): 1.8e-3 / 2.7e-3."""
    _check_kgrad_x(dtype, d, P, N, M)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_sgp_kgrad_x_at_the_full_lds_budget(dtype):
    """M = 512, d = 3: 512 x 32 doubles of K plus the waves' column sums, four row tiles per wave.
    Observed on MI355X: unweighted 1.6e-10 against a bound of 6.9e-6 (abs-scale 1.5e7), weighted 3.4e-10 against 2.4e-5."""
    _check_kgrad_x(dtype, 3, 2, 4099, 512)


@pytest.mark.parametrize("M", [96, 50])
def test_sgp_kgrad_x_one_shared_lengthscale_in_three_dimensions(M):
    """d = 3 with ONE lengthscale (dl = 1 < d): every dimension of xbar is divided by the same ell^2."""
    _check_kgrad_x("float32", 3, 2, 97, M, True)


def test_a_column_of_xbar_does_not_depend_on_the_rest_of_the_call():
    """Strip form: rows 0 .. 96 of xbar of an N = 4099 call are the bits of the N = 97 call on the first 97 rows -- a
    column's sum runs over the rows in an order that depends on M alone, in the one workgroup that owns its step."""
    X, Y, z, ell, Q, Rw, R1, w, rr, _, _ = _kernel_case("float64", 3, 2, 4099, 96)
    f64 = torch.float64
    tail = [dev(v, f64) for v in (z, ell, Q, Rw)]
    _, _, big = H.sgp_kgrad(dev(X, f64), dev(Y, f64), *tail, x_grad=True)
    _, _, small = H.sgp_kgrad(dev(X[:97], f64), dev(Y[:97], f64), *tail, x_grad=True)
    assert torch.equal(big[:97], small)
    tail[3] = dev(R1, f64)
    _, _, big = H.sgp_wkgrad(dev(X, f64), dev(w, f64), dev(rr, f64), *tail, x_grad=True)
    _, _, small = H.sgp_wkgrad(dev(X[:97], f64), dev(w[:97], f64), dev(rr[:97], f64), *tail, x_grad=True)
    assert torch.equal(big[:97], small)


def test_sgp_kgrad_x_plain_form_agrees_with_the_strips():
    """The diagnostic switch sgp_kgrad_plain runs an aligned shape through the plain loops: the same xbar to the order
    of summation, 4 gamma x the abs-scale.
    Observed on MI355X: 7.5e-12 at abs-scale 6.8e5 (bound 6.3e-8); weighted 1.2e-11 at 1.7e6 (bound 1.6e-7)."""
    X, Y, z, ell, Q, Rw, R1, w, rr, plain, weighted = _kernel_case("float32", 3, 2, 4099, 96)
    f32, f64 = torch.float32, torch.float64
    tail = [dev(v, f64) for v in (z, ell, Q)]
    runs = [(H.sgp_kgrad, [dev(X, f32), dev(Y, f32)] + tail + [dev(Rw, f64)], plain[2], 2),
            (H.sgp_wkgrad, [dev(X, f32), dev(w, f64), dev(rr, f64)] + tail + [dev(R1, f64)], weighted[2], 1)]
    for fn, args, scale, P in runs:
        _, _, xs = fn(*args, x_grad=True)
        H.debug_set("sgp_kgrad_plain", 1)
        try:
            _, _, xp = fn(*args, x_grad=True)
        finally:
            H.debug_clear()
        err = float((xs - xp).abs().max().cpu())
        print("strips vs plain (%s): %.3e, abs-scale %.3e, bound %.3e" % (fn.__name__, err, scale, 4 * KX.gamma(96, P) * scale))
        assert err <= 4.0 * KX.gamma(96, P) * scale
    with pytest.raises(ValueError):
        H.sgp_kgrad(runs[0][1][0], runs[0][1][1][:100].contiguous(), *runs[0][1][2:], x_grad=True)


# ------------------------------------------------------------------------------------------------ 2. end to end
class _OnlyGP(hb.model.Model):
    def setUp(self, Z, ell):
        self.gp = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(ell), z=Z)


def _stored(m, a):
    """`a` as the session stores it, in double."""
    return np.asarray(a, dtype=m._session.np_dtype).astype(np.float64)


@pytest.mark.parametrize("dtype, residual", [("float64", "diagonal"), ("float64", "neglected"), ("float32", "diagonal"),
                                             ("float32", "neglected")])
def test_collapsed_bound_and_grad_input_gradient_against_autograd(dtype, residual):
    """SparseGP.collapsed_bound_and_grad(x_grad=True)["X"] at N = 4099, M = 32, d = 3 (ARD) against torch.autograd of
    the bound on the inputs as the session stores them; float64 arithmetic in either session, so the same rule.  The
    other entries and the value are the bits of x_grad=False, whose dict holds no "X".
    Observed on MI355X (device error / CPU gap / bound): float64 'diagonal' 6.3e-13 / 6.4e-13 / 3.3e-10 (max|dF/dX| 25.6,
    abs-scale 9.1e3); 'neglected' 7.2e-13 / 8.3e-13 / 3.0e-10; float32 session 5.3e-13 / 6.1e-13 and 6.0e-13 / 6.5e-13."""
    N, M, d, P = 4099, 32, 3, 2
    X, Y, z, ell = C.case(N, M, d, P, seed=7)
    m = _OnlyGP(Z=z, ell=ell, dtype=dtype)
    m.initialize()
    s2, k = 0.09, 1.3
    val, g = m.gp.collapsed_bound_and_grad(X, Y, s2, k, residual=residual, x_grad=True)
    val0, g0 = m.gp.collapsed_bound_and_grad(X, Y, s2, k, residual=residual)
    assert set(g0) == {"z", "lengthscales", "noise_var", "k_var"} and set(g) == set(g0) | {"X"}
    assert val == val0 and all(np.array_equal(g[n], g0[n]) for n in g0)
    assert g["X"].dtype == np.float64 and g["X"].shape == (N, d)
    Xs, Ys, zs, es = _stored(m, X), _stored(m, Y), _stored(m, z), _stored(m, m.gp.kern.lengthscales.value).reshape(-1)
    r = C.bound_and_grad(Xs, Ys, zs, es, JITTER, s2, k, residual)
    ref = KX.bound_autograd_x(Xs, Ys, zs, es, JITTER, s2, k, residual)
    gap = np.abs(KX.streamed_x(Xs, Ys, zs, es, r["Q"], r["R"]) - ref).max()
    scale = KX.abs_scale(Xs, Ys, zs, es, r["Q"], r["R"]).max()
    err, bnd = np.abs(g["X"] - ref).max(), KX.bound(gap, scale, M, P)
    print("collapsed_bound_and_grad(x_grad) %s %s: device %.3e, CPU gap %.3e, abs-scale %.3e (max|dF/dX| %.3e), bound %.3e"
          % (dtype, residual, err, gap, scale, np.abs(ref).max(), bnd))
    assert err <= bnd


def test_input_gradient_against_the_psi_route_at_zero_variance():
    """A second, independent device route: psi_bound_and_grad(X, 0.0, Y, ..)["X_mean"] at N = 97, M = 32, d = 2 (double
    exponentials on the vector unit) against collapsed_bound_and_grad(x_grad=True)["X"]; the same rule.
    Observed on MI355X: 1.36e-9 between the routes (against autograd: this route 1.1e-11, the psi route 1.36e-9), CPU gap
    1.4e-11, abs-scale 6.8e5, bound 2.4e-8."""
    N, M, d, P = 97, 32, 2, 1
    rng = np.random.RandomState(11)
    X, z = rng.uniform(0, 4, (N, d)), rng.uniform(0, 4, (M, d))
    Y = np.sin(X.sum(1, keepdims=True)) + 0.3 * rng.randn(N, P)
    ell = np.array([0.9, 1.1])
    m = _OnlyGP(Z=z, ell=ell, dtype="float64")
    m.initialize()
    s2, k = 0.09, 1.3
    _, g = m.gp.collapsed_bound_and_grad(X, Y, s2, k, x_grad=True)
    _, gp = m.gp.psi_bound_and_grad(X, 0.0, Y, s2, k)
    r = C.bound_and_grad(X, Y, z, ell, JITTER, s2, k)
    ref = KX.bound_autograd_x(X, Y, z, ell, JITTER, s2, k)
    gap = np.abs(KX.streamed_x(X, Y, z, ell, r["Q"], r["R"]) - ref).max()
    scale = KX.abs_scale(X, Y, z, ell, r["Q"], r["R"]).max()
    err, bnd = np.abs(g["X"] - gp["X_mean"]).max(), KX.bound(gap, scale, M, P)
    print("x_grad against the psi route: %.3e (against autograd: %.3e and %.3e), CPU gap %.3e, abs-scale %.3e, bound %.3e"
          % (err, np.abs(g["X"] - ref).max(), np.abs(gp["X_mean"] - ref).max(), gap, scale, bnd))
    assert err <= bnd and np.abs(g["X"] - ref).max() <= bnd


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("lik", [SR.BERNOULLI, SR.POISSON])
def test_elbo_and_grad_input_gradient_against_autograd(lik, dtype):
    """SparseGP.elbo_and_grad(x_grad=True)["X"] at N = 4099, M = 32, at the q of 3 natgrad_q steps from the prior, against
    torch.autograd of elbo_grad_ref's torch objective with X.requires_grad.  Tolerance: the one test_elbo_grad_gpu.py
    applies to its z gradient, 4 x max(CPU gap, 1e-10 x scale), with the abs-scale of xbar (Bernoulli: the gap holds
    the Stein-versus-quadrature difference).  The other entries are the bits of x_grad=False.
    Observed on MI355X (device error / CPU gap / bound): Bernoulli 2.9e-13 / 3.3e-13 / 1.6e-8 (float32 session 3.0e-13 /
    1.7e-13); Poisson 1.4e-12 / 2.2e-12 / 2.0e-6 (float32 session 3.8e-12 / 2.5e-12)."""
    N, M = 4099, 32
    X, y, Z = SR.problem(lik, N=N, M=M)
    m = SVGPLik(X=X, Y=y, Z=Z, likelihood=LIKS[lik](), dtype=dtype)
    m.gp.kern.lengthscales = SR.ELL.copy()
    m.k_var = np.ones(1) * SR.K_VAR
    m.initialize()
    gp = object.__getattribute__(m, "gp")
    Xm, Ym = object.__getattribute__(m, "X"), object.__getattribute__(m, "Y")
    qm, qS, _ = gp.natgrad_q(Xm, Ym, LIKS[lik](), k_var=SR.K_VAR, steps=3, tol=0.0)
    val, g = gp.elbo_and_grad(Xm, Ym, LIKS[lik](), (qm, qS), k_var=SR.K_VAR, x_grad=True)
    val0, g0 = gp.elbo_and_grad(Xm, Ym, LIKS[lik](), (qm, qS), k_var=SR.K_VAR)
    assert set(g0) == {"z", "lengthscales", "k_var"} and set(g) == set(g0) | {"X"}
    assert val == val0 and all(np.array_equal(g[n], g0[n]) for n in g0)
    assert g["X"].dtype == np.float64 and g["X"].shape == (N, 1)
    Xs, ys, zs, es = _stored(m, X), _stored(m, y), _stored(m, Z), _stored(m, m.gp.kern.lengthscales.value).reshape(-1)
    r = E.elbo_and_grad(Xs, ys, zs, es, JITTER, lik, qm, qS, 1.0, SR.K_VAR)
    ref = KX.elbo_autograd_x(Xs, ys, zs, es, JITTER, lik, qm, qS, 1.0, SR.K_VAR)
    gap = np.abs(KX.streamed_x_w(Xs, r["w"], r["r"], zs, es, r["Q"], r["R"]) - ref).max()
    scale = KX.abs_scale(Xs, r["r"][:, None], zs, es, r["Q"], r["R"], w=r["w"]).max()
    err, bnd = np.abs(g["X"] - ref).max(), 4.0 * max(gap, 1e-10 * scale)
    print("elbo_and_grad(x_grad) lik %d %s: device %.3e, CPU gap %.3e, abs-scale %.3e (max|dF/dX| %.3e), bound %.3e"
          % (lik, dtype, err, gap, scale, np.abs(ref).max(), bnd))
    assert err <= bnd
