"""Hyper-parameter gradient of the ELBO at a fixed q(u) on the GPU: hb_sgp_wkgrad, SparseGP.elbo_and_grad,
SVGPLik.elbo_and_grad and SVGPLik.fit_hyper against the numpy restatement tests/elbo_grad_ref.py (itself pinned on the
host by tests/test_elbo_grad_cpu.py against autograd and central differences).

Bounds are built as in test_collapsed_grad_gpu.py.  Each gradient bound is 4 x the gap between the two independent
float64 CPU evaluations (restatement against torch.autograd) ON THE SAME INPUTS, the gap floored at 1e-10 x the
cancelling scale max|streamed part| + max|K(z, z) part|; k_var's floor is 1e-10 x the sum of its absolute terms.  For
the kernel the autograd side differentiates the surrogate sum_j (r_j mu_j - w_j v_j / 2) of the drawn weights; for the
likelihoods it differentiates the ELBO (Bernoulli: the gap then holds the Stein-versus-quadrature difference, 1e-9 ..
1e-8 of the gradient, test_elbo_grad_cpu.py).  Model level: 4 x the error the same central difference makes on the CPU
restatement at the same h.  Every figure is printed before it is asserted.

Observed on MI355X: in the docstrings of the tests; profiles/sgp_elbo_grad.txt holds every printed line."""
import functools

import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd import graph as G
from henbun_amd import hip_ops as H
from henbun_amd.models import SVGP, SVGPLik, svgp_data

import collapsed_grad_ref as C
import elbo_grad_ref as E
import optimal_q_ref as R
import sites_ref as SR

pytestmark = pytest.mark.gpu

JITTER = 1e-5
LIKS = {SR.BERNOULLI: hb.likelihoods.Bernoulli, SR.POISSON: hb.likelihoods.Poisson}


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def _bound(gap, scale):
    return 4.0 * max(gap, 1e-10 * scale)


def _scales(r):
    return (np.abs(r["z_streamed"]).max() + np.abs(r["z_kmm"]).max(),
            np.abs(r["ell_streamed"]).max() + np.abs(r["ell_kmm"]).max())


# ------------------------------------------------------------------------------------------------ 1. the kernel
@functools.lru_cache(maxsize=4)
def _kernel_case(dtype, d, N, M, scalar_ell=False):
    """Inputs (X rounded to the storage type; w with both signs and exact zeros) and the two CPU evaluations on them."""
    npdt = np.float64 if dtype == "float64" else np.float32
    X, Y, z, ell = C.case(N, M, d, 1, seed=N + M + d, scalar_ell=scalar_ell)
    X = X.astype(npdt).astype(np.float64)
    Y = Y.astype(npdt).astype(np.float64)
    w, rr = E.weights_case(N, N + M + d)
    m, S = E.q_case(M, N + d)
    r = E.grad_from_weights(X, w, rr, z, ell, JITTER, m, S, 1.3)
    a = E.surrogate_autograd(X, w, rr, z, ell, JITTER, m, S, 1.3)
    return X, Y, z, ell, r, a


def _check_wkgrad(dtype, d, N, M, scalar_ell):
    dt = torch.float64 if dtype == "float64" else torch.float32
    X, _, z, ell, r, a = _kernel_case(dtype, d, N, M, scalar_ell)
    assert ell.shape == ((1,) if scalar_ell or d == 1 else (d,))
    if N > 50:
        assert (r["w"] == 0).any() and (r["w"] < 0).any() and (r["w"] > 0).any()
    args = [dev(X, dt)] + [dev(v, torch.float64) for v in (r["w"], r["r"], z, ell, r["Q"], r["R"])]
    zb, eb = H.sgp_wkgrad(*args)
    zb2, eb2 = H.sgp_wkgrad(*args)
    torch.cuda.synchronize()
    assert zb.dtype == torch.float64 and eb.dtype == torch.float64
    assert torch.equal(zb, zb2) and torch.equal(eb, eb2)
    zb, eb = zb.cpu().numpy(), eb.cpu().numpy()
    assert zb.shape == (M, d) and eb.shape == ell.shape
    zs, es = _scales(r)
    gz, ge = np.abs(r["z"] - a["z"]).max(), np.abs(r["lengthscales"] - a["lengthscales"]).max()
    ez, ee = np.abs(zb - r["z_streamed"]).max(), np.abs(eb - r["ell_streamed"]).max()
    print("sgp_wkgrad %s N=%d M=%d d=%d dl=%d: z: device %.3e, CPU gap %.3e, scale %.3e (max|grad| %.3e), bound %.3e; "
          "ell: device %.3e, CPU gap %.3e, scale %.3e, bound %.3e"
          % (dtype, N, M, d, ell.size, ez, gz, zs, np.abs(r["z"]).max(), _bound(gz, zs), ee, ge, es, _bound(ge, es)))
    assert np.all(np.isfinite(zb)) and np.all(np.isfinite(eb))
    assert ez <= _bound(gz, zs)
    assert ee <= _bound(ge, es)


@pytest.mark.parametrize("M", [32, 512, 50])
@pytest.mark.parametrize("N", [1, 97, 40001])
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_sgp_wkgrad_against_the_restatement(dtype, d, N, M):
    """hb_sgp_wkgrad_f64 / _f32 against the restatement's streamed part on the same Q, R, w, r; two runs bitwise equal.
    M = 32, 512 take the column-strip MFMA form (512: the largest LDS shape), M = 50 the plain loops; N = 1 is a single
    ragged step, 97 leaves a ragged tail, 40001 gives more steps than workgroups with uneven runs.
    Observed on MI355X (36 cases): device error of zbar <= 0.037 % of its bound (worst: float32, N = 1, M = 512, d = 3:
    5.4e-11 against 1.5e-7) and <= 1.5e-13 of the cancelling scale; of ellbar <= 12 % of its bound (float64, N = 40001,
    M = 512, d = 3: 1.0e-8 against 8.7e-8) and <= 4.7e-11 of the scale.  Worst per M (fraction of the bound, zbar /
    ellbar): 32: 7.7e-6 / 1.7e-3; 512: 3.6e-4 / 1.2e-1; 50 (plain loops): 1.4e-4 / 2.1e-3."""
    _check_wkgrad(dtype, d, N, M, False)


@pytest.mark.parametrize("M", [32, 512, 50])
@pytest.mark.parametrize("N", [1, 97, 40001])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_sgp_wkgrad_one_shared_lengthscale_in_three_dimensions(dtype, N, M):
    """d = 3 with ONE lengthscale (dl = 1 < d: ellbar [1] is the sum over the dimensions, the shape models.SVGPLik has);
    same bounds.
    Observed on MI355X (18 cases): zbar <= 0.019 % of its bound (7.8e-14 of the cancelling scale); ellbar <= 18 % of its
    bound (float64, N = 40001, M = 512: 1.3e-8 against 7.5e-8; 7.2e-11 of the scale)."""
    _check_wkgrad(dtype, 3, N, M, True)


@pytest.mark.parametrize("M, plain", [(96, False), (96, True), (50, False)])
def test_sgp_wkgrad_with_unit_weights_has_the_bits_of_sgp_kgrad(M, plain):
    """w == 1, r = Y[:, 0]: the bits of hb_sgp_kgrad at P = 1 (x * 1.0 is exact and every other operation is shared), in
    the strip form, in the plain form forced on the same aligned shape, and in the plain form of an unaligned one.
    Observed on MI355X: 0 differing entries in all three (max|zbar| 7.5e3 at M = 96, 1.8e3 at M = 50)."""
    X, Y, z, ell, r, _ = _kernel_case("float32", 3, 4097, M)
    N = X.shape[0]
    base = [dev(v, torch.float64) for v in (z, ell, r["Q"], r["R"])]
    Xd, Yd = dev(X, torch.float32), dev(Y, torch.float32)
    ones, y0 = torch.ones(N, dtype=torch.float64, device="cuda"), dev(Y[:, 0], torch.float64)
    if plain:
        H.debug_set("sgp_kgrad_plain", 1)
    try:
        zk, ek = H.sgp_kgrad(Xd, Yd, *base)
        zw, ew = H.sgp_wkgrad(Xd, ones, y0, *base)
    finally:
        H.debug_clear()
    torch.cuda.synchronize()
    print("unit weights M=%d plain=%s: max|zbar| %.3e, differing entries %d / %d"
          % (M, plain, float(zk.abs().max().cpu()), int((zk != zw).sum().cpu()), int((ek != ew).sum().cpu())))
    assert float(zk.abs().max().cpu()) > 0
    assert torch.equal(zk, zw) and torch.equal(ek, ew)


def test_sgp_wkgrad_plain_form_agrees_with_the_strips_and_checks_its_operands():
    """The diagnostic switch runs an aligned shape through the plain loops: the same numbers to summation order
    (4e-10 of the cancelling scale, as for hb_sgp_kgrad).
    Observed on MI355X: zbar 2.3e-12 at scale 2.2e3 (1.0e-15 of it), ellbar 2.4e-12 at scale 61 (3.9e-14)."""
    X, _, z, ell, r, a = _kernel_case("float32", 3, 4097, 96)
    args = [dev(X, torch.float32)] + [dev(v, torch.float64) for v in (r["w"], r["r"], z, ell, r["Q"], r["R"])]
    zf, ef = H.sgp_wkgrad(*args)
    H.debug_set("sgp_kgrad_plain", 1)
    try:
        zp, ep = H.sgp_wkgrad(*args)
    finally:
        H.debug_clear()
    zs, es = _scales(r)
    ez, ee = float((zf - zp).abs().max().cpu()), float((ef - ep).abs().max().cpu())
    print("strips vs plain: z %.3e (scale %.3e) ell %.3e (scale %.3e)" % (ez, zs, ee, es))
    assert ez <= 4e-10 * zs and ee <= 4e-10 * es
    with pytest.raises(TypeError):
        H.sgp_wkgrad(args[0], args[1].float(), *args[2:])
    with pytest.raises(TypeError):
        H.sgp_wkgrad(args[0], args[1], args[2], args[3].float(), *args[4:])
    with pytest.raises(ValueError):
        H.sgp_wkgrad(args[0], args[1][:100].contiguous(), *args[2:])
    with pytest.raises(ValueError):
        H.sgp_wkgrad(*args[:6], torch.cat([args[6], args[6]], 1).contiguous())


# ------------------------------------------------------------------------------------------------ 2. end to end
def _lik_model(lik, N, M, dtype, residual="diagonal", ell=None):
    X, y, Z = SR.problem(lik, N=N, M=M)
    m = SVGPLik(X=X, Y=y, Z=Z, likelihood=LIKS[lik](), residual=residual, dtype=dtype)
    m.gp.kern.lengthscales = SR.ELL.copy() if ell is None else np.ones(1) * ell
    m.k_var = np.ones(1) * SR.K_VAR
    m.initialize()
    return m, X, y, Z


def _stored(m, a):
    """`a` as the session stores it, in double."""
    return np.asarray(a, dtype=m._session.np_dtype).astype(np.float64)


def _rows(g, r, a):
    """(name, device error, CPU gap, floor scale, size) per gradient."""
    zs, es = _scales(r)
    return [("z", np.abs(g["z"] - r["z"]).max(), np.abs(r["z"] - a["z"]).max(), zs, np.abs(r["z"]).max()),
            ("lengthscales", np.abs(g["lengthscales"] - r["lengthscales"]).max(),
             np.abs(r["lengthscales"] - a["lengthscales"]).max(), es, np.abs(r["lengthscales"]).max()),
            ("k_var", abs(g["k_var"] - r["k_var"]), abs(r["k_var"] - a["k_var"]), r["k_var_abs"], abs(r["k_var"]))]


def _print_rows(rows):
    for name, err, gap, scale, size in rows:
        print("   %-12s device %.3e, CPU gap %.3e, cancelling scale %.3e (max|grad| %.3e), bound %.3e"
              % (name, err, gap, scale, size, _bound(gap, scale)))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("lik", [SR.BERNOULLI, SR.POISSON])
def test_elbo_and_grad_against_the_restatement(lik, dtype):
    """SparseGP.elbo_and_grad at N = 20000, M = 64, jitter_level 1e-5 in a float64 and a float32 session (float64
    arithmetic either way: the SAME bounds), at the q of 3 natgrad_q steps from the prior -- not converged, so the
    partial gradient is tested away from the optimum.  Gradients: 4 x the CPU gap (floored); value: 1e-8 relative.
    Observed on MI355X (device error / CPU gap / bound): Bernoulli float64: value 8.9e-16 relative; z 1.7e-10 / 7.5e-11 /
    2.1e-8 (max|z gradient| 0.030, cancelling scale 53); lengthscales 1.4e-10 / 1.6e-9 / 6.1e-8; k_var 1.2e-11 / 7.2e-13 /
    9.3e-9.  Bernoulli float32 session: value 3.8e-15; z 8.8e-11 / 3.5e-11 / 2.1e-8; lengthscales 1.6e-10 / 3.6e-10 /
    6.2e-8; k_var 1.4e-11 / 9.4e-12 / 9.3e-9.  Poisson float64: value 4.4e-15; z 1.1e-9 / 5.0e-10 / 2.3e-7 (max 24.4,
    scale 575); lengthscales 1.0e-9 / 8.2e-9 / 7.5e-8; k_var 2.9e-10 / 2.2e-10 / 3.4e-8.  Poisson float32 session: value
    1.2e-14; z 2.3e-9 / 4.9e-10 / 2.3e-7; lengthscales 1.8e-9 / 2.8e-9 / 7.6e-8; k_var 7.8e-11 / 3.0e-10 / 3.4e-8.  The
    natural-gradient residual at the q used: 2.6e-3 (Bernoulli), 0.12 (Poisson)."""
    N, M = 20000, 64
    assert hb.settings.numerics.jitter_level == JITTER
    m, X, y, Z = _lik_model(lik, N, M, dtype)
    gp = object.__getattribute__(m, "gp")
    Xm, Ym = object.__getattribute__(m, "X"), object.__getattribute__(m, "Y")
    qm, qS, info = gp.natgrad_q(Xm, Ym, LIKS[lik](), k_var=SR.K_VAR, steps=3, tol=0.0)
    assert info["residual"][-1] > 1e-6                                   # not at the fixed point
    val, g = gp.elbo_and_grad(Xm, Ym, LIKS[lik](), (qm, qS), k_var=SR.K_VAR)
    assert isinstance(val, float) and g["z"].dtype == np.float64 and g["z"].shape == (M, 1)
    assert g["lengthscales"].shape == (1,) and isinstance(g["k_var"], float) and set(g) == {"z", "lengthscales", "k_var"}
    Xs, ys, zs_, ells = _stored(m, X), _stored(m, y), _stored(m, Z), _stored(m, m.gp.kern.lengthscales.value).reshape(-1)
    r = E.elbo_and_grad(Xs, ys, zs_, ells, JITTER, lik, qm, qS, 1.0, SR.K_VAR)
    a = E.elbo_autograd(Xs, ys, zs_, ells, JITTER, lik, qm, qS, 1.0, SR.K_VAR)
    rows = _rows(g, r, a)
    print("elbo_and_grad lik %d %s: value %.9f ref %.9f (rel %.2e); natgrad residual %.2e"
          % (lik, dtype, val, r["value"], abs(val / r["value"] - 1), info["residual"][-1]))
    _print_rows(rows)
    assert abs(val - r["value"]) <= 1e-8 * abs(r["value"])
    for name, err, gap, scale, size in rows:
        assert err <= _bound(gap, scale), name
    # two calls: the same bits
    val2, g2 = gp.elbo_and_grad(Xm, Ym, LIKS[lik](), (qm, qS), k_var=SR.K_VAR)
    assert val2 == val and all(np.array_equal(g[n], g2[n]) for n in g)


def test_envelope_gaussian_at_the_optimal_q_is_the_gradient_of_the_collapsed_bound():
    """Gaussian likelihood, float64, N = 4096, M = 32, q = the device's optimal_q: the value equals
    collapsed_bound_and_grad's to 1e-8 relative, and z / lengthscales / k_var agree within 4 x the gap the two CPU
    restatements show for the same comparison, floored at 1e-10 x the sum of the two cancelling scales.
    Observed on MI355X (device gap / CPU gap / bound): value 4.4e-16 relative; z 4.4e-10 / 1.3e-10 / 1.3e-7 (max|z
    gradient| 0.116, summed scales 318); lengthscales 3.4e-10 / 2.7e-10 / 1.2e-7 (gradient 49.1); k_var 1.1e-11 / 2.1e-12 /
    1.6e-6 (gradient 7.29)."""
    N, M, s2, k = 4096, 32, 0.4, 1.3
    X, Y, Z = svgp_data(N, M, 0)
    m = SVGP(X=X, Y=Y, Z=Z, q_shape="fullrank", dtype="float64")
    m.gp.kern.lengthscales = np.ones(1) * 0.9
    m.initialize()
    gp = object.__getattribute__(m, "gp")
    qm, qS = gp.optimal_q(X, Y, s2, k)
    cval, cg = gp.collapsed_bound_and_grad(X, Y, s2, k)
    val, g = gp.elbo_and_grad(X, Y, hb.likelihoods.Gaussian(s2), (qm, qS), k_var=k)
    ell = np.ones(1) * 0.9
    c = C.bound_and_grad(X, Y, Z, ell, JITTER, s2, k)
    rm, rS, _, _ = R.optimal_q(c["Phi"], c["b"], s2, k)
    r = E.elbo_and_grad(X, Y, Z, ell, JITTER, E.GAUSSIAN, rm, rS, s2, k)
    zs, es = (p + q for p, q in zip(_scales(r), _scales(c)))
    rows = [("z", np.abs(g["z"] - cg["z"]).max(), np.abs(r["z"] - c["z"]).max(), zs, np.abs(c["z"]).max()),
            ("lengthscales", np.abs(g["lengthscales"] - cg["lengthscales"]).max(),
             np.abs(r["lengthscales"] - c["lengthscales"]).max(), es, np.abs(c["lengthscales"]).max()),
            ("k_var", abs(g["k_var"] - cg["k_var"]), abs(r["k_var"] - c["k_var"]), r["k_var_abs"] + c["k_var_abs"],
             abs(c["k_var"]))]
    print("envelope: elbo_and_grad value %.9f, collapsed_bound_and_grad %.9f (rel %.2e), CPU %.9f"
          % (val, cval, abs(val / cval - 1), c["value"]))
    _print_rows(rows)
    assert abs(val - cval) <= 1e-8 * abs(cval)
    for name, err, gap, scale, size in rows:
        assert err <= _bound(gap, scale), name


# ------------------------------------------------------------------------------------------------ 3. model level
def _raw_of(m):
    return {n: m._session.read_raw(v).copy() for n, v in m._hyper_variables().items()}


def test_svgplik_gradient_against_central_differences_of_its_own_value():
    """SVGPLik.elbo_and_grad() (raw parameters, through the transforms) in a float64 Bernoulli model at the q of 3
    natural-gradient steps, against directional central differences of the device's own VALUE along a random raw-space
    direction per parameter group.  Bound: 4 x the error the same difference makes on the CPU restatement at the same h.
    Observed on MI355X (h = 0.01; value -1746.1256, equal to the restatement's to the last digit; |analytic - difference| on
    the device / bound): z 7.95e-5 / 3.18e-4 (directional derivative 3.83e-3); lengthscales 1.250e-2 / 5.00e-2 (-5.464);
    k_var 1.822e-4 / 7.29e-4 (0.7109): the device makes the CPU restatement's truncation error to four digits or more."""
    lik, N, M, h = SR.BERNOULLI, 3000, 32, 1e-2
    m, X, y, Z = _lik_model(lik, N, M, "float64", ell=1.2)
    m.reset_q()
    m.fit_q(steps=3, tol=0.0)
    T = hb.transforms.positive
    val, g = m.elbo_and_grad()
    raw0 = _raw_of(m)
    assert set(g) == {"z", "lengthscales", "k_var"} and all(g[n].shape == raw0[n].shape for n in g)
    qm, (qS,) = m._current_blocks()
    hv = m._hyper_variables()

    def f_dev(name, x):
        m._session.write_raw(hv[name], x)
        try:
            return m.elbo_and_grad()[0]
        finally:
            m._session.write_raw(hv[name], raw0[name])

    def cons(p):
        return p["z"], T.forward(p["lengthscales"]).reshape(-1), float(T.forward(p["k_var"]).reshape(-1)[0])

    def f_ref(name, x):
        p = dict(raw0)
        p[name] = x
        z_, ell_, k_ = cons(p)
        _, W = R.chol_factor(z_, ell_, JITTER)
        mu, v = E.marginals(qm, qS, R.A_of(W, z_, X, ell_), k_)
        return float(SR.sites(lik, y, mu, v)[0].sum()) - E.kl(qm, qS)

    z0, ell0, k0 = cons(raw0)
    r = E.elbo_and_grad(X, y, z0, ell0, JITTER, lik, qm, qS, 1.0, k0)
    print("SVGPLik.elbo_and_grad: value %.9f, restatement %.9f (rel %.2e)" % (val, r["value"], abs(val / r["value"] - 1)))
    assert abs(val - r["value"]) <= 1e-8 * abs(r["value"])
    g_ref = dict(z=r["z"], lengthscales=r["lengthscales"] * T.dforward(raw0["lengthscales"]),
                 k_var=r["k_var"] * T.dforward(raw0["k_var"]))
    rng = np.random.RandomState(3)
    rows = []
    for name in ("z", "lengthscales", "k_var"):
        u = np.asarray(rng.standard_normal(raw0[name].shape))
        u = u / np.sqrt((u * u).sum())
        fd_dev = C.directional_fd(lambda x: f_dev(name, x), raw0[name], u, h)
        fd_ref = C.directional_fd(lambda x: f_ref(name, x), raw0[name], u, h)
        an_dev, an_ref = float((g[name] * u).sum()), float((np.reshape(g_ref[name], u.shape) * u).sum())
        rows.append((name, abs(an_dev - fd_dev), 4.0 * abs(an_ref - fd_ref)))
        print("%-12s analytic (device) %.9e, central difference of the device's value %.9e (h = %g): |gap| %.3e; the same "
              "on the CPU restatement: analytic %.9e difference %.9e; bound %.3e"
              % (name, an_dev, fd_dev, h, abs(an_dev - fd_dev), an_ref, fd_ref, rows[-1][2]))
    for name, err, bound in rows:
        assert err <= bound, name


# ------------------------------------------------------------------------------------------------ 4. behaviour
def test_fit_hyper_climbs_the_elbo_and_leaves_the_fitted_q():
    """Bernoulli on sites_ref.problem(N = 3000, M = 32) with the lengthscale started at 3 x its generating value:
    fit_hyper(steps=40, lr=0.05) returns a finite trace of steps + 1 entries whose last entry exceeds the first and
    equals the ELBO a fit_q() run afterwards reports, to 1e-8 relative (float64 model); train_z=False leaves z alone.
    q(u) is first set to the prior (reset_q): from the random q(u) of a fresh model a full step overshoots.
    Observed on MI355X: ELBO -1775.3808 -> -1744.9447 in 40 steps (ell 2.7 -> 1.679, k_var 1.3 -> 2.214, max|dz| 1.31); the
    fit_q() afterwards stops after 1 step at -1744.9447, 8.5e-14 relative from the trace's last entry; float32 model, 3
    steps, z fixed: -1775.3979 -> -1764.8423."""
    m, X, y, Z = _lik_model(SR.BERNOULLI, 3000, 32, "float64", ell=3.0 * SR.ELL[0])
    m.reset_q()
    z0 = m.gp.z.value.copy()
    trace = m.fit_hyper(steps=40, lr=0.05)
    _, _, info = m.fit_q()
    print("fit_hyper: %.6f -> %.6f in 40 steps (fit_q afterwards: %.6f after %d steps, rel %.2e); ell %.4f -> %.4f, k_var "
          "%.4f -> %.4f, max|dz| %.3e" % (trace[0], trace[-1], info["elbo"][-1], info["steps"],
                                           abs(trace[-1] / info["elbo"][-1] - 1), 3.0 * SR.ELL[0],
                                           m.gp.kern.lengthscales.value[0], SR.K_VAR, m.k_var.value[0],
                                           np.abs(m.gp.z.value - z0).max()))
    assert trace.shape == (41,) and np.all(np.isfinite(trace))
    assert trace[-1] > trace[0]
    assert abs(trace[-1] - info["elbo"][-1]) <= 1e-8 * abs(info["elbo"][-1])
    assert np.abs(m.gp.z.value - z0).max() > 0
    m2, _, _, _ = _lik_model(SR.BERNOULLI, 3000, 32, "float32", ell=3.0 * SR.ELL[0])
    m2.reset_q()
    z0 = m2.gp.z.value.copy()
    t2 = m2.fit_hyper(steps=3, lr=0.05, train_z=False, q_steps=2)
    print("   float32 model, train_z=False: %.6f -> %.6f" % (t2[0], t2[-1]))
    assert t2.shape == (4,) and np.all(np.isfinite(t2)) and np.array_equal(m2.gp.z.value, z0)


def test_fit_hyper_restores_the_parameters_when_a_factorisation_fails(monkeypatch):
    """A factorisation that fails on the THIRD evaluation: the raw parameters are those of the last successful
    evaluation, not the initial ones and not the stepped ones."""
    m, X, y, Z = _lik_model(SR.BERNOULLI, 3000, 32, "float64", ell=3.0 * SR.ELL[0])
    m.reset_q()
    real = SVGPLik.elbo_and_grad
    seen = []

    def failing_third(self):
        if len(seen) == 2:
            seen.append(_raw_of(self))
            raise G.CholeskyError("injected: K(z, z) is not positive definite")
        out = real(self)
        seen.append(_raw_of(self))
        return out

    monkeypatch.setattr(SVGPLik, "elbo_and_grad", failing_third)
    with pytest.raises(G.CholeskyError, match="injected"):
        m.fit_hyper(steps=5, lr=0.05, q_steps=2)
    after = _raw_of(m)
    assert len(seen) == 3
    for n in after:
        assert np.array_equal(after[n], seen[1][n]), n                      # the last successful evaluation
        assert not np.array_equal(seen[2][n], seen[1][n]), n                # the failing step had moved them
        assert not np.array_equal(seen[0][n], seen[1][n]), n


def test_elbo_and_grad_refuses_what_it_does_not_cover():
    m, X, y, Z = _lik_model(SR.BERNOULLI, 3000, 32, "float64")
    lik = hb.likelihoods.Bernoulli()
    q = (np.zeros((1, 32)), np.eye(32))
    with pytest.raises(NotImplementedError, match="fullrank"):
        m.gp.elbo_and_grad(X, y, lik, q, residual="fullrank")
    with pytest.raises(NotImplementedError, match="mean-field"):
        m.gp.elbo_and_grad(X, y, lik, (np.zeros((1, 32)), np.ones(32)))
    with pytest.raises(NotImplementedError, match="one latent function"):
        m.gp.elbo_and_grad(X, np.concatenate([y, y], 1), lik, q)
    with pytest.raises(TypeError):
        m.gp.elbo_and_grad(X, y, "bernoulli", q)
    with pytest.raises(ValueError):
        m.gp.elbo_and_grad(X, y, lik, q, k_var=-1.0)

    class Other(hb.model.Model):
        def setUp(self, Z, kern):
            self.gp = hb.gp.SparseGP(kern=kern, z=Z)

    with pytest.raises(NotImplementedError, match="UnitRBF"):
        Other(Z=Z, kern=hb.gp.kernels.UnitMatern52(np.ones(1)), dtype="float64").gp.elbo_and_grad(X, y, lik, q)
    with pytest.raises(NotImplementedError, match="one expert"):
        Other(Z=np.stack([Z, Z]), kern=hb.gp.kernels.UnitRBF(np.ones((2, 1))), dtype="float64").gp.elbo_and_grad(X, y, lik, q)
    cfg = hb.settings.get_settings()
    cfg.numerics.jitter_level = 0.0
    with hb.settings.temp_settings(cfg):
        bad = SVGPLik(X=X, Y=y, Z=np.zeros((32, 1)), likelihood=lik, dtype="float64")
        with pytest.raises(G.CholeskyError):
            bad.gp.elbo_and_grad(X, y, lik, q)
