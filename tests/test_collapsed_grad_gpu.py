"""Gradient of the collapsed bound on the GPU: hb_sgp_kgrad, SparseGP.collapsed_bound_and_grad, SVGP.collapsed_bound_and_grad
and SVGP.fit_hyper against the numpy restatement tests/collapsed_grad_ref.py (itself pinned on the host by
tests/test_collapsed_grad_cpu.py against autograd and central differences).

Bounds are not constants.  Each gradient bound is 4 x the gap between the two independent float64 CPU evaluations
(restatement against torch.autograd) ON THE SAME INPUTS, the gap floored at 1e-10 x the cancelling scale
max|streamed part| + max|Kmm part| (the z gradient is the difference of those two parts, each about 1000 times
larger); the factor 4 covers the order of summation, as in test_optimal_q_gpu.py.  The scalars' floor is 1e-10 x the sum
of their absolute terms.  Model level: 4 x the error the same central difference makes on the CPU restatement at the
same h.  Every figure is printed before it is asserted.

Observed on MI355X: in the docstrings of the tests; profiles/sgp_cbgrad.txt holds every printed line."""
import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd import graph as G
from henbun_amd import hip_ops as H
from henbun_amd.models import SVGP, svgp_data

import collapsed_grad_ref as C
import optimal_q_ref as R

pytestmark = pytest.mark.gpu
tf = hb.tf

JITTER = 1e-5


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def _bound(gap, scale):
    return 4.0 * max(gap, 1e-10 * scale)


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _kernel_case(dtype, d, P, N, M, scalar_ell=False):
    """Inputs (X, Y rounded to the storage type) and the two CPU evaluations on them."""
    npdt = np.float64 if dtype == "float64" else np.float32
    X, Y, z, ell = C.case(N, M, d, P, seed=N + M + d + P, scalar_ell=scalar_ell)
    X, Y = X.astype(npdt).astype(np.float64), Y.astype(npdt).astype(np.float64)
    r = C.bound_and_grad(X, Y, z, ell, JITTER, 0.09, 1.0)
    a = C.bound_autograd(X, Y, z, ell, JITTER, 0.09, 1.0)
    return X, Y, z, ell, r, a


@pytest.mark.parametrize("M", [32, 96, 512, 50])
@pytest.mark.parametrize("N", [1, 97, 4096, 40001])
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_sgp_kgrad_against_the_restatement(dtype, d, P, N, M):
    """hb_sgp_kgrad_f64 / _f32 against the restatement's streamed part on the same Q, R; two runs bitwise equal.  M = 32,
    96, 512 take the column-strip MFMA form, M = 50 the plain loops; N = 1 .. 40001 leave ragged steps and uneven runs
    of steps per workgroup.
    Observed on MI355X (128 cases): device error of zbar <= 1.1 % of its bound (worst: float32, N = 40001, M = 512,
    d = 3, P = 1: 7.8e-8 against 7.0e-6) and <= 4.6e-12 of the cancelling scale; of ellbar <= 0.64 % of its bound and
    <= 4.2e-11 of the scale.  Worst per M (fraction of the bound, zbar / ellbar): 32: 1.2e-4 / 3.7e-4; 96: 5.1e-3 /
    6.0e-4; 512: 1.1e-2 / 6.4e-3; 50 (plain loops): 5.6e-5 / 2.9e-4."""
    _check_kgrad(dtype, d, P, N, M, False)


@pytest.mark.parametrize("M", [96, 50])
@pytest.mark.parametrize("N", [97, 40001])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_sgp_kgrad_one_shared_lengthscale_in_three_dimensions(dtype, N, M):
    """d = 3 with ONE lengthscale (dl = 1 < d: ellbar [1] is the sum over the dimensions, the shape models.SVGP has), in
    the strip form (M = 96) and the plain form (M = 50); same bounds.
    Observed on MI355X: N = 40001, M = 96: zbar 1.1e-7 (bound 7.9e-5), ellbar 7.1e-9 (2.5e-5); M = 50: zbar 1.2e-9
    (2.1e-5), ellbar 3.5e-10 (6.9e-5); N = 97: zbar <= 1.3e-11 (2.5e-7), ellbar <= 3.3e-11 (7.7e-8)."""
    _check_kgrad(dtype, 3, 2, N, M, True)


def _check_kgrad(dtype, d, P, N, M, scalar_ell):
    dt = torch.float64 if dtype == "float64" else torch.float32
    X, Y, z, ell, r, a = _kernel_case(dtype, d, P, N, M, scalar_ell)
    assert ell.shape == ((1,) if scalar_ell or d == 1 else (d,))
    args = [dev(X, dt), dev(Y, dt)] + [dev(v, torch.float64) for v in (z, ell, r["Q"], r["R"])]
    zb, eb = H.sgp_kgrad(*args)
    zb2, eb2 = H.sgp_kgrad(*args)
    torch.cuda.synchronize()
    assert zb.dtype == torch.float64 and eb.dtype == torch.float64
    assert torch.equal(zb, zb2) and torch.equal(eb, eb2)
    zb, eb = zb.cpu().numpy(), eb.cpu().numpy()
    assert zb.shape == (M, d) and eb.shape == ell.shape
    zs = np.abs(r["z_streamed"]).max() + np.abs(r["z_kmm"]).max()
    es = np.abs(r["ell_streamed"]).max() + np.abs(r["ell_kmm"]).max()
    gz, ge = np.abs(r["z"] - a["z"]).max(), np.abs(r["lengthscales"] - a["lengthscales"]).max()
    ez, ee = np.abs(zb - r["z_streamed"]).max(), np.abs(eb - r["ell_streamed"]).max()
    print("sgp_kgrad %s N=%d M=%d d=%d P=%d: z: device %.3e, CPU gap %.3e, scale %.3e (max|grad| %.3e), bound %.3e; "
          "ell: device %.3e, CPU gap %.3e, scale %.3e, bound %.3e"
          % (dtype, N, M, d, P, ez, gz, zs, np.abs(r["z"]).max(), _bound(gz, zs), ee, ge, es, _bound(ge, es)))
    assert np.all(np.isfinite(zb)) and np.all(np.isfinite(eb))
    assert ez <= _bound(gz, zs)
    assert ee <= _bound(ge, es)


def test_sgp_kgrad_plain_form_agrees_with_the_strips_and_checks_its_operands():
    """The diagnostic switch runs an aligned shape through the plain loops: the same numbers to summation order (4 x the
    floor of the other tests, 1e-10 of the cancelling scale).
    Observed on MI355X: zbar 3.6e-10 at scale 2.5e4 (1.5e-14 of it), ellbar 6.9e-10 at scale 4.4e3 (1.6e-13)."""
    X, Y, z, ell, r, a = _kernel_case("float32", 3, 2, 4096, 96)
    args = [dev(X, torch.float32), dev(Y, torch.float32)] + [dev(v, torch.float64) for v in (z, ell, r["Q"], r["R"])]
    zf, ef = H.sgp_kgrad(*args)
    H.debug_set("sgp_kgrad_plain", 1)
    try:
        zp, ep = H.sgp_kgrad(*args)
    finally:
        H.debug_clear()
    zs = np.abs(r["z_streamed"]).max() + np.abs(r["z_kmm"]).max()
    es = np.abs(r["ell_streamed"]).max() + np.abs(r["ell_kmm"]).max()
    ez, ee = float((zf - zp).abs().max().cpu()), float((ef - ep).abs().max().cpu())
    print("strips vs plain: z %.3e (scale %.3e) ell %.3e (scale %.3e)" % (ez, zs, ee, es))
    assert ez <= 4e-10 * zs and ee <= 4e-10 * es
    with pytest.raises(TypeError):
        H.sgp_kgrad(args[0], args[1], args[2].float(), *args[3:])
    with pytest.raises(ValueError):
        H.sgp_kgrad(args[0], args[1][:100].contiguous(), *args[2:])


# ------------------------------------------------------------------------------------------------ 2. end to end
def _model(N, M, dtype, residual="diagonal", q_shape="fullrank", ell=0.9, k_var=1.3, var=0.4, seed=0):
    X, Y, Z = svgp_data(N, M, seed)
    m = SVGP(X=X, Y=Y, Z=Z, q_shape=q_shape, residual=residual, dtype=dtype)
    m.gp.kern.lengthscales = np.ones(1) * ell
    m.k_var = np.ones(1) * k_var
    m.var = np.ones(1) * var
    m.initialize()
    return m, X, Y, Z


def _stored(m, a):
    """`a` as the session stores it, in double."""
    return np.asarray(a, dtype=m._session.np_dtype).astype(np.float64)


@pytest.mark.parametrize("dtype, residual", [("float64", "diagonal"), ("float64", "neglected"), ("float32", "diagonal")])
def test_collapsed_bound_and_grad_against_the_restatement(dtype, residual):
    """SparseGP.collapsed_bound_and_grad at N = 1e5, M = 128, jitter_level 1e-5 (the project's default), in a float64
    and a float32 session: float64 arithmetic either way, so the SAME bounds hold -- 4 x the CPU gap (floored) for the
    gradients, 1e-8 relative for the value.
    Observed on MI355X (device error / CPU gap / bound): float64 'diagonal': value 3.5e-13 relative; z 3.0e-8 / 1.5e-8 /
    1.3e-6 (max|z gradient| 2.08, cancelling scale 3323); lengthscales 1.6e-7 / 1.2e-7 / 5.0e-7; noise_var 8.4e-8 /
    1.8e-7 / 5.4e-3; k_var 7.4e-9 / 1.6e-8 / 2.2e-4.  float64 'neglected': value 1.6e-15; z 3.1e-7 / 2.1e-7 / 8.3e-7;
    lengthscales 1.3e-6 / 7.2e-7 / 2.9e-6.  float32 session: value 1.8e-13; z 3.7e-8 / 2.2e-8 / 1.3e-6; lengthscales
    7.9e-9 / 8.6e-8 / 4.4e-7; noise_var 4.2e-8 / 5.3e-8 / 5.4e-3; k_var 3.1e-9 / 4.8e-9 / 2.2e-4."""
    N, M = 100000, 128
    assert hb.settings.numerics.jitter_level == JITTER
    m, X, Y, Z = _model(N, M, dtype, residual)
    s2, k = 0.09, 1.0
    gp = object.__getattribute__(m, "gp")
    val, g = gp.collapsed_bound_and_grad(object.__getattribute__(m, "X"), object.__getattribute__(m, "Y"), s2, k,
                                         residual=residual)
    assert isinstance(val, float) and g["z"].dtype == np.float64 and g["z"].shape == (M, 1)
    assert g["lengthscales"].shape == (1,) and isinstance(g["noise_var"], float) and isinstance(g["k_var"], float)
    Xs, Ys, zs_, ells = _stored(m, X), _stored(m, Y), _stored(m, Z), _stored(m, m.gp.kern.lengthscales.value).reshape(-1)
    r = C.bound_and_grad(Xs, Ys, zs_, ells, JITTER, s2, k, residual)
    a = C.bound_autograd(Xs, Ys, zs_, ells, JITTER, s2, k, residual)
    zsc = np.abs(r["z_streamed"]).max() + np.abs(r["z_kmm"]).max()
    esc = np.abs(r["ell_streamed"]).max() + np.abs(r["ell_kmm"]).max()
    rows = [("z", np.abs(g["z"] - r["z"]).max(), np.abs(r["z"] - a["z"]).max(), zsc, np.abs(r["z"]).max()),
            ("lengthscales", np.abs(g["lengthscales"] - r["lengthscales"]).max(),
             np.abs(r["lengthscales"] - a["lengthscales"]).max(), esc, np.abs(r["lengthscales"]).max()),
            ("noise_var", abs(g["noise_var"] - r["noise_var"]), abs(r["noise_var"] - a["noise_var"]), r["noise_var_abs"],
             abs(r["noise_var"])),
            ("k_var", abs(g["k_var"] - r["k_var"]), abs(r["k_var"] - a["k_var"]), r["k_var_abs"], abs(r["k_var"]))]
    print("collapsed_bound_and_grad %s %s: value %.9f ref %.9f (rel %.2e)" % (dtype, residual, val, r["value"],
                                                                           abs(val / r["value"] - 1)))
    for name, err, gap, scale, size in rows:
        print("   %-12s device %.3e, CPU gap %.3e, cancelling scale %.3e (max|grad| %.3e), bound %.3e"
              % (name, err, gap, scale, size, _bound(gap, scale)))
    assert abs(val - r["value"]) <= 1e-8 * abs(r["value"])
    for name, err, gap, scale, size in rows:
        assert err <= _bound(gap, scale), name
    if dtype == "float64":
        assert abs(val - m.gp.collapsed_bound(X, Y, s2, k, residual=residual)) <= 1e-8 * abs(val)


def test_collapsed_bound_and_grad_refuses_what_it_does_not_cover():
    X, Y, Z = svgp_data(200, 32, 0)
    m, _, _, _ = _model(200, 32, "float64")
    with pytest.raises(NotImplementedError, match="fullrank"):
        m.gp.collapsed_bound_and_grad(X, Y, 0.4, residual="fullrank")
    with pytest.raises(ValueError):
        m.gp.collapsed_bound_and_grad(X, Y, -1.0)

    class Other(hb.model.Model):
        def setUp(self, Z, kern):
            self.gp = hb.gp.SparseGP(kern=kern, z=Z)

    with pytest.raises(NotImplementedError, match="UnitRBF"):
        Other(Z=Z, kern=hb.gp.kernels.UnitMatern52(np.ones(1)), dtype="float64").gp.collapsed_bound_and_grad(X, Y, 0.4)
    with pytest.raises(NotImplementedError, match="one expert"):
        Other(Z=np.stack([Z, Z]), kern=hb.gp.kernels.UnitRBF(np.ones((2, 1))),
              dtype="float64").gp.collapsed_bound_and_grad(X, Y, 0.4)


# ------------------------------------------------------------------------------------------------ 3. model level
def _raw_of(m):
    return {n: m._session.read_raw(v).copy() for n, v in m._hyper_variables().items()}


def test_svgp_gradient_against_central_differences_of_collapsed_bound():
    """SVGP.collapsed_bound_and_grad() (raw parameters, through the transforms) in a float64 model against directional
    central differences of the EXISTING SVGP.collapsed_bound() along a random raw-space direction per parameter group
    (z alone included: the var gradient is about 1e5 times the z gradient).  Bound: 4 x the error the same difference
    makes on the CPU restatement at the same h.
    Observed on MI355X (h = 0.01; |analytic - difference| on the device / bound): z 1.09e-7 / 4.34e-7 (directional
    derivative -1.9e-3); lengthscales 2.23e-4 / 8.91e-4 (-19.5); k_var 4.75e-5 / 1.90e-4 (3.65); var 1.565e-2 / 6.26e-2
    (1020.9): the device makes the CPU restatement's truncation error to four digits."""
    N, M, h = 4096, 32, 1e-2
    m, X, Y, Z = _model(N, M, "float64", ell=1.2, k_var=0.8, var=0.2)
    T = hb.transforms.positive
    val, g = m.collapsed_bound_and_grad()
    raw0 = _raw_of(m)
    assert set(g) == {"z", "lengthscales", "k_var", "var"} and all(g[n].shape == raw0[n].shape for n in g)
    assert abs(val - m.collapsed_bound()) <= 1e-8 * abs(val)
    hv = m._hyper_variables()

    def f_dev(name, x):
        m._session.write_raw(hv[name], x)
        try:
            return m.collapsed_bound()
        finally:
            m._session.write_raw(hv[name], raw0[name])

    def f_ref(name, x):
        p = dict(raw0)
        p[name] = x
        ell, kv, s2 = (T.forward(p[n]).reshape(-1) for n in ("lengthscales", "k_var", "var"))
        st = R.stats(X, Y, p["z"], ell, JITTER)
        return R.collapsed_bound(*st, N, float(s2[0]), float(kv[0]))

    ell0, kv0, s20 = (T.forward(raw0[n]).reshape(-1) for n in ("lengthscales", "k_var", "var"))
    r = C.bound_and_grad(X, Y, raw0["z"], ell0, JITTER, float(s20[0]), float(kv0[0]))
    g_ref = dict(z=r["z"], lengthscales=r["lengthscales"] * T.dforward(raw0["lengthscales"]),
                 k_var=r["k_var"] * T.dforward(raw0["k_var"]), var=r["noise_var"] * T.dforward(raw0["var"]))
    rng = np.random.RandomState(3)
    rows = []
    for name in ("z", "lengthscales", "k_var", "var"):
        u = np.asarray(rng.standard_normal(raw0[name].shape))
        u = u / np.sqrt((u * u).sum())
        fd_dev = C.directional_fd(lambda x: f_dev(name, x), raw0[name], u, h)
        fd_ref = C.directional_fd(lambda x: f_ref(name, x), raw0[name], u, h)
        an_dev, an_ref = float((g[name] * u).sum()), float((np.reshape(g_ref[name], u.shape) * u).sum())
        rows.append((name, an_dev, fd_dev, abs(an_dev - fd_dev), 4.0 * abs(an_ref - fd_ref)))
        print("%-12s analytic (device) %.9e, central difference of collapsed_bound() %.9e (h = %g): |gap| %.3e; the same "
              "on the CPU restatement: analytic %.9e difference %.9e; bound %.3e"
              % (name, an_dev, fd_dev, h, abs(an_dev - fd_dev), an_ref, fd_ref, rows[-1][4]))
    for name, _, _, err, bound in rows:
        assert err <= bound, name


# ------------------------------------------------------------------------------------------------ 4. behaviour
def test_fit_hyper_climbs_the_bound_and_leaves_the_optimal_q():
    """From deliberately wrong hyper-parameters (ell x 3, var x 10) fit_hyper's last bound exceeds its first and the
    collapsed_bound() of the starting point evaluated independently; afterwards fit_q() has been applied: the existing
    Monte-Carlo ELBO over all rows equals the bound within 4 standard errors of 64 evaluations (the tolerance
    test_optimal_q_gpu.py uses for the same comparison).
    Observed on MI355X: bound -3822.68 -> -910.45 in 60 steps (ell 3.0 -> 2.158, k_var 1.0 -> 1.708, var 0.9 -> 0.0925,
    max|dz| 0.95); Monte-Carlo ELBO afterwards -910.4525 +- 0.0791; float32 model, 10 steps, z fixed: -3822.68 -> -3158.72."""
    np.random.seed(0)
    m, X, Y, Z = _model(4096, 32, "float64", ell=3.0, k_var=1.0, var=0.9)
    start = m.collapsed_bound()
    z0 = m.gp.z.value.copy()
    trace = m.fit_hyper(steps=60, lr=0.05)
    end = m.collapsed_bound()
    print("fit_hyper: start %.4f (collapsed_bound() %.4f) -> %.4f (collapsed_bound() %.4f); ell %.4f k_var %.4f var %.4f; "
          "max|dz| %.3e" % (trace[0], start, trace[-1], end, m.gp.kern.lengthscales.value[0], m.k_var.value[0], m.var.value[0],
                          np.abs(m.gp.z.value - z0).max()))
    assert trace.shape == (61,) and np.all(np.isfinite(trace))
    assert abs(trace[0] - start) <= 1e-8 * abs(start) and abs(trace[-1] - end) <= 1e-8 * abs(end)
    assert trace[-1] > trace[0] and trace[-1] > start
    assert np.abs(m.gp.z.value - z0).max() > 0
    opt = m.ELBO()
    opt.compile(optimizer=tf.train.AdamOptimizer(1e-2))
    vals = np.array([opt.run() for _ in range(64)])
    mean, se = vals.mean(), vals.std(ddof=1) / 8.0
    print("   Monte-Carlo ELBO over all rows after fit_hyper: %.4f +- %.4f" % (mean, se))
    assert se > 0 and abs(end - mean) <= 4.0 * se
    # train_z=False leaves z alone
    m2, _, _, _ = _model(4096, 32, "float32", ell=3.0, k_var=1.0, var=0.9)
    z0 = m2.gp.z.value.copy()
    t2 = m2.fit_hyper(steps=10, lr=0.05, train_z=False)
    print("   float32 model, train_z=False: %.4f -> %.4f" % (t2[0], t2[-1]))
    assert np.array_equal(m2.gp.z.value, z0) and t2[-1] > t2[0]


def test_fit_hyper_restores_the_parameters_when_a_factorisation_fails(monkeypatch):
    """A factorisation that fails AFTER two good steps: the raw parameters are those of the last successful evaluation,
    not the initial ones and not the stepped ones.  And one that fails at the start leaves everything as it was."""
    m, X, Y, Z = _model(2000, 32, "float64", ell=3.0, k_var=1.0, var=0.9)
    real = SVGP.collapsed_bound_and_grad
    seen = []

    def failing_third(self):
        if len(seen) == 2:
            seen.append(_raw_of(self))
            raise G.CholeskyError("injected: Lambda is not positive definite")
        out = real(self)
        seen.append(_raw_of(self))
        return out

    monkeypatch.setattr(SVGP, "collapsed_bound_and_grad", failing_third)
    with pytest.raises(G.CholeskyError, match="injected"):
        m.fit_hyper(steps=5, lr=0.05)
    after = _raw_of(m)
    assert len(seen) == 3
    for n in after:
        assert np.array_equal(after[n], seen[1][n]), n                      # the last successful evaluation
        assert not np.array_equal(seen[2][n], seen[1][n]), n                # the failing step had moved them
        assert not np.array_equal(seen[0][n], seen[1][n]), n
    # a real failure, at the first evaluation
    cfg = hb.settings.get_settings()
    cfg.numerics.jitter_level = 0.0
    with hb.settings.temp_settings(cfg):
        m = SVGP(X=X, Y=Y, Z=np.zeros((32, 1)), q_shape="diagonal", dtype="float64")
        m.initialize()
        before = _raw_of(m)
        with pytest.raises(G.CholeskyError):
            m.fit_hyper(steps=3, lr=0.1)
        after = _raw_of(m)
    assert all(np.array_equal(before[n], after[n]) for n in before)
