"""Hyper-parameter gradient of the multi-class ELBO at fixed q(u_c) on the GPU: hb_lik_softmax_grad,
SparseGP.elbo_and_grad_multi, SVGPMulticlass.elbo_and_grad and SVGPMulticlass.fit_hyper against the numpy restatement
tests/softmax_grad_ref.py (itself pinned on the host by tests/test_softmax_grad_cpu.py against autograd of the node sum).

Bounds.  The weights: |w - w_ref| <= 1e-12 a + 1e-300 with a = mean_s |d eps| / sqrt(v) the scale of w's summands (a
float64 numpy evaluation of these inputs stays within 9e-15 a of an 80-bit one; a naive 1 - p misses by 5e-3; 1e-12 leaves
the two orders of magnitude test_softmax_gpu.py grants lam), |r - g_ref| <= 1e-12 (1 + |mu|), and on v = 0 columns w is
p (1 - p) at mu within 1e-11 x 0.25 + 1e-16.  lsum: the BITS of hb_lik_softmax_sites.  Gradients: test_elbo_grad_gpu.py's
4 x max(gap, 1e-10 x scale), gap = the difference of the two float64 CPU evaluations (restatement against
torch.autograd) ON THE SAME INPUTS, scale = max|streamed part| + max|K(z, z) part| of the class sums.  Model level: 4 x the
error the same central difference makes on the CPU restatement at the same h.  Every figure is printed before it is
asserted."""
import functools

import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd import _lib
from henbun_amd import graph as G
from henbun_amd import hip_ops as H
from henbun_amd.models import SVGPMulticlass

import collapsed_grad_ref as CG
import softmax_grad_ref as MG
import softmax_ref as F
from test_softmax_gpu import MS, VS, _site_inputs

pytestmark = pytest.mark.gpu

JITTER = 1e-5


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def _bound(gap, scale):
    return 4.0 * max(gap, 1e-10 * scale)


def _scales(r):
    return (np.abs(r["z_streamed"]).max() + np.abs(r["z_kmm"]).max(),
            np.abs(r["ell_streamed"]).max() + np.abs(r["ell_kmm"]).max())


# ------------------------------------------------------------------------------------------------ 1. the weights
_GRAD_CASES = [(C, N, S) for C in (2, 3, 10, 33, 64) for N in (1, 77, 1000) for S in (1, 128)]
_GRAD_CASES += [(64, 5000, 128), (3, 70001, 16)]      # a workgroup walks its loop over point tiles more than once


@pytest.mark.parametrize("C, N, S", _GRAD_CASES)
def test_softmax_grad_against_the_restatement(C, N, S):
    """hb_lik_softmax_grad, float64 and float32 storage (the outputs are double either way: the SAME bounds, against the
    restatement on the rounded inputs), on test_softmax_gpu's inputs: exact v = 0 columns, |mu| up to 40, groups of 2 .. 64
    lanes per point, a partly idle last wave, two sizes with more than one trip through the point loop.  lsum has the
    bits of hb_lik_softmax_sites; two calls return the same bits; padded output rows (ldo > N) hold the same bits.
    Observed on MI355X (32 cases x 2 storage types): w <= 1.6 % of its bound (1.6e-14 a; worst C = 64, N = 1000, S = 1), r
    within its bound, the v <= 0 entries and the v = 0 columns within theirs; 0 differing bits everywhere."""
    y, mean, var = _site_inputs(C, N, seed=100 * C + N + S)
    nodes = np.random.RandomState(S + C).randn(S, C)
    nd = dev(nodes, torch.float64)
    for dtype in ("float64", "float32"):
        dt, npdt = (torch.float64, np.float64) if dtype == "float64" else (torch.float32, np.float32)
        yq, mq, vq = (a.astype(npdt) for a in (y, mean, var))
        yd, md, vd = dev(yq, dt), dev(mq, dt), dev(vq, dt)
        w, r, lsum = H.lik_softmax_grad(yd, md, vd, nd, mscale=MS, vscale=VS)
        w2, r2, lsum2 = H.lik_softmax_grad(yd, md, vd, nd, mscale=MS, vscale=VS)
        _, _, lsites = H.lik_softmax_sites(yd, md, vd, nd, mscale=MS, vscale=VS)
        pad = torch.full((2, C, N + 5), 7.0, dtype=torch.float64, device="cuda")
        H.lik_softmax_grad(yd, md, vd, nd, mscale=MS, vscale=VS, out=(pad[0, :, :N], pad[1, :, :N]))
        torch.cuda.synchronize()
        assert w.dtype == torch.float64 and r.dtype == torch.float64 and tuple(w.shape) == (C, N)
        assert torch.equal(w, w2) and torch.equal(r, r2) and torch.equal(lsum, lsum2)
        assert torch.equal(lsum, lsites)
        assert torch.equal(pad[0, :, :N], w) and torch.equal(pad[1, :, :N], r) and bool((pad[:, :, N:] == 7.0).all())
        w, r = w.cpu().numpy(), r.cpu().numpy()
        mu, v = MS * mq.astype(np.float64), VS * vq.astype(np.float64)
        _, rw, rg, ra, rlam = MG.weights(yq, mu, v, nodes)
        pos = v > 0.0
        assert np.all(np.isfinite(w)) and np.all(np.isfinite(r))
        e_w = (np.abs(w - rw) / (1e-12 * ra + 1e-300))[pos].max() if pos.any() else 0.0
        e_r = (np.abs(r - rg) / (1.0 + np.abs(mu))).max()
        # v_jc <= 0: w is mean_s p (1 - p); on a column whose every class has v = 0 that is p (1 - p) at mu
        zero = v.sum(0) == 0.0
        p0 = np.exp(F.log_softmax(mu))
        e_l = np.abs(w - rlam)[~pos].max() if (~pos).any() else 0.0
        e_0 = np.abs(w - p0 * (1.0 - p0))[:, zero].max() if zero.any() else 0.0
        print("softmax_grad C=%d N=%d S=%d %s: w %.3e of its bound (min w %.3e, %.1f %% negative), r %.2e, v <= 0: %.2e, "
              "v = 0 columns: %.2e" % (C, N, S, dtype, e_w, w.min(), 100.0 * (w < 0).mean(), e_r, e_l, e_0))
        assert e_w <= 1.0
        assert e_r <= 1e-12
        assert e_l <= 1e-11 * 0.25 + 1e-16 and e_0 <= 1e-11 * 0.25 + 1e-16
        if S > 1 and N >= 77:
            assert (w[pos] < 0).any()                                   # signed, unlike lam


def test_softmax_grad_refuses_bad_arguments_before_any_launch():
    """C outside 2 .. 64, S outside 1 .. 1024, a negative vscale or N, rows closer than N; N = 0 writes lsum = 0.  The
    wrapper refuses outputs that are not float64 [C, N] with one row stride."""
    C, N, S = 3, 8, 4
    f64 = dict(dtype=torch.float64, device="cuda")
    y, mean, var = (torch.zeros(s, **f64) for s in ((N,), (C, N), (C, N)))
    nodes, out, one = torch.zeros((S, C), **f64), torch.empty((C, N), **f64), torch.full((1,), 7.0, **f64)
    ws = H.workspace(torch.float64, y.device, 1024)
    call, p = _lib.lib().call, H._p

    def grad(n=N, c=C, s=S, vs=1.0, ldo=N):
        call("hb_lik_softmax_grad_f64", p(y), p(mean), p(var), 1.0, vs, p(nodes), s, p(out), p(out), ldo, p(one), n, c, p(ws),
             H.stream())

    for kw in (dict(c=1), dict(c=65), dict(s=0), dict(s=1025), dict(vs=-1.0), dict(n=-1), dict(ldo=N - 1)):
        with pytest.raises(_lib.HipBackendError):
            grad(**kw)
    assert float(one.cpu()[0]) == 7.0
    grad(n=0)
    assert float(one.cpu()[0]) == 0.0
    with pytest.raises(ValueError, match="out ="):
        H.lik_softmax_grad(y, mean, var, nodes, out=(out, out.float()))
    with pytest.raises(ValueError, match="out ="):
        H.lik_softmax_grad(y, mean, var, nodes, out=(out, torch.empty((C, N + 1), **f64)[:, :N]))
    with pytest.raises(ValueError):
        H.lik_softmax_grad(y, mean, var, nodes.float())


# ------------------------------------------------------------------------------------------------ 2. end to end
K_VAR = 4.0


@functools.lru_cache(maxsize=2)
def _ring(N, M, seed):
    return F.ring(3, N, M, 128, seed)


def _model(N, M, dtype, residual="diagonal", seed=0, ell=1.0, k_var=K_VAR):
    X, y, Z, eps = _ring(N, M, seed)
    m = SVGPMulticlass(X=X, y=y, Z=Z, num_classes=3, nodes=eps, residual=residual, dtype=dtype)
    m.gp.kern.lengthscales = np.ones(1) * ell
    m.k_var = np.ones(1) * k_var
    m.initialize()
    return m, X, y, Z, eps


def _stored(m, a):
    """`a` as the session stores it, in double."""
    return np.asarray(a, dtype=m._session.np_dtype).astype(np.float64)


@pytest.mark.parametrize("residual", ["diagonal", "neglected"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_elbo_and_grad_multi_against_the_restatement(dtype, residual):
    """SparseGP.elbo_and_grad_multi on ring(3, 2000, 32, 128), k_var = 4, jitter_level 1e-5, in a float64 and a float32
    session (float64 arithmetic either way: the SAME bounds), at the q of 3 natural-gradient steps from the prior -- the
    residual is asserted above 1e-6, so the partial gradient is tested away from the fixed point.  Value: 1e-8 relative;
    gradients: 4 x the CPU gap against autograd of the node sum (floored); a second call returns the same bits.
    Observed on MI355X (device error / CPU gap / bound; the floor decides every bound): value <= 2.0e-15 relative; z
    3.9e-13 .. 3.2e-12 / 1.3e-12 .. 2.2e-12 / 6.0e-9 .. 7.7e-9 (max|z gradient| 0.92 .. 4.0, cancelling scale 15 .. 19);
    lengthscale 2.6e-13 .. 2.1e-11 / 2.8e-14 .. 2.5e-11 / 2.2e-8; k_var <= 4.4e-14 / 5.3e-14 / 1.7e-9; the natural-gradient
    residual at the q used is 8.8 (three half steps from the prior)."""
    N, M = 2000, 32
    assert hb.settings.numerics.jitter_level == JITTER
    m, X, y, Z, eps = _model(N, M, dtype)
    gp, lik = object.__getattribute__(m, "gp"), object.__getattribute__(m, "likelihood")
    Xm, Ym = object.__getattribute__(m, "X"), object.__getattribute__(m, "Y")
    qm, qS, info = gp.natgrad_q(Xm, Ym, lik, k_var=K_VAR, residual=residual, steps=3, rho=0.5, tol=0.0)
    assert info["residual"][-1] > 1e-6                                   # not at the fixed point
    val, g = gp.elbo_and_grad_multi(Xm, Ym, lik, (qm, qS), k_var=K_VAR, residual=residual)
    assert isinstance(val, float) and g["z"].dtype == np.float64 and g["z"].shape == (M, 2)
    assert g["lengthscales"].shape == (1,) and isinstance(g["k_var"], float) and set(g) == {"z", "lengthscales", "k_var"}
    Xs, zs_, ells = _stored(m, X), _stored(m, Z), _stored(m, m.gp.kern.lengthscales.value).reshape(-1)
    r = MG.elbo_and_grad(Xs, y, zs_, ells, JITTER, eps, qm, qS, K_VAR, residual)
    a = MG.elbo_autograd(Xs, y, zs_, ells, JITTER, eps, qm, qS, K_VAR, residual)
    zs, es = _scales(r)
    rows = [("z", np.abs(g["z"] - r["z"]).max(), np.abs(r["z"] - a["z"]).max(), zs, np.abs(r["z"]).max()),
            ("lengthscales", np.abs(g["lengthscales"] - r["lengthscales"]).max(),
             np.abs(r["lengthscales"] - a["lengthscales"]).max(), es, np.abs(r["lengthscales"]).max()),
            ("k_var", abs(g["k_var"] - r["k_var"]), abs(r["k_var"] - a["k_var"]), r["k_var_abs"], abs(r["k_var"]))]
    print("elbo_and_grad_multi %s %s: value %.9f ref %.9f (rel %.2e); natgrad residual %.2e; %.1f %% of w negative"
          % (dtype, residual, val, r["value"], abs(val / r["value"] - 1), info["residual"][-1], 100.0 * (r["w"] < 0).mean()))
    for name, err, gap, scale, size in rows:
        print("   %-12s device %.3e, CPU gap %.3e, cancelling scale %.3e (max|grad| %.3e), bound %.3e"
              % (name, err, gap, scale, size, _bound(gap, scale)))
    assert abs(val - r["value"]) <= 1e-8 * abs(r["value"])
    for name, err, gap, scale, size in rows:
        assert err <= _bound(gap, scale), name
    val2, g2 = gp.elbo_and_grad_multi(Xm, Ym, lik, (qm, qS), k_var=K_VAR, residual=residual)
    assert val2 == val and all(np.array_equal(g[n], g2[n]) for n in g)


# ------------------------------------------------------------------------------------------------ 3. model level
def _raw_of(m):
    return {n: m._session.read_raw(v).copy() for n, v in m._hyper_variables().items()}


def test_svgp_multiclass_gradient_against_central_differences_of_its_own_value():
    """SVGPMulticlass.elbo_and_grad() (raw parameters, through the transforms) in a float64 model on ring(3, 300, 16, 128)
    at the q of 3 natural-gradient steps, against central differences of the device's own VALUE at h = 1e-2 in a handful
    of raw entries of z, the lengthscale and k_var.  Bound: 4 x the error the same difference makes on the CPU
    restatement (the convention of test_svgplik_gradient_against_central_differences_of_its_own_value).
    Observed on MI355X: value -25.195663910, equal to the restatement's to 1.1e-16; |analytic - difference| on the device /
    bound: z 5.4e-6 .. 4.1e-4 / 2.1e-5 .. 1.7e-3; lengthscale 8.4e-4 / 3.4e-3 (derivative 4.874); k_var 9.8e-6 / 3.9e-5
    (1.042): the device makes the CPU restatement's truncation error to all digits printed."""
    N, M, h = 300, 16, 1e-2
    m, X, y, Z, eps = _model(N, M, "float64", seed=3, ell=1.2)
    m.reset_q()
    m.fit_q(steps=3, tol=0.0)
    T = hb.transforms.positive
    val, g = m.elbo_and_grad()
    raw0 = _raw_of(m)
    assert set(g) == {"z", "lengthscales", "k_var"} and all(g[n].shape == raw0[n].shape for n in g)
    qm, qS = m._current_blocks()
    hv = m._hyper_variables()
    res = m._likelihood_residual()
    assert res == "neglected"

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
        return MG.value(X, y, z_, ell_, JITTER, eps, qm, qS, k_, res)

    z0, ell0, k0 = cons(raw0)
    r = MG.elbo_and_grad(X, y, z0, ell0, JITTER, eps, qm, qS, k0, res)
    print("SVGPMulticlass.elbo_and_grad: value %.9f, restatement %.9f (rel %.2e)" % (val, r["value"], abs(val / r["value"] - 1)))
    assert abs(val - r["value"]) <= 1e-8 * abs(r["value"])
    g_ref = dict(z=r["z"], lengthscales=r["lengthscales"] * T.dforward(raw0["lengthscales"]),
                 k_var=r["k_var"] * T.dforward(raw0["k_var"]))
    entries = [("z", (0, 0)), ("z", (5, 1)), ("z", (11, 0)), ("z", (15, 1)), ("lengthscales", (0,)), ("k_var", (0,))]
    rows = []
    for name, idx in entries:
        u = np.zeros(raw0[name].shape)
        u[idx] = 1.0
        fd_dev = CG.directional_fd(lambda x: f_dev(name, x), raw0[name], u, h)
        fd_ref = CG.directional_fd(lambda x: f_ref(name, x), raw0[name], u, h)
        an_dev, an_ref = float(g[name][idx]), float(np.reshape(g_ref[name], u.shape)[idx])
        rows.append(("%s%s" % (name, list(idx)), abs(an_dev - fd_dev), 4.0 * abs(an_ref - fd_ref)))
        print("%-16s analytic (device) %.9e, central difference of the device's value %.9e (h = %g): |gap| %.3e; the same "
              "on the CPU restatement: analytic %.9e difference %.9e; bound %.3e"
              % (rows[-1][0], an_dev, fd_dev, h, abs(an_dev - fd_dev), an_ref, fd_ref, rows[-1][2]))
    for name, err, bound in rows:
        assert err <= bound, name


# ------------------------------------------------------------------------------------------------ 4. behaviour
def test_fit_hyper_climbs_the_elbo_and_leaves_the_fitted_q():
    """ring(3, 300, 16, 128, seed 3), float64, lengthscale and k_var started at 1, q(u) at the prior: fit_hyper(30, lr =
    0.05) returns 31 finite entries whose last exceeds the first and equals the ELBO a fit_q() run afterwards starts from,
    to 1e-8 relative; z moved; train_z=False leaves z bit-identical.
    Observed on MI355X: -45.538888 -> -25.140432 in 30 steps, every step up (smallest increase 0.22); the fit_q() afterwards
    starts 8.9e-16 relative from the trace's last entry; ell 1 -> 1.842, k_var 1 -> 2.030, max|dz| 1.23; train_z=False, 3
    steps: -47.084589 -> -41.096315."""
    m, X, y, Z, eps = _model(300, 16, "float64", seed=3, ell=1.0, k_var=1.0)
    m.reset_q()
    z0 = m.gp.z.value.copy()
    trace = m.fit_hyper(30, lr=0.05)
    _, _, info = m.fit_q()
    print("fit_hyper: %.6f -> %.6f in 30 steps, smallest increase %.3e (fit_q afterwards starts at %.6f, rel %.2e); ell -> "
          "%.4f, k_var -> %.4f, max|dz| %.3e"
          % (trace[0], trace[-1], np.diff(trace).min(), info["elbo"][0], abs(trace[-1] / info["elbo"][0] - 1),
             m.gp.kern.lengthscales.value[0], m.k_var.value[0], np.abs(m.gp.z.value - z0).max()))
    assert trace.shape == (31,) and np.all(np.isfinite(trace))
    assert trace[-1] > trace[0]
    assert abs(trace[-1] - info["elbo"][0]) <= 1e-8 * abs(info["elbo"][0])
    assert np.abs(m.gp.z.value - z0).max() > 0
    m2, _, _, _, _ = _model(300, 16, "float64", seed=3, ell=1.0, k_var=1.0)
    m2.reset_q()
    z0 = m2.gp.z.value.copy()
    t2 = m2.fit_hyper(3, lr=0.05, train_z=False, q_steps=2)
    print("   train_z=False: %.6f -> %.6f" % (t2[0], t2[-1]))
    assert t2.shape == (4,) and np.all(np.isfinite(t2)) and np.array_equal(m2.gp.z.value, z0)


def test_fit_hyper_restores_the_parameters_when_a_factorisation_fails(monkeypatch):
    """A factorisation that fails on the THIRD evaluation: the raw parameters are those of the last successful
    evaluation, not the initial ones and not the stepped ones."""
    m, X, y, Z, eps = _model(300, 16, "float64", seed=3, ell=1.0, k_var=1.0)
    m.reset_q()
    real = SVGPMulticlass.elbo_and_grad
    seen = []

    def failing_third(self):
        if len(seen) == 2:
            seen.append(_raw_of(self))
            raise G.CholeskyError("injected: K(z, z) is not positive definite")
        out = real(self)
        seen.append(_raw_of(self))
        return out

    monkeypatch.setattr(SVGPMulticlass, "elbo_and_grad", failing_third)
    with pytest.raises(G.CholeskyError, match="injected"):
        m.fit_hyper(5, lr=0.05, q_steps=2)
    after = _raw_of(m)
    assert len(seen) == 3
    for n in after:
        assert np.array_equal(after[n], seen[1][n]), n                      # the last successful evaluation
        assert not np.array_equal(seen[2][n], seen[1][n]), n                # the failing step had moved them
        assert not np.array_equal(seen[0][n], seen[1][n]), n
