"""models.DeepKernelSVGP on the GPU: bound_and_grad() against directional central differences of its own
collapsed_bound(), fit() in a float64 and a float32 session, the predictive's shapes.

Bound of the gradient test: 4 x the error the same central difference makes on the CPU restatement
(kgrad_x_ref.dkl_bound: a float64 torch MLP feeding optimal_q_ref's bound, its gradient from torch.autograd) at the same
h -- the rule of test_svgp_gradient_against_central_differences_of_collapsed_bound.  Every figure is printed before it
is asserted."""
import numpy as np
import pytest

import henbun_amd as hb
from henbun_amd.models import DeepKernelSVGP

import kgrad_x_ref as KX

pytestmark = pytest.mark.gpu

JITTER = 1e-5
T = hb.transforms.positive


def _data(N, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.uniform(-2, 2, (N, 2))
    Y = np.sin(2 * X[:, :1]) * np.cos(X[:, 1:]) + 0.1 * rng.randn(N, 1)
    return X, Y


def _model(N, dtype, hidden=(16,), M=32, seed=0):
    np.random.seed(seed)
    X, Y = _data(N, seed)
    m = DeepKernelSVGP(X=X, Y=Y, M=M, hidden=hidden, feature_dim=2, activation="tanh", dtype=dtype)
    m.gp.kern.lengthscales = np.ones(2) * 0.2
    m.k_var = np.ones(1) * 0.8
    m.var = np.ones(1) * 0.2
    m.initialize()
    return m, X, Y


def _raw_of(m):
    return {n: m._session.read_raw(v).copy() for n, v in m._hyper_variables().items()}


def test_gradient_against_central_differences_of_collapsed_bound():
    """Float64 session, N = 512, D_in = 2, net [2, 16, 2] tanh, M = 32: one random raw-space direction per parameter
    group, the network's weights and biases as ONE group.
    Observed on MI355X (|analytic - difference| on the device / bound): value -230.696227826 on device and CPU; z 1.542 /
    6.169 (directional derivative 13.35); lengthscales 1.681e-3 / 6.726e-3 (-10.67); k_var 3.041e-5 / 1.216e-4 (-5.61);
    var 1.971e-3 / 7.885e-3 (107.9); net 6.855e-2 / 2.742e-1 (-5.08): the device makes the CPU restatement's truncation
    error to four digits."""
    N, M, h = 512, 32, 1e-2
    assert hb.settings.numerics.jitter_level == JITTER
    m, X, Y = _model(N, "float64")
    val, g = m.bound_and_grad()
    raw0 = _raw_of(m)
    hv = m._hyper_variables()
    nets = [n for n in raw0 if n.startswith("net")]
    assert nets == ["net0.w", "net0.b", "net1.w", "net1.b"]
    assert set(g) == set(raw0) and all(g[n].shape == raw0[n].shape and g[n].dtype == np.float64 for n in g)
    assert abs(val - m.collapsed_bound()) <= 1e-8 * abs(val)
    assert m.features().shape == (N, 2) and m.features(X[:5]).shape == (5, 2)

    def f_dev(p):
        for n in p:
            m._session.write_raw(hv[n], p[n])
        try:
            return m.collapsed_bound()
        finally:
            for n in p:
                m._session.write_raw(hv[n], raw0[n])

    def cons(p):
        ws = [(p["net%d.w" % i], p["net%d.b" % i]) for i in range(2)]
        return ws, p["z"], T.forward(p["lengthscales"]).reshape(-1), float(T.forward(p["var"]).reshape(-1)[0]), \
            float(T.forward(p["k_var"]).reshape(-1)[0])

    def f_ref(p):
        q = dict(raw0)
        q.update(p)
        ws, z, ell, s2, k = cons(q)
        return KX.dkl_bound(X, Y, ws, z, ell, JITTER, s2, k)

    ws, z, ell, s2, k = cons(raw0)
    vref, gr = KX.dkl_bound(X, Y, ws, z, ell, JITTER, s2, k, grad=True)
    g_ref = dict(z=gr["z"], lengthscales=gr["lengthscales"] * T.dforward(raw0["lengthscales"]).reshape(-1),
                 k_var=gr["k_var"] * T.dforward(raw0["k_var"]), var=gr["noise_var"] * T.dforward(raw0["var"]))
    for i, (dw, db) in enumerate(gr["net"]):
        g_ref["net%d.w" % i], g_ref["net%d.b" % i] = dw, db
    print("value: device %.9f, CPU restatement %.9f" % (val, vref))
    assert abs(val - vref) <= 1e-8 * abs(vref)
    rng = np.random.RandomState(3)
    rows = []
    for group in (["z"], ["lengthscales"], ["k_var"], ["var"], nets):
        u = {n: np.asarray(rng.standard_normal(raw0[n].shape)) for n in group}
        norm = np.sqrt(sum((v * v).sum() for v in u.values()))
        u = {n: v / norm for n, v in u.items()}
        step = lambda s: {n: raw0[n] + s * h * u[n] for n in group}
        fd_dev = (f_dev(step(1.0)) - f_dev(step(-1.0))) / (2 * h)
        fd_ref = (f_ref(step(1.0)) - f_ref(step(-1.0))) / (2 * h)
        an_dev = float(sum((g[n] * u[n]).sum() for n in group))
        an_ref = float(sum((np.reshape(g_ref[n], u[n].shape) * u[n]).sum() for n in group))
        name = group[0] if len(group) == 1 else "net"
        rows.append((name, abs(an_dev - fd_dev), 4.0 * abs(an_ref - fd_ref)))
        print("%-12s analytic (device) %.9e, central difference of collapsed_bound() %.9e (h = %g): |gap| %.3e; the same on "
              "the CPU restatement: analytic %.9e difference %.9e; bound %.3e"
              % (name, an_dev, fd_dev, h, rows[-1][1], an_ref, fd_ref, rows[-1][2]))
    for name, err, bound in rows:
        assert err <= bound, name


def test_fit_climbs_the_bound_and_predicts():
    """fit(30, lr=0.05) from a random network: the trace is finite and climbs, its ends are collapsed_bound() before and
    after, predict_y returns [P, n] arrays with positive variances above the noise.  (The Monte-Carlo check of fit_q is
    SVGP's.)
    Observed on MI355X: -462.27 -> 211.47 (ell 0.2 -> 0.33 / 0.37, k_var 0.8 -> 0.60, var 0.2 -> 0.077)."""
    m, X, Y = _model(1024, "float64")
    start = m.collapsed_bound()
    w0 = m._session.read_raw(m._hyper_variables()["net0.w"]).copy()
    trace = m.fit(30, lr=0.05)
    end = m.collapsed_bound()
    print("fit: %.4f (collapsed_bound() %.4f) -> %.4f (collapsed_bound() %.4f); ell %s k_var %.4f var %.4f"
          % (trace[0], start, trace[-1], end, m.gp.kern.lengthscales.value, m.k_var.value[0], m.var.value[0]))
    assert trace.shape == (31,) and np.all(np.isfinite(trace))
    assert abs(trace[0] - start) <= 1e-8 * abs(start) and abs(trace[-1] - end) <= 1e-8 * abs(end)
    assert trace[-1] > trace[0]
    assert np.abs(m._session.read_raw(m._hyper_variables()["net0.w"]) - w0).max() > 0
    Xs, _ = _data(50, seed=1)
    mean, var = m.predict_y(Xs)
    fmean, fvar = m.predict_f(Xs)
    assert mean.shape == (1, 50) and var.shape == (1, 50) and fmean.shape == (1, 50) and fvar.shape == (1, 50)
    assert np.all(np.isfinite(mean)) and np.all(fvar >= 0) and np.all(var > fvar)
    idx = m.select_inducing()
    assert idx.shape == (32,) and len(set(idx.tolist())) == 32


def test_fit_in_a_float32_session_climbs():
    """float32 features and network chain, float64 bound and gradient at the stored features: 5 steps climb.
    Observed on MI355X: -462.27 -> -354.41."""
    m, X, Y = _model(1024, "float32")
    trace = m.fit(5, lr=0.05)
    print("float32 session: %.4f -> %.4f" % (trace[0], trace[-1]))
    assert trace.shape == (6,) and np.all(np.isfinite(trace)) and trace[-1] > trace[0]
