"""SparseGP.predict_f(full_cov=True) and predict_f_samples on the host: the C ABI of hb_sgp_predict_cov_* validates its
arguments before any launch, the graph has the documented shapes and lowering, the cases it does not take are refused,
and the generic composition, evaluated in fp64 by the test-only CPU evaluator, is the covariance of the definition

    cov_p = A^T S_p S_p^T A + K(x, x) - A^T A + jitter I   ('fullrank')
          = A^T S_p S_p^T A + diag(|1 - colsum(A^2)|)      ('diagonal')
          = A^T S_p S_p^T A                                ('neglected'),   A = chol(K(z, z) + jitter I)^-1 K(z, x).

No HIP kernel runs here."""
import numpy as np
import pytest

import henbun_amd as hb
from henbun_amd import graph as G
from henbun_amd.gp.gp import _posterior_of
from henbun_amd.models import SVGP, ExpertsGPR, svgp_data

import graph_oracle as GO

tf = hb.tf


# ---------------------------------------------------------------- C ABI
def _call(lib, suffix, **kw):
    a = dict(kind=0, x=1, sx=0, z=1, ell=1, dl=1, W=1, Wf=None, s=1, s_kind=0, mode=1, jitter=1e-5, cov=1, E=1, n=64, M=64,
             d=1, P=1, ws=None)
    a.update(kw)
    return lib.raw("hb_sgp_predict_cov" + suffix)(a["kind"], a["x"], a["sx"], a["z"], a["ell"], a["dl"], a["W"], a["Wf"],
                                                  a["s"], a["s_kind"], a["mode"], a["jitter"], a["cov"], a["E"], a["n"],
                                                  a["M"], a["d"], a["P"], a["ws"], None)


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
@pytest.mark.parametrize("bad, word", [
    (dict(mode=7), "mode"),
    (dict(s_kind=3), "s_kind"),
    (dict(kind=1), "UnitRBF"),
    (dict(s_kind=1, P=2), "E P == 1"),
    (dict(s_kind=1, E=3, sx=0), "E P == 1"),
    (dict(cov=None), "NULL"),
    (dict(s=None), "NULL"),
    (dict(ws=None), "workspace"),
    (dict(n=-1), "extents"),
    (dict(M=-5), "extents"),
    (dict(P=-1), "extents"),
])
def test_predict_cov_entry_points_reject_bad_arguments(suffix, bad, word):
    from henbun_amd import _lib

    lib = _lib.lib()
    rc = _call(lib, suffix, **bad)
    assert rc < 0 and word in lib.last_error(), (rc, lib.last_error())


def test_predict_cov_workspace_is_linear_in_n():
    from henbun_amd import _lib

    f = _lib.lib().raw("hb_sgp_predict_cov_ws_elems")
    for E, M, P, sk, b in [(1, 512, 1, 0, 4), (1, 512, 1, 1, 4), (4, 64, 3, 0, 8), (1, 1024, 1, 1, 4)]:
        w1, w2, w4 = (f(E, n, M, P, sk, b) for n in (8192, 16384, 32768))
        assert w1 > 0
        assert w4 - w2 == 2 * (w2 - w1)                    # linear (up to the fixed 64-element rounding)
        per_col = (w4 - w2) / 16384
        assert per_col == E * M + (M if sk else 0) + E     # A, C = S^T A (full rank), a2
        assert w4 < 32768 ** 2 // 8                        # far below the n^2 output


# ---------------------------------------------------------------- graph
def _svgp(q_shape="diagonal", M=64, N=100, dtype="float64"):
    X, Y, Z = svgp_data(N, M, 0)
    return SVGP(X=X, Y=Y, Z=Z, q_shape=q_shape, dtype=dtype), X


@pytest.mark.parametrize("q_shape", ["diagonal", "fullrank"])
@pytest.mark.parametrize("residual", ["diagonal", "neglected", "fullrank"])
def test_full_cov_builds_sgp_predict_cov_and_reuses_the_mean(q_shape, residual):
    m, X = _svgp(q_shape)
    xs = G.as_tensor(np.linspace(0, 30, 77)[:, None])
    q = object.__getattribute__(m, "u")
    with m.tf_mode():
        mean0, var0 = m.gp.predict_f(xs, q, q_shape=residual)
        mean, cov = m.gp.predict_f(xs, q, q_shape=residual, full_cov=True)
    assert cov.node.op == "sgp_predict_cov" and cov.shape == (1, 77, 77)
    assert cov.node.attrs["mode"] == residual and cov.node.attrs["s_kind"] == ("diag" if q_shape == "diagonal" else "tril")
    assert mean is mean0 and mean.node.op == "sgp_predict"
    # the covariance reads the same factor W = L^-1 as the moments (one factorisation, one Wfrag image)
    assert cov.node.inputs[4] is mean.node.inputs[4]


def test_full_cov_expert_batched_z():
    X, Y, Z = svgp_data(200, 32, 0)
    m = ExpertsGPR(X=X, Y=Y, Z=Z, ells=[0.5, 1.0, 1.5, 2.0])
    q = object.__getattribute__(m, "u")
    xs = G.as_tensor(X[:45])
    with m.tf_mode():
        mean0, _ = m.gp.predict_f(xs, q)
        mean, cov = m.gp.predict_f(xs, q, full_cov=True)
    assert cov.node.op == "sgp_predict_cov" and cov.shape == (4, 1, 45, 45)
    assert mean is mean0 and mean.shape == (4, 1, 45)


def _op_list(outs):
    return [(n.op, tuple(t.shape for t in n.outputs)) for n in G.topo_order(list(outs))]


@pytest.mark.parametrize("q_shape", ["diagonal", "fullrank"])
def test_full_cov_false_leaves_the_graph_unchanged(q_shape):
    """predict_f(full_cov=False) builds exactly the graph the moments-only predict_f built: one sgp_predict node on the
    factorisation of z and the parameters of q."""
    m, X = _svgp(q_shape)
    xs = G.as_tensor(X[:33])
    q = object.__getattribute__(m, "u")
    with m.tf_mode():
        mean, var = m.gp.predict_f(xs, q, q_shape="diagonal", full_cov=False)
        mm, s, kind = _posterior_of(q)
        kern, z = m.gp.kern, m.gp._z()
        em, ev = G.sgp_predict(xs, z, kern._ell(), kern.Cholesky(z), mm, s, mode="diagonal", s_kind=kind,
                               jitter=hb.settings.numerics.jitter_level)
    assert _op_list([mean, var]) == _op_list([em, ev])
    assert mean is em and var is ev


def test_generic_composition_for_matern_tril_with_several_latents_and_fused_predict_off():
    X, Y, Z = svgp_data(60, 16, 0)
    xs = G.as_tensor(X[:20])
    gp = hb.gp.SparseGP(kern=hb.gp.kernels.UnitMatern52(np.ones(1)), z=Z)
    mean, cov = gp.predict_f(xs, hb.variationals.Normal(shape=[2, 16]), full_cov=True)
    assert cov.node.op != "sgp_predict_cov" and cov.shape == (2, 20, 20) and mean.shape == (2, 20)
    gp = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(np.ones(1)), z=Z)
    mean, cov = gp.predict_f(xs, hb.variationals.Normal(shape=[2, 16], q_shape="fullrank"), full_cov=True)
    assert cov.node.op != "sgp_predict_cov" and cov.shape == (2, 20, 20) and mean.node.op == "sgp_predict"
    cfg = hb.settings.get_settings()
    cfg.runtime.fused_predict = False
    with hb.settings.temp_settings(cfg):
        mean, cov = gp.predict_f(xs, hb.variationals.Normal(shape=[2, 16]), full_cov=True)
    assert cov.node.op != "sgp_predict_cov" and cov.shape == (2, 20, 20) and mean.node.op == "sgp_predict"
    assert "sgp_predict_cov" not in [n.op for n in G.topo_order([cov])]


def test_full_cov_refuses_3d_x():
    X, Y, Z = svgp_data(60, 16, 0)
    gp = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(np.ones(1)), z=Z)
    q = hb.variationals.Normal(shape=[3, 16])
    with pytest.raises(NotImplementedError, match="2-D"):
        gp.predict_f(np.random.rand(3, 7, 1), q, full_cov=True)


def test_predict_f_samples_shape_and_neglected():
    m, X = _svgp("fullrank")
    q = object.__getattribute__(m, "u")
    with m.tf_mode():
        f = m.gp.predict_f_samples(X[:25], q, 11)
        with pytest.raises(ValueError, match="neglected"):
            m.gp.predict_f_samples(X[:25], q, 11, q_shape="neglected")
    assert f.shape == (1, 11, 25)
    ops = [n.op for n in G.topo_order([f])]
    assert "sgp_predict_cov" in ops and "cholesky" in ops and "leaf:noise" in ops
    assert q._draw is None              # no sample of q was drawn / cached for the trace
    X, Y, Z = svgp_data(200, 32, 0)
    me = ExpertsGPR(X=X, Y=Y, Z=Z, ells=[0.5, 1.0, 1.5, 2.0])
    with me.tf_mode():
        fe = me.gp.predict_f_samples(X[:9], object.__getattribute__(me, "u"), 5, q_shape="diagonal")
    assert fe.shape == (4, 1, 5, 9)


def test_full_cov_and_draws_are_forward_only():
    m, X = _svgp()
    q = object.__getattribute__(m, "u")
    mu, sq = q._raw_params()
    _, cov = m.gp.predict_f(X[:10], q, full_cov=True)
    f = m.gp.predict_f_samples(X[:10], q, 3)
    for out in (cov, f):
        with pytest.raises(NotImplementedError, match="forward-only"):
            G.gradients(G.reduce_sum(out), [mu, sq])


# ---------------------------------------------------------------- the generic composition in fp64
class CovModel(hb.model.Model):
    def setUp(self, Z, kern, shape, q_shape):
        self.gp = hb.gp.SparseGP(kern=kern, z=Z)
        self.u = hb.variationals.Normal(shape=shape, q_shape=q_shape)


def _leaf_values(model):
    return {v._leaf: v._host_raw for v in model.get_variables() if v.is_parameter}


def _k(kind, a, b, ell):
    d = (a[:, None, :] - b[None, :, :]) / ell
    r2 = (d * d).sum(-1)
    if kind == "rbf":
        return np.exp(-0.5 * r2)
    r2 = r2 + 1e-12                       # the Matern kernels' euclid_dist
    r = np.sqrt(5.0 * r2)
    return (1.0 + r + 5.0 / 3.0 * r2) * np.exp(-r)


def _reference_cov(kind, x, z, ell, s, s_kind, P, mode, jitter):
    M = z.shape[0]
    L = np.linalg.cholesky(_k(kind, z, z, ell) + jitter * np.eye(M))
    A = np.linalg.solve(L, _k(kind, z, x, ell))
    out = []
    for p in range(P):
        Sp = np.diag(s[p]) if s_kind == "diag" else s[p * M:(p + 1) * M, :]
        C = Sp.T @ A
        cov = C.T @ C
        if mode == "fullrank":
            cov = cov + _k(kind, x, x, ell) - A.T @ A + jitter * np.eye(len(x))
        elif mode == "diagonal":
            cov = cov + np.diag(np.abs(1.0 - (A * A).sum(0)))
        out.append(cov)
    return np.stack(out)


@pytest.mark.parametrize("kern_kind", ["matern52", "rbf"])
@pytest.mark.parametrize("q_shape", ["diagonal", "fullrank"])
@pytest.mark.parametrize("mode", ["fullrank", "diagonal", "neglected"])
def test_generic_composition_is_the_covariance_of_the_definition(kern_kind, q_shape, mode):
    rng = np.random.RandomState(7)
    M, n, P, jitter = 12, 17, 2, 1e-4
    Z = np.linspace(0.0, 6.0, M)[:, None]
    kern = hb.gp.kernels.UnitMatern52(np.ones(1) * 1.3) if kern_kind == "matern52" else hb.gp.kernels.UnitRBF(np.ones(1) * 1.3)
    m = CovModel(Z=Z, kern=kern, shape=[P, M], q_shape=q_shape)
    q = object.__getattribute__(m, "u")
    size = P * M
    q.q_mu = rng.randn(size)
    if q_shape == "diagonal":
        q.q_sqrt = np.log(rng.uniform(0.2, 1.0, size))
    else:
        q.q_sqrt = np.tril(0.3 * rng.randn(size, size) / np.sqrt(size)) + np.diag(rng.uniform(0.2, 0.9, size))
    x = rng.uniform(-0.5, 6.5, (n, 1))
    cfg = hb.settings.get_settings()
    cfg.numerics.jitter_level = jitter
    cfg.runtime.fused_predict = False
    with hb.settings.temp_settings(cfg):
        mean, cov = m.gp.predict_f(x, q, q_shape=mode, full_cov=True)
        mm, s, kind = _posterior_of(q)
        gmean, gvar = m.gp._predict_generic(G.as_tensor(x), mm, s, kind, mode, jitter)
        ell = m.gp.kern._ell()
        z = m.gp._z()
    assert cov.node.op != "sgp_predict_cov" and cov.shape == (P, n, n)
    vals = GO.evaluate([cov, gvar, s, ell, z], _leaf_values(m))
    got = vals[cov].numpy()
    ref = _reference_cov(kern_kind, x, vals[z].numpy(), vals[ell].numpy(), vals[s].numpy(), kind, P, mode, jitter)
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() <= 1e-10 * scale, np.abs(got - ref).max() / scale
    # diag(cov) == predict_f's var (the generic moments, evaluated the same way)
    dg = np.diagonal(got, axis1=-2, axis2=-1)
    assert np.abs(dg - vals[gvar].numpy()).max() <= 1e-10 * scale
