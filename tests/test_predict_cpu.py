"""SparseGP.predict_f on the host: the C ABI of hb_sgp_predict_* validates its arguments before any launch, the graph op
it lowers to has the shapes of samples(), and the cases it does not take are refused.  No HIP kernel runs here."""
import numpy as np
import pytest

import henbun_amd as hb
from henbun_amd import graph as G
from henbun_amd.models import SVGP, ExpertsGPR, svgp_data

tf = hb.tf


# ---------------------------------------------------------------- C ABI
def _call(lib, suffix, **kw):
    a = dict(kind=0, x=1, sx=0, z=1, ell=1, dl=1, W=1, Wf=None, m=1, s=1, s_kind=0, mode=1, jitter=1e-5, mean=1, var=1,
             E=1, n=64, M=64, d=1, P=1, ws=None)
    a.update(kw)
    return lib.raw("hb_sgp_predict" + suffix)(a["kind"], a["x"], a["sx"], a["z"], a["ell"], a["dl"], a["W"], a["Wf"], a["m"],
                                              a["s"], a["s_kind"], a["mode"], a["jitter"], a["mean"], a["var"], a["E"], a["n"],
                                              a["M"], a["d"], a["P"], a["ws"], None)


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
@pytest.mark.parametrize("bad, word", [
    (dict(mode=7), "mode"),
    (dict(s_kind=3), "s_kind"),
    (dict(kind=1), "UnitRBF"),
    (dict(P=0), "extents"),
    (dict(M=0), "extents"),
    (dict(dl=3), "lengthscales"),
    (dict(sx=5), "sx"),
    (dict(m=None), "NULL"),
    (dict(var=None), "NULL"),
    (dict(ws=None), "workspace"),          # chunked form (no Wfrag) without its scratch
])
def test_predict_entry_points_reject_bad_arguments(suffix, bad, word):
    from henbun_amd import _lib

    lib = _lib.lib()
    rc = _call(lib, suffix, **bad)
    assert rc < 0 and word in lib.last_error(), (rc, lib.last_error())


def test_predict_workspace_is_bounded_by_a_chunk_not_by_n():
    from henbun_amd import _lib

    f = _lib.lib().raw("hb_sgp_predict_ws_elems")
    # fused form: nothing (diagonal S) or the S^T image (full rank), whatever n is
    assert f(1, 10 ** 6, 512, 1, 1, 0, 1, 4) == 0
    assert f(1, 10 ** 6, 512, 1, 1, 1, 1, 4) == 512 * 512
    # chunked form: one chunk of A (and of S^T A), the same for 1e5 and 1e7 columns
    for args in [(1, 512, 1, 1, 0, 0, 4), (1, 1024, 1, 1, 1, 1, 4), (1, 512, 1, 1, 1, 0, 8), (4, 512, 6, 3, 0, 1, 4)]:
        E, M, d, P, sk, wf, b = args
        small, big = f(E, 10 ** 5, M, d, P, sk, wf, b), f(E, 10 ** 7, M, d, P, sk, wf, b)
        assert small == big and 0 < big <= (1 << 24) + E * M * 32 * (1 + E * P * E * P)
    # fp64 never takes the fused form
    assert f(1, 10 ** 6, 512, 1, 1, 0, 1, 8) > 0


# ---------------------------------------------------------------- graph
def _svgp(q_shape="diagonal", M=64, N=100):
    X, Y, Z = svgp_data(N, M, 0)
    return SVGP(X=X, Y=Y, Z=Z, q_shape=q_shape), X


@pytest.mark.parametrize("q_shape", ["diagonal", "fullrank"])
@pytest.mark.parametrize("residual", ["diagonal", "neglected", "fullrank"])
def test_predict_f_builds_sgp_predict_with_the_shape_of_samples(q_shape, residual):
    m, X = _svgp(q_shape)
    xs = np.linspace(0, 30, 77)[:, None]
    q = object.__getattribute__(m, "u")
    with m.tf_mode():
        mean, var = m.gp.predict_f(xs, q, q_shape=residual)
        f = m.gp.samples(xs, m.u, q_shape="neglected")
    assert mean.node.op == "sgp_predict" and var.node is mean.node
    assert mean.shape == var.shape == f.shape == (1, 77)
    assert mean.node.attrs["mode"] == residual
    assert mean.node.attrs["s_kind"] == ("diag" if q_shape == "diagonal" else "tril")


def test_predict_f_expert_batched_z():
    X, Y, Z = svgp_data(200, 32, 0)
    m = ExpertsGPR(X=X, Y=Y, Z=Z, ells=[0.5, 1.0, 1.5, 2.0])
    q = object.__getattribute__(m, "u")
    with m.tf_mode():
        mean, var = m.gp.predict_f(X[:45], q)
    assert mean.node.op == "sgp_predict"
    assert mean.shape == var.shape == (4, 1, 45)
    assert mean.node.inputs[1].shape == (4, 32, 1)


def test_predict_f_generic_composition_for_other_kernels_and_3d_x():
    X, Y, Z = svgp_data(60, 16, 0)
    gp = hb.gp.SparseGP(kern=hb.gp.kernels.UnitMatern32(np.ones(1)), z=Z)
    q = hb.variationals.Normal(shape=[2, 16])
    mean, var = gp.predict_f(X[:20], q)
    assert mean.node.op != "sgp_predict" and mean.shape == var.shape == (2, 20)
    gp3 = hb.gp.SparseGP(kern=hb.gp.kernels.UnitRBF(np.ones(1)), z=Z)
    q3 = hb.variationals.Normal(shape=[3, 16], q_shape="fullrank")
    mean, var = gp3.predict_f(np.random.rand(3, 7, 1), q3, q_shape="diagonal")
    assert mean.node.op != "sgp_predict" and mean.shape == var.shape == (3, 7)


def test_predict_f_reads_parameters_only():
    m, X = _svgp("diagonal")
    q = object.__getattribute__(m, "u")
    with m.tf_mode():
        m.gp.predict_f(X[:10], q)
    assert q._draw is None              # no sample was drawn / cached for the trace


def test_predict_f_refuses_a_sample_tensor():
    m, X = _svgp()
    with m.tf_mode():
        with pytest.raises(TypeError, match="Variational"):
            m.gp.predict_f(X[:10], m.u)
    with pytest.raises(TypeError):
        m.gp.predict_f(X[:10], np.zeros((1, 64)))


@pytest.mark.parametrize("make", [
    lambda M: hb.variationals.Normal(shape=[1, M], collections=hb.param.graph_key.LOCAL),
    lambda M: hb.variationals.OffsetGaussian(shape=[1, M]),
    lambda M: hb.variationals.Normal(shape=[1, M], n_layers=[2]),
    lambda M: hb.variationals.Variational(shape=[1, M]),
])
def test_predict_f_refuses_unsupported_variationals(make):
    m, X = _svgp()
    with pytest.raises(NotImplementedError):
        m.gp.predict_f(X[:10], make(64))


def test_predict_f_refuses_a_non_identity_transform():
    m, X = _svgp()
    q = hb.variationals.Normal(shape=[1, 64])
    q.transform = hb.transforms.positive
    with pytest.raises(NotImplementedError, match="Identity"):
        m.gp.predict_f(X[:10], q)


def test_predict_f_is_forward_only():
    m, X = _svgp()
    q = object.__getattribute__(m, "u")
    mu, _ = q._raw_params()
    mean, var = m.gp.predict_f(X[:10], q)
    for out in (mean, var):
        with pytest.raises(NotImplementedError, match="forward-only"):
            G.gradients(G.reduce_sum(out), [mu])
