"""Parameters laid out at odd offsets of the flat parameter buffer.

Session.ensure_layout packs the parameters without padding, so one short parameter sorted ahead of the others moves every
`leaf:param` view off 16-byte alignment.  A kernel form that needs aligned operands must then be declined by the planner
(plan.explain says so) in favour of the form that does not -- not raise at the first run.  The models here get such a
parameter (`a_pad`, 1 to 4 elements, unused by the objective) and are held to the oracle and to their unshifted selves."""
import numpy as np
import pytest
import torch

import henbun_amd as hb
import henbun_oracle as O
from henbun_amd import graph as G
from henbun_amd.models import SVGP, Amortised, DenseGPR

import graph_device as GD
import graph_oracle as GO
import parity

pytestmark = pytest.mark.gpu

FUSED = "fused encoder (hb_mlp2_sample_fwd / _bwd)"


def _shifted(cls, pad):
    class Shifted(cls):
        def setUp(self, *args, **kw):
            cls.setUp(self, *args, **kw)
            if pad:
                self.a_pad = hb.param.Variable([pad])      # created last (same random start for the others), laid out first

    Shifted.__name__ = cls.__name__ + "Pad%d" % pad
    return Shifted


def _params(m):
    return [v for v in m.get_variables() if v.is_parameter]


def _leaf_values(m):
    vals, sess = {}, m._session
    for v in m.get_variables():
        if v.is_parameter:
            vals[v._leaf] = sess.read_raw(v)
        elif isinstance(v, hb.param.MinibatchData):
            for size, leaf in v._leaves.items():
                vals[leaf] = v.data[:size]
        elif isinstance(v, hb.param.Data):
            vals[v._tensor] = v.data
    return vals


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _amortised(pad, dtype):
    np.random.seed(1)
    rng = np.random.RandomState(0)
    N, Din, H, L = 64, 32, 128, 16          # a shape the fused encoder takes (csrc/mlp.hip)
    Y, u = _f32(rng.randn(N, Din)), _f32(rng.randn(N, L))
    m = _shifted(Amortised, pad)(Y=Y, L=L, H=H, dtype=dtype)
    m.z.inject_noise(u)
    opt = m.ELBO()
    opt.compile()
    val, grads = opt.gradients()            # the first run of the model
    return m, opt, Y, u, val, grads


def _encoder_note(plan):
    notes = [(fired, why) for p, _, fired, why in plan.explain if p == FUSED]
    assert len(notes) == 1
    return notes[0]


def _amortised_reference(m, opt, dtype):
    obj = opt._trace(None)
    ps = [v for v in _params(m) if v.long_name != "model.a_pad"]
    gs = G.gradients(obj, [v._leaf for v in ps])
    assert all(g is not None for g in gs)
    vals = GO.evaluate([obj] + gs, _leaf_values(m))
    ref = {"": vals[obj].numpy(), **{v.long_name: vals[g].numpy() for v, g in zip(ps, gs)}}
    e32 = None
    if dtype == "float32":
        v32 = GO.evaluate([obj] + gs, _leaf_values(m), dtype=torch.float32)
        e32 = max(GD.measure(v32[t].numpy(), vals[t].numpy()) for t in [obj] + gs)
    return ref, e32


@pytest.mark.parametrize("pad", [1, 2, 3])
def test_amortised_fp32_with_encoder_weights_at_an_odd_offset(pad):
    m, opt, Y, u, val, grads = _amortised(pad, "float32")
    sess = m._session
    assert sess._offsets[id(m.a_pad)] == (0, pad)
    for w in (m.enc.matbias0.w, m.enc.matbias1.w):
        assert sess._offsets[id(w)][0] % 4 == pad and sess.param_view(w).data_ptr() % 16 != 0
    fired, why = _encoder_note(opt.last_plan)
    assert not fired and "16-byte aligned" in why
    ref, e32 = _amortised_reference(m, opt, "float32")
    err = max([GD.measure(val, ref[""])] + [GD.measure(grads[k], r) for k, r in ref.items() if k])
    print("amortised fp32 pad %d: device error %.3e, evaluator float32 error %.3e" % (pad, err, e32))
    parity.observe("amortised fp32 odd offset, pad %d" % pad, err, GD.FP32_FACTOR * e32 + GD.FP32_FLOOR)
    assert not grads["model.a_pad"].any()
    # the update step (gradients bound into the flat buffer at the same odd offsets, Adam over it) runs as well
    opt.compile()
    opt.optimize(maxiter=2)
    assert np.isfinite(opt.run())


def test_amortised_fp32_with_a_four_element_parameter_keeps_the_fused_encoder():
    for pad in (0, 4):
        m, opt, Y, u, val, grads = _amortised(pad, "float32")
        assert m._session.param_view(m.enc.matbias0.w).data_ptr() % 16 == 0
        fired, why = _encoder_note(opt.last_plan)
        assert fired and why == ""
        ref, e32 = _amortised_reference(m, opt, "float32")
        err = max([GD.measure(val, ref[""])] + [GD.measure(grads[k], r) for k, r in ref.items() if k])
        print("amortised fp32 pad %d (fused): device error %.3e, evaluator float32 error %.3e" % (pad, err, e32))
        parity.observe("amortised fp32 fused encoder, pad %d" % pad, err, GD.FP32_FACTOR * e32 + GD.FP32_FLOOR)


def test_amortised_fp64_with_encoder_weights_at_an_odd_offset():
    m, opt, Y, u, val, grads = _amortised(1, "float64")
    sess = m._session
    assert sess._offsets[id(m.enc.matbias0.w)][0] % 4 == 1
    assert not _encoder_note(opt.last_plan)[0]
    params = {
        "enc_w0": O.T(sess.read_raw(m.enc.matbias0.w)), "enc_b0": O.T(sess.read_raw(m.enc.matbias0.b)),
        "enc_w1": O.T(sess.read_raw(m.enc.matbias1.w)), "enc_b1": O.T(sess.read_raw(m.enc.matbias1.b)),
        "dec_w0": O.T(sess.read_raw(m.dec.matbias0.w)), "dec_b0": O.T(sess.read_raw(m.dec.matbias0.b)),
        "var_raw": O.T(sess.read_raw(m.var)),
    }
    ref_val, ref = O.grads_of(lambda p: O.amortised_elbo(p, O.T(Y), O.T(u)), params)
    # (the bounds of test_model_gpu.py::test_amortised_fp64_parity_and_training)
    assert abs(val - ref_val.item()) <= 1e-8 * abs(ref_val.item())
    names = {"model.enc.matbias0.w": "enc_w0", "model.enc.matbias0.b": "enc_b0", "model.enc.matbias1.w": "enc_w1",
             "model.enc.matbias1.b": "enc_b1", "model.dec.matbias0.w": "dec_w0", "model.dec.matbias0.b": "dec_b0",
             "model.var": "var_raw"}
    for k, r in names.items():
        assert parity.rel_err(grads[k], ref[r].numpy()) <= 1e-7, k


# ---- every other model: the same values whether or not the parameter views are aligned ----------------------------------
def _svgp(pad, dtype):
    np.random.seed(0)
    rng = np.random.RandomState(0)
    N, M = 64, 16
    X = _f32(rng.uniform(0, 6, (N, 1)))
    Y = _f32(np.sin(X) + 0.3 * rng.randn(N, 1))
    Z = _f32(np.linspace(0, 6, M)[:, None])
    m = _shifted(SVGP, pad)(X=X, Y=Y, Z=Z, eps=_f32(rng.randn(N)), dtype=dtype)
    m.u.inject_noise(_f32(rng.randn(M)))
    return m


def _dense(pad, dtype):
    np.random.seed(2)
    rng = np.random.RandomState(0)
    n = 16
    X = _f32(np.sort(rng.uniform(0, 5, (n, 1)), axis=0))
    Y = _f32(np.sin(X) + 0.1 * rng.randn(n, 1))
    m = _shifted(DenseGPR, pad)(X=X, Y=Y, dtype=dtype)
    m.q.q_sqrt = 0.5 * np.eye(n) + 0.05 * rng.randn(n, n)
    m.q.inject_noise(_f32(rng.randn(n)))
    return m


def _run(make, pad, dtype):
    cfg = hb.settings.get_settings()
    cfg.numerics.jitter_level = 1e-3
    with hb.settings.temp_settings(cfg):
        m = make(pad, dtype)
        opt = m.ELBO()
        opt.compile()
        val, grads = opt.gradients()
    forms = [(p, fired) for p, _, fired, _ in opt.last_plan.explain]
    return m, val, grads, forms


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("make", [_svgp, _dense], ids=["svgp", "dense_gpr"])
def test_model_with_every_parameter_view_four_bytes_off(make, dtype):
    m0, val0, g0, forms0 = _run(make, 0, dtype)
    m1, val1, g1, forms1 = _run(make, 1, dtype)
    s1 = m1._session
    assert s1._offsets[id(m1.a_pad)] == (0, 1)
    for v in _params(m1):
        if v is not m1.a_pad:
            assert s1._offsets[id(v)][0] == m0._session._offsets[id([w for w in _params(m0) if w.long_name == v.long_name][0])][0] + 1
    assert set(g1) == set(g0) | {"model.a_pad"} and not g1["model.a_pad"].any()
    same_forms = forms0 == forms1
    # Where a kernel takes another form for the shifted operands the two runs differ by the rounding of another summation
    # order: the longest sum here has 64 terms, so 64 ulp of the largest entry bounds it; with the same forms everywhere
    # the two runs are the same computation, bit for bit.
    ulp = 2.0 ** -24 if dtype == "float32" else 2.0 ** -53
    worst = 0.0
    for k in sorted(g0):
        d = GD.measure(g1[k], g0[k])
        worst = max(worst, d)
        print("%s %s %s: shifted against unshifted %.3e (same forms: %s)" % (make.__name__, dtype, k, d, same_forms))
    dv = GD.measure(val1, val0)
    print("%s %s value: shifted against unshifted %.3e (same forms: %s)" % (make.__name__, dtype, dv, same_forms))
    if same_forms:
        assert dv == 0.0 and worst == 0.0
        for k in g0:
            assert np.array_equal(g0[k], g1[k]), k
    else:
        assert max(dv, worst) <= 64 * ulp
