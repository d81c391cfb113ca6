"""Every planner pass once firing and once declining (tests/graph_passes.py), on the device.

Each test first asserts from the plan -- plan.explain, the step labels, plan._place, plan._lazy_cols, plan._colsum_of,
plan._gll_post, buffer sizes -- that the pass did what the test's name says, then sends the values of the graph and of
its gradients through the harness of tests/graph_device.py (float64: the default plan, the plain lowering and the
captured graph; float32: the default plan).  The plain lowering must show no fusion at all."""
import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd import graph as G

import graph_device as GD
import graph_passes as GP

pytestmark = pytest.mark.gpu


def _inspect(spec, tr):
    def inspect(plan, mode):
        if mode == "plain":
            assert not plan._clusters and not plan._colclusters and not plan._gll_post
            assert not any(lab.startswith(("ew_cluster[", "col_cluster[")) for lab in GD.labels(plan))
            assert ("elementwise fusion", "-", False, "settings.runtime.fuse_elementwise is off") in plan.explain
        else:
            spec.check(plan, tr)
    return inspect


@pytest.mark.parametrize("name", sorted(GP.PASSES))
def test_pass(name):
    spec = GP.PASSES[name]
    tr = GD.Traced(spec.build, spec.shapes, kinds=spec.kinds, positive=spec.positive, dtype="float64", weighted=spec.weighted)
    if name in GP.PURE:
        order = tr.order()
        ew, col, m = GP.pure_decisions(order, tr.outputs, column_programs=bool(spec.runtime.get("column_programs", True)))
        GP.PURE[name](order, ew, col, tr.y, m)
    GD.run_modes(tr, name, ("default", "plain", "captured"), inspect=_inspect(spec, tr), runtime=spec.runtime)
    tr32 = GD.Traced(spec.build, spec.shapes, kinds=spec.kinds, positive=spec.positive, dtype="float32", weighted=spec.weighted)
    GD.run_modes(tr32, name, ("default",), inspect=_inspect(spec, tr32), runtime=spec.runtime)
    print("graph_device programs compiled so far: %d" % GD.PROGRAMS["compiled"])


def test_serial_chain_of_three_programs_and_the_same_plan_without_chains():
    spec = GP.PASSES["fullsum_read_by_the_same_space_starts_a_new_program"]
    tr = GD.Traced(spec.build, spec.shapes, dtype="float64")

    def inspect(plan, mode):
        ch = GD.chains(plan)
        if mode == "nochain":
            assert ch == [] and len([l for l in GD.labels(plan) if l.startswith("ew_cluster[")]) == 3
            assert not any(p == "serial chain" for p, _, _, _ in plan.explain)
        else:
            assert len(ch) == 1 and len(ch[0]) == 3 and all(l.startswith("ew_cluster[") for l in ch[0])
            assert [f for p, _, f, _ in plan.explain if p == "serial chain"] == [True]

    GD.run_modes(tr, "serial chain", ("default", "nochain", "captured"), inspect=inspect)


# ---- outputs and binds: gradients written into a caller's flat buffer (Optimizer._get_plan binds them this way) ----------
def _bound(build, shapes, weighted=True, kinds=None):
    """Lower the graph with every gradient bound to its slice of one flat buffer; returns (traced, plan, flat, slices)."""
    tr = GD.Traced(build, shapes, kinds=kinds, dtype="float64", weighted=weighted)
    sess = tr.model._session
    sess.ensure_layout()
    sizes = [int(np.prod(s)) for s in shapes]
    flat = torch.full((sum(sizes) + 3,), np.nan, dtype=torch.float64, device=sess.device)
    binds, slices, off = [], [], 1        # (one element in: the slices are not 16-byte aligned)
    for g, s in zip(tr.grads, sizes):
        if g is not None:
            binds.append((g, flat[off:off + s]))
        slices.append((off, s))
        off += s
    plan = tr.make_plan(binds=binds)
    GD.run_plan(tr, plan, "binds")
    ref = tr.reference()
    got = flat.cpu().numpy()
    for g, (o, s) in zip(tr.grads, slices):
        if g is None:
            assert np.isnan(got[o:o + s]).all()
            continue
        r = ref[tr.outputs.index(g)].reshape(-1)
        assert GD.measure(got[o:o + s], r) <= GD.FP64_BOUND, (g, got[o:o + s], r)
    assert np.isnan(got[0]) and np.isnan(got[off:]).all()       # nothing was written outside the bound slices
    return tr, plan, flat, slices


def test_bound_gradient_that_is_a_reshape_of_another_bound_gradient():
    tr, plan, flat, slices = _bound(lambda p, q: G.unary("TANH", p + G.reshape(q, [12])), [(12,), (3, 4)])
    gp, gq = tr.grads
    assert gq.node.op == "reshape" and gq.node.inputs[0] is gp
    assert gp in plan._bind and [t for t, _ in plan._extra_copies] == [gp]      # one buffer written in place, one copy
    assert plan.buf(gp).data_ptr() in (flat[slices[0][0]:].data_ptr(), flat[slices[1][0]:].data_ptr())


def test_one_gradient_tensor_bound_to_two_parameters():
    tr, plan, flat, slices = _bound(lambda p, q: G.unary("TANH", p + q), [(12,), (12,)], kinds=["param", "param"])
    assert tr.grads[0] is tr.grads[1] and [t for t, _ in plan._extra_copies] == [tr.grads[0]]


def test_bound_gradient_that_is_a_stop_gradient_or_a_leaf():
    # with a one-element objective, d (stop_gradient(x) * z) / dz IS the stop_gradient node and d (x * z) / dz IS the
    # leaf x: neither may be written in place (the bound buffer would alias an input); both arrive by the closing copy
    tr, plan, flat, slices = _bound(lambda x, z: G.stop_gradient(G.unary("TANH", x)) * z, [(1,), (1,)], weighted=None)
    assert tr.grads[0] is None and tr.grads[1].node.op == "stop_gradient"
    assert plan.buf(tr.grads[1]).data_ptr() != flat[slices[1][0]:].data_ptr()
    tr, plan, flat, slices = _bound(lambda x, z: x * z, [(1,), (1,)], weighted=None)
    assert tr.grads[1] is tr.leaves[0] and tr.grads[0] is tr.leaves[1]
    assert plan.buf(tr.grads[1]).data_ptr() != flat[slices[1][0]:].data_ptr()


class _Small(hb.model.Model):
    def setUp(self, X):
        self.X = hb.param.Data(X)
        self.a = hb.param.Variable([12])
        self.b = hb.param.Variable([3, 4])
        self.c = hb.param.Variable([1])
        self.d = hb.param.Variable([1])

    @hb.model.AutoOptimize()
    def objective(self):
        # db is a reshape of da; dc IS stop_gradient(d), and d itself gets no gradient
        t = G.unary("TANH", self.a + G.reshape(self.b, [12]))
        return G.reduce_sum(t * G.reshape(self.X, [12])) + G.stop_gradient(self.d) * self.c


def test_optimizer_gradients_of_a_small_model_are_the_evaluators():
    import graph_oracle as GO

    rng = np.random.RandomState(3)
    m = _Small(X=rng.randn(3, 4), dtype="float64")
    opt = m.objective()
    opt.compile()
    val, grads = opt.gradients()
    sess = m._session
    obj = opt._trace(None)
    ps = [m.a, m.b, m.c, m.d]
    gs = G.gradients(obj, [v._leaf for v in ps])
    assert gs[1].node.op == "reshape" and gs[1].node.inputs[0] is gs[0] and gs[2].node.op == "stop_gradient" and gs[3] is None
    vals = GO.evaluate([obj] + gs[:3], {**{v._leaf: sess.read_raw(v) for v in ps}, m.X._tensor: m.X.data})
    assert GD.measure(val, vals[obj].numpy()) <= GD.FP64_BOUND
    for v, g in zip(ps[:3], gs):
        assert GD.measure(grads[v.long_name], vals[g].numpy()) <= GD.FP64_BOUND, v.long_name
    assert not grads["model.d"].any()
