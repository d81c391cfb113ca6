"""TEST INFRASTRUCTURE: run a traced graph on the device and hold it to the CPU evaluator (tests/graph_oracle.py).

The kernels have exact tests of their own; what this checks is the layer between the graph and the kernels
(henbun_amd.graph.Plan): which kernel runs, on which buffer, in what order.  A builder `f(*leaves) -> Tensor` becomes
`y = f(...)`, `loss = reduce_sum(y * w)` and `gradients(loss, leaves)`, lowered as ONE plan and run in every execution
mode of the planner:

    default     ewise = jit, elementwise clusters, column programs, serial chains, eager
    nochain     settings.runtime.serial_chains = False
    interpret   settings.runtime.ewise = interpret (no compiled programs, no column programs, no chains)
    plain       settings.runtime.fuse_elementwise = False: one launch per node
    captured    the default plan after Plan.capture(), replayed twice

Every mode is held to the float64 evaluator (fp64: 1e-10, with a factorisation or a Gram matrix 1e-8; fp32: eight times
the evaluator's own float32 error plus four ulp), and in every mode a second run must give the bits of the first, no leaf
buffer (the data arrays, the flat parameter buffer) may change, and no side job may be left pending.
"""
import numpy as np
import torch

import henbun_amd as hb
from henbun_amd import graph as G

import graph_cases as GC
import graph_oracle as GO
import parity

MODES = ("default", "nochain", "interpret", "plain", "captured")
FP64_BOUND, FP64_BOUND_FACTORISED = 1e-10, 1e-8
FP32_FACTOR, FP32_FLOOR = 8.0, 4.0 * 2.0 ** -24


PROGRAMS = {"compiled": 0}      # fused programs built by the plans of this process (compiled modes): reported by the tests


def mode_settings(mode, runtime=None):
    cfg = hb.settings.get_settings()
    for k, v in (runtime or {}).items():
        setattr(cfg.runtime, k, v)
    if mode == "nochain":
        cfg.runtime.serial_chains = False
    elif mode == "interpret":
        cfg.runtime.ewise = "interpret"
    elif mode == "plain":
        cfg.runtime.fuse_elementwise = False
    elif mode not in ("default", "captured"):
        raise ValueError(mode)
    return cfg


def measure(got, ref):
    """max |got - ref| / max(1, max |ref|)"""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    if got.size == 0:
        return 0.0
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


def leaf_arrays(shapes, seed, positive=False, dtype="float64"):
    rng = np.random.RandomState(seed)
    arrs = [np.abs(rng.randn(*s)) + 0.5 if positive else rng.randn(*s) for s in shapes]
    if dtype == "float32":
        arrs = [a.astype(np.float32).astype(np.float64) for a in arrs]
    return arrs, rng


class Traced:
    """A model whose leaves are real device buffers, and the graph [y, loss] + gradients traced over them."""

    def __init__(self, build, shapes, kinds=None, seed=0, positive=False, dtype="float64", pad=1, weighted=True):
        G.reset_interning()
        self.dtype = dtype
        arrs, rng = leaf_arrays(shapes, seed, positive, dtype)
        kinds = list(kinds) if kinds is not None else ["param" if i % 2 else "data" for i in range(len(shapes))]
        m = hb.model.Model(dtype=dtype)
        if pad:
            # one short parameter laid out first: every parameter view then starts `pad` elements into the flat buffer
            m.a_pad = hb.param.Variable([pad])
        self.vars, self.leaves = [], []
        for i, (a, k) in enumerate(zip(arrs, kinds)):
            if k == "param":
                v = hb.param.Variable(list(a.shape))
                setattr(m, "leaf%02d" % i, v)
                v.assign(a)
                self.leaves.append(v._leaf)
            else:
                v = hb.param.Data(a if dtype == "float64" else a.astype(np.float32))
                setattr(m, "leaf%02d" % i, v)
                self.leaves.append(v._tensor)
            self.vars.append(v)
        self.model, self.arrs, self.kinds = m, arrs, kinds
        self.y, self.loss, self.grads, self.outputs = GC.trace_graph(build, self.leaves, rng, weighted)
        self.leaf_values = dict(zip(self.leaves, arrs))
        self._ref = self._ref32 = None

    def order(self):
        return G.topo_order(self.outputs)

    def reference(self):
        if self._ref is None:
            vals = GO.evaluate(self.outputs, self.leaf_values)
            self._ref = [vals[t].numpy() for t in self.outputs]
        return self._ref

    def e32(self):
        """The evaluator's own float32 evaluation against its float64 one."""
        if self._ref32 is None:
            vals = GO.evaluate(self.outputs, self.leaf_values, dtype=torch.float32)
            self._ref32 = max(measure(vals[t].numpy(), r) for t, r in zip(self.outputs, self.reference()))
        return self._ref32

    def factorised(self):
        return any(n.op in ("cholesky", "trinv", "gram", "gram_grad") for n in self.order())

    def make_plan(self, binds=None):
        return self.model._session.make_plan(self.outputs, binds=binds)


def _leaf_buffers(tr):
    sess = tr.model._session
    bufs = [sess.theta] + [sess.data_buffer(v) for v, k in zip(tr.vars, tr.kinds) if k != "param"]
    return bufs


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def run_plan(tr, plan, name, factor=FP32_FACTOR, captured=False):
    """run(), check(), read every output; run again: same bits, untouched leaves, nothing pending; then the bound."""
    H = plan.H
    torch.cuda.synchronize()
    before = [b.clone() for b in _leaf_buffers(tr)]
    plan.run()
    plan.check()
    first = [plan.value(t).copy() for t in tr.outputs]
    plan.run()
    plan.check()
    second = [plan.value(t).copy() for t in tr.outputs]
    for t, a, b in zip(tr.outputs, first, second):
        assert np.array_equal(_bits(a), _bits(b)), "%s: a second run of the same plan gave other bits for %r" % (name, t)
    for b0, b1 in zip(before, _leaf_buffers(tr)):
        assert torch.equal(b0.view(torch.uint8), b1.view(torch.uint8)), "%s: the run wrote into a leaf buffer" % name
    assert H.side_pending() == 0, "%s: side jobs left pending" % name
    assert plan.is_captured == captured
    ref = tr.reference()
    for t, a, r in zip(tr.outputs, first, ref):
        assert tuple(a.shape) == tuple(t.shape) == tuple(r.shape), (name, t, a.shape, r.shape)
    err = max(measure(a, r) for a, r in zip(first, ref))
    if tr.dtype == "float64":
        bound = FP64_BOUND_FACTORISED if tr.factorised() else FP64_BOUND
        assert np.isfinite(err) and err <= bound, "%s: error %.3e against the evaluator exceeds %.1e" % (name, err, bound)
    else:
        e32 = tr.e32()
        bound = factor * e32 + FP32_FLOOR
        print("fp32 %s: device error %.3e, evaluator float32 error %.3e, ratio to bound %.3f" % (name, err, e32, err / bound))
        parity.observe("graph_device " + name, err, bound)
    return first


def run_modes(tr, name, modes=MODES, factor=FP32_FACTOR, inspect=None, runtime=None):
    """Lower and run `tr` in each of `modes`; `inspect(plan, mode)` sees every plan before it runs (the fire / decline
    assertions of tests/test_graph_passes_gpu.py); `runtime`: further settings.runtime values.  Returns {mode: plan}."""
    plans = {}
    for mode in modes:
        with hb.settings.temp_settings(mode_settings(mode, runtime)):
            plan = tr.make_plan()
            if mode != "interpret":
                PROGRAMS["compiled"] += sum(1 for lab in labels(plan) if lab.startswith(("ew_cluster[", "col_cluster[")))
            if inspect is not None:
                inspect(plan, mode)
            label = "%s[%s,%s]" % (name, tr.dtype, mode)
            eager = run_plan(tr, plan, label, factor)
            if mode == "captured":
                assert plan.capture(), "%s: the plan refuses capture: %s" % (label, plan._nocap)
                replay = run_plan(tr, plan, label + " replay", factor, captured=True)
                for t, a, b in zip(tr.outputs, eager, replay):
                    assert np.array_equal(_bits(a), _bits(b)), "%s: the captured replay differs from the eager run for %r" % (label, t)
            plans[mode] = plan
    return plans


def labels(plan):
    """Step labels of the plan, chains opened up: what was launched, in order."""
    plan.fuse_chains()
    return [plan.step_labels.get(id(m), "other") for s in plan.steps for m in plan.chain_members.get(id(s), [s])]


def chains(plan):
    """The serial chains of the plan: one list of member labels per fused step."""
    plan.fuse_chains()
    return [[plan.step_labels.get(id(m), "other") for m in plan.chain_members[id(s)]] for s in plan.steps if id(s) in plan.chain_members]
