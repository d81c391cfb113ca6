"""CPU half of the planner tests (the device half: tests/test_graph_device_gpu.py, tests/test_graph_passes_gpu.py).

Every graph the device tests run is traced, differentiated and evaluated here first, with the CPU evaluator
(tests/graph_oracle.py), in float64 and in float32; the generated graphs are shown to be 32 graphs with finite, moderate
values that make the planner cluster and concatenate; and the fire / decline expectations that depend only on the
planner's graph-only functions (the clustering, the likelihood head's tail, concat placement, the colsum pairing) are
asserted without a device."""
import re

import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd import graph as G

import graph_cases as GC
import graph_oracle as GO
import graph_passes as GP


def _trace(build, shapes, positive=False, seed=0, weighted=True):
    """The graph tests/graph_device.Traced builds, with plain data leaves (no device, no model)."""
    G.reset_interning()
    rng = np.random.RandomState(seed)
    arrs = [np.abs(rng.randn(*s)) + 0.5 if positive else rng.randn(*s) for s in shapes]
    leaves = [G.leaf("data", tuple(s), var=None) for s in shapes]
    y, loss, grads, outs = GC.trace_graph(build, leaves, rng, weighted)
    return leaves, arrs, y, grads, outs


@pytest.mark.parametrize("case", GC.CATALOGUE, ids=lambda c: c.name)
def test_catalogue_graph_traces_differentiates_and_evaluates(case):
    leaves, arrs, y, grads, outs = _trace(case.build, case.shapes, case.positive)
    assert all(g is not None for g in grads), "a leaf of the catalogue graph has no gradient path"
    v64 = GO.evaluate(outs, dict(zip(leaves, arrs)))
    v32 = GO.evaluate(outs, dict(zip(leaves, [a.astype(np.float32).astype(np.float64) for a in arrs])), dtype=torch.float32)
    for t in outs:
        a, b = v64[t].numpy(), v32[t].numpy()
        assert a.dtype == np.float64 and b.dtype == np.float32 and a.shape == tuple(t.shape) == b.shape
        assert np.isfinite(a).all() and np.isfinite(b).all()
        # float32 inputs and float32 arithmetic: the same numbers to single precision (the catalogue graphs are a few
        # well-conditioned ops deep; 1e-3 separates "single precision" from "another graph")
        assert np.abs(a - b).max() <= 1e-3 * max(1.0, np.abs(a).max()), t


def test_generated_graphs_trace_evaluate_and_exercise_the_planner():
    ran = clustered = with_concat = 0
    for seed in GC.GEN_SEEDS:
        build, shapes = GC.generated(seed)
        leaves, arrs, y, grads, outs = _trace(build, shapes, seed=seed)
        assert GC.op_count(y) <= GC.GEN_MAX_NODES, seed
        assert all(tuple(s) in GC.GEN_LEAF_SHAPES for s in shapes)
        assert all(g is not None for g in grads), "seed %d: a leaf does not reach the result" % seed
        vals = GO.evaluate(outs, dict(zip(leaves, arrs)))
        for t in G.topo_order(outs):
            for o in t.outputs:
                v = vals[o].numpy()
                assert np.isfinite(v).all() and (v.size == 0 or np.abs(v).max() <= 1e6), (seed, o)
        order = G.topo_order(outs)
        members = G.cluster_elementwise(order, max_elems=G.EW_CLUSTER_MAX_ELEMS_JIT, skip=set(G.cluster_columns(order, outputs=outs)))
        if any(len(c.nodes) >= 3 for c in members.values()):
            clustered += 1
        if any(n.op in ("concat", "scatter_strided") for n in order):
            with_concat += 1
        # the same seed gives the same graph
        G.reset_interning()
        again = G.as_tensor(build(*[G.leaf("data", tuple(s), var=None) for s in shapes]))
        assert [n.op for n in G.topo_order([again])] == [n.op for n in G.topo_order([y])]
        ran += 1
    assert ran == 32
    assert clustered >= 16, clustered
    assert with_concat >= 4, with_concat


@pytest.mark.parametrize("name", sorted(GP.PURE))
def test_clustering_decisions_that_need_no_device(name):
    """The fire / decline expectations of tests/test_graph_passes_gpu.py that the planner's graph-only functions decide
    alone (tests/graph_passes.pure_decisions)."""
    spec = GP.PASSES[name]
    leaves, arrs, y, grads, outs = _trace(spec.build, spec.shapes, spec.positive)
    order = G.topo_order(outs)
    ew, col, m = GP.pure_decisions(order, outs)
    GP.PURE[name](order, ew, col, y, m)
    GO.evaluate(outs, dict(zip(leaves, arrs)))


def test_runtime_flag_table():
    """Every settings.runtime flag the planner reads goes through graph._runtime, whose table holds the defaults the
    call sites carried before there was a table."""
    with open(G.__file__) as f:
        src = f.read()
    used = re.findall(r'_runtime\("(\w+)"\)', src)
    assert len(used) == src.count("_runtime(") - 1 == 11          # (every call names its flag literally; one is the def)
    assert set(used) == set(G._RUNTIME_DEFAULTS)
    assert src.count("_settings.runtime") == 1 and not re.search(r"^\s+from \._settings import", src, re.M)
    assert G._RUNTIME_DEFAULTS == {
        "fuse_elementwise": True, "column_programs": True, "head_in_contraction": True, "head_in_decoder": True,
        "side_jobs": True, "serial_chains": True, "fused_encoder": True, "fold_gram": True, "fused_predict": True,
        "early_forward": False, "gram_vjp_in_product": False}
    cfg = hb.settings.get_settings()
    for name, default in G._RUNTIME_DEFAULTS.items():
        if hasattr(cfg.runtime, name):
            delattr(cfg.runtime, name)
    with hb.settings.temp_settings(cfg):
        assert {k: G._runtime(k) for k in G._RUNTIME_DEFAULTS} == G._RUNTIME_DEFAULTS       # unnamed: the default
        for name, default in G._RUNTIME_DEFAULTS.items():
            setattr(cfg.runtime, name, not default)
            assert G._runtime(name) is (not default)                                        # named: the setting
