"""The graph planner on the device against the CPU evaluator: the op catalogue and the generated graphs of
tests/graph_cases.py through the harness of tests/graph_device.py.

What is under test is henbun_amd.graph.Plan -- which kernel runs, on which buffer, in what order -- not the arithmetic of
the kernels (tests/test_kernels_gpu.py and the other kernel files hold those to exact references).  Every graph is
lowered with its gradient with respect to every leaf as ONE plan, in each execution mode of the planner, and each mode is
held to the float64 evaluator; modes are not compared with one another bit for bit (compiled, interpreted and per-op
forms may contract differently), a second run and a captured replay of the same plan are."""
import numpy as np
import pytest

import graph_cases as GC
import graph_device as GD

pytestmark = pytest.mark.gpu


def _traced(case, dtype):
    return GD.Traced(case.build, case.shapes, kinds=case.kinds, positive=case.positive, dtype=dtype)


@pytest.mark.parametrize("case", GC.CATALOGUE, ids=lambda c: c.name)
def test_catalogue_graph_in_every_mode(case):
    # float64: compiled, interpreted and one launch per node for every graph; the two modes that launch the SAME plan
    # differently (no serial chains, captured) on the subset named in graph_cases
    modes = GD.MODES if case.name in GC.LAUNCH_MODE_SUBSET else ("default", "interpret", "plain")
    GD.run_modes(_traced(case, "float64"), case.name, modes)
    # float32 (side jobs on): the default plan and the plain lowering, to 8 x the evaluator's own float32 error + 4 ulp
    GD.run_modes(_traced(case, "float32"), case.name, ("default", "plain"))
    print("graph_device programs compiled so far: %d" % GD.PROGRAMS["compiled"])


RAN = []


def _generated(seed):
    build, shapes = GC.generated(seed)
    tr = GD.Traced(build, shapes, seed=seed)
    assert all(g is not None for g in tr.grads)
    GD.run_modes(tr, "generated[%d]" % seed, ("default", "plain"))
    RAN.append(seed)


@pytest.mark.parametrize("seed", GC.GEN_SEEDS)
def test_generated_graph_default_and_plain(seed):
    _generated(seed)
    print("graph_device programs compiled so far: %d" % GD.PROGRAMS["compiled"])


def test_all_generated_graphs_ran():
    """No generated graph may drop out: 32 graphs, seeds 0..31, each run to the end (the seeds that the selection of
    this run left out are run here)."""
    for seed in GC.GEN_SEEDS:
        if seed not in RAN:
            _generated(seed)
    assert sorted(set(RAN)) == list(GC.GEN_SEEDS) and len(set(RAN)) == 32
