"""TEST INFRASTRUCTURE: one minimal graph per planner pass on which the pass fires, and neighbours on which it must
decline (henbun_amd.graph: the graph-only matchers _match_gauss_ll_tails, _match_concat_placement and _match_colsum that
Plan.__init__ runs, cluster_elementwise, cluster_columns and the lazy forms of the emit functions).

PASSES[name] is a Spec: the builder, its leaf shapes, and `check(plan, tr)`, which asserts FROM THE PLAN (plan.explain,
step labels, plan._place, plan._lazy_cols, plan._colsum_of, plan._gll_post, buffer sizes) that the pass did what the
name says -- so that a planner change cannot leave the test passing while it tests something else.  PURE[name] asserts
the part of the same expectation that the graph-only functions decide alone, from (order, elementwise clusters, column
clusters, y, Pure): `pure_decisions` computes those without a plan, `plan_decisions` reads them off a plan.  The CPU suite
runs the PURE half (tests/test_graph_lowering_cpu.py), the device suite runs both and then sends the values through
tests/graph_device.py.
"""
from collections import namedtuple

import numpy as np

import henbun_amd as hb
from henbun_amd import graph as G

Spec = namedtuple("Spec", "name build shapes positive kinds runtime weighted check")
PASSES = {}
PURE = {}


Pure = namedtuple("Pure", "tails absorbed colsum fused_colsum place notes")


def pure_decisions(order, outputs, column_programs=True):
    """(elementwise clusters, column clusters, Pure): what the graph-only functions of henbun_amd.graph decide for this
    graph, called in Plan.__init__'s order with its defaults (compiled programs, nothing bound); no plan, no device."""
    consumers = G.consumer_map(order)
    tails, absorbed, notes = G._match_gauss_ll_tails(order, consumers, set(outputs))
    col = G.cluster_columns(order, outputs=outputs, skip=absorbed, enabled=column_programs)
    ew = G.cluster_elementwise(order, max_elems=G.EW_CLUSTER_MAX_ELEMS_JIT, skip=set(col) | absorbed)
    place = G._match_concat_placement(order, consumers, col, outputs, ())
    colsum, fused_colsum, more = G._match_colsum(order, consumers, ew)
    return ew, col, Pure(tails, absorbed, colsum, fused_colsum, place, notes + more)


def plan_decisions(plan):
    """The same record read off a plan (its ledger entries carry the node's label where the matchers' carry the node)."""
    return Pure(plan._gll_post, plan._absorbed, plan._colsum_of, plan._fused_colsum, plan._place, plan.explain)


def spec(name, build, shapes, check, positive=False, kinds=None, runtime=None, weighted=True, pure=None):
    assert name not in PASSES
    PASSES[name] = Spec(name, build, [tuple(s) for s in shapes], positive, kinds, runtime or {}, weighted, check)
    if pure is not None:
        PURE[name] = pure


# ---- helpers -------------------------------------------------------------------------------------------------------
def ancestors(y):
    return G.topo_order([y])


def fwd_nodes(y, op, f=None):
    """Nodes of the FORWARD graph (what the builder traced) with this op (and elementwise function)."""
    return [n for n in ancestors(y) if n.op == op and (f is None or n.attrs.get("f") == f)]


def one(nodes):
    assert len(nodes) == 1, nodes
    return nodes[0]


def step_labels(plan):
    plan.fuse_chains()
    out = []
    for s in plan.steps:
        for m in plan.chain_members.get(id(s), [s]):
            out.append(plan.step_labels.get(id(m), "other"))
    return out


def multi(c):
    return c is not None and len(c.nodes) >= 2


def fused_fwd(plan):
    return plan._clusters  # {node id: cluster}: clusters of >= 2 nodes become one program


def launched_alone(plan, node):
    """The node got a launch of its own (it is not inside a fused program)."""
    c = plan._clusters.get(node.id)
    return node.id not in plan._colclusters and not multi(c)


# ---- elementwise clusters ------------------------------------------------------------------------------------------
def _chain(x):
    return G.unary("TANH", G.unary("EXP", x) * 0.5)


def _pure_chain(order, ew, col, y, m=None):
    c = ew.get(y.node.id)
    assert multi(c) and ew.get(one(fwd_nodes(y, "ew", "EXP")).id) is c


def _check_chain(plan, tr):
    _pure_chain(None, plan._clusters, None, tr.y)
    assert any(l.startswith("ew_cluster[") for l in step_labels(plan))
    assert not any(l in ("ew:EXP", "ew:TANH") for l in step_labels(plan))


spec("ew_chain_fires", _chain, [(3, 4)], _check_chain, pure=_pure_chain)


def _sum13(*xs):
    t = G.unary("TANH", xs[0])
    for x in xs[1:]:
        t = t + G.unary("TANH", x)
    return t


def _ext_inputs(c, ew):
    return {t for m in c.nodes for t in m.inputs if ew.get(t.node.id) is not c}


def _pure_many_in(order, ew, col, y, m=None):
    assert G.EW_CLUSTER_MAX_IN == 12
    cl = {id(c): c for c in ew.values()}.values()
    assert all(len(_ext_inputs(c, ew)) <= G.EW_CLUSTER_MAX_IN for c in cl)
    tanhs = fwd_nodes(y, "ew", "TANH")
    assert len(tanhs) == 13 and len({id(ew[n.id]) for n in tanhs}) >= 2     # the thirteenth operand opened a new program


def _check_many_in(plan, tr):
    _pure_many_in(None, plan._clusters, None, tr.y)


spec("ew_more_than_12_operands_splits", _sum13, [(3, 4)] * 13, _check_many_in, pure=_pure_many_in, kinds=["data"] * 13)

_SEVEN = ("EXP", "TANH", "SIGMOID", "SOFTPLUS", "SQUARE", "ABS", "NEG")


def _seven_outputs(x):
    return G.concat([G.unary(f, x) for f in _SEVEN], 0)


def _pure_seven(order, ew, col, y, m=None):
    assert G.EW_CLUSTER_MAX_OUT == 6
    parts = [t.node for t in y.node.inputs]
    c = ew[parts[0].id]
    assert all(ew[p.id] is c for p in parts)          # the clustering keeps a margin only: seven results in one cluster


def _check_seven(plan, tr):
    _pure_seven(None, plan._clusters, None, tr.y)
    # ... which _emit_cluster cannot turn into one program (more than six values read outside): one launch per node
    labs = step_labels(plan)
    for f in _SEVEN:
        assert "ew:" + f in labs, (f, labs)


spec("ew_seven_results_fall_back_to_one_launch_per_node", _seven_outputs, [(3, 4)], _check_seven, pure=_pure_seven)


def _long_chain(x):
    t = x
    for i in range(50):
        t = G.unary("TANH" if i % 2 else "SIGMOID", t)
    return t


def _pure_long(order, ew, col, y, m=None):
    # EW_CLUSTER_MAX_INSTR (44) is never the limit that binds: the margin on results, 4 * EW_CLUSTER_MAX_OUT = 24 nodes,
    # closes a cluster first.  A 50-op chain therefore splits at 24 nodes, and no cluster passes either limit.
    assert G.EW_CLUSTER_MAX_INSTR == 44 and 4 * G.EW_CLUSTER_MAX_OUT == 24
    cl = {id(c): c for c in ew.values()}.values()
    assert all(c.ninstr <= G.EW_CLUSTER_MAX_INSTR and len(c.nodes) <= 24 for c in cl)
    chain = [n for n in ancestors(y) if n.op == "ew"]
    assert len(chain) == 50 and len({id(ew[n.id]) for n in chain}) >= 3 and max(len(c.nodes) for c in cl) == 24


def _check_long(plan, tr):
    _pure_long(None, plan._clusters, None, tr.y)
    labs = step_labels(plan)
    # every forward value is read again by the backward pass: 24 results are more than one program writes, so the
    # forward clusters run as one launch per node
    assert labs.count("ew:TANH") + labs.count("ew:SIGMOID") >= 24


spec("ew_chain_of_50_ops_splits_at_24_nodes", _long_chain, [(3, 4)], _check_long, pure=_pure_long)


def _outer(x, y):
    return G.unary("TANH", x) + G.unary("SIGMOID", y)


def _pure_outer(order, ew, col, y, m=None):
    assert G._merge_space((3, 1), (1, 4)) is None and G._merge_space((3, 1), (3, 4)) == (3, 4)
    a, b = one(fwd_nodes(y, "ew", "TANH")), one(fwd_nodes(y, "ew", "SIGMOID"))
    assert ew[a.id] is not ew[b.id]


def _check_outer(plan, tr):
    _pure_outer(None, plan._clusters, None, tr.y)


spec("ew_outer_product_spaces_do_not_merge", _outer, [(3, 1), (1, 4)], _check_outer, pure=_pure_outer)


def _sealed(x):
    a = G.unary("EXP", x) * 0.5
    m = G.reduce_max(a, 1, keepdims=True)
    return G.unary("TANH", a * m) + 1.0       # (reads the maximum: it cannot be ordered before the reduction)


def _pure_sealed(order, ew, col, y, m=None):
    a = one(fwd_nodes(y, "ew", "EXP"))
    b = one(fwd_nodes(y, "ew", "TANH"))
    ca, cb = ew[a.id], ew[b.id]
    assert multi(ca) and ca.sealed and cb is not ca and multi(cb)
    mul = one(fwd_nodes(y, "ew", "MUL"))
    assert ew[mul.id] is cb and any(ew.get(t.node.id) is ca for t in mul.inputs)     # read from memory, not from a register


def _check_sealed(plan, tr):
    _pure_sealed(None, plan._clusters, None, tr.y)
    labs = step_labels(plan)
    i = [k for k, l in enumerate(labs) if l.startswith("ew_cluster[")]
    assert len(i) >= 2 and "reduce" in labs[i[0]:i[-1]]      # a program, the reduction that sealed it, a later program


spec("ew_sealed_cluster_then_a_new_program", _sealed, [(3, 4)], _check_sealed, pure=_pure_sealed)


# ---- full sums absorbed into a program -----------------------------------------------------------------------------
def _fullsum(x):
    return G.reduce_sum(G.unary("TANH", x) * 2.0)


def _pure_fullsum(fires):
    def pure(order, ew, col, y, m=None):
        assert G.EW_REDUCE_MAX_ELEMS == 512
        r = one(fwd_nodes(y, "reduce"))
        c = ew.get(r.id)
        if fires:
            assert c is not None and r.outputs[0] in c.reduced and c is ew[one(fwd_nodes(y, "ew", "TANH")).id]
        else:
            assert c is None
    return pure


def _check_fullsum(fires):
    def check(plan, tr):
        _pure_fullsum(fires)(None, plan._clusters, None, tr.y)
        # (the gradient graph holds no reduction: its incoming gradient is one element, broadcast)
        assert ("reduce" in step_labels(plan)) == (not fires)
    return check


spec("fullsum_of_512_elements_is_absorbed", _fullsum, [(2, 256)], _check_fullsum(True), pure=_pure_fullsum(True))
spec("fullsum_of_513_elements_is_a_launch", _fullsum, [(3, 171)], _check_fullsum(False), pure=_pure_fullsum(False))


def _four_sums(x):
    return G.concat([G.reduce_sum(G.unary(f, x), keepdims=True) for f in ("TANH", "SIGMOID", "EXP", "SOFTPLUS")], 1)


def _pure_four(order, ew, col, y, m=None):
    rs = [t.node for t in y.node.inputs]
    assert [r.op for r in rs] == ["reduce"] * 4
    inside = [r for r in rs if r.id in ew]
    assert len(inside) == 3                               # a program folds at most three sums; the fourth is a launch
    c = ew[inside[0].id]
    assert all(ew[r.id] is c for r in inside) and len(c.reduced) == 3
    assert all(ew[r.inputs[0].node.id] is c for r in rs)  # (all four summands come out of that one program)


def _check_four(plan, tr):
    _pure_four(None, plan._clusters, None, tr.y)
    assert step_labels(plan).count("reduce") >= 1


spec("fullsum_three_absorbed_and_a_fourth_launched", _four_sums, [(2, 8)], _check_four, pure=_pure_four)


def _sum_read_inside(x):
    t = G.unary("TANH", x)
    return t / G.reduce_sum(G.unary("EXP", t), keepdims=True)


def _pure_read_inside(order, ew, col, y, m=None):
    r = one(fwd_nodes(y, "reduce"))
    c = ew[r.id]
    assert r.outputs[0] in c.reduced and ew[y.node.id] is not c       # the division reads the complete sum: next program


def _check_read_inside(plan, tr):
    _pure_read_inside(None, plan._clusters, None, tr.y)


spec("fullsum_read_by_the_same_space_starts_a_new_program", _sum_read_inside, [(2, 8)], _check_read_inside, pure=_pure_read_inside)


# ---- column clusters -------------------------------------------------------------------------------------------------
def _softmax0(x):
    e = G.unary("EXP", x - G.reduce_max(x, 0, keepdims=True))
    return e / G.reduce_sum(e, 0, keepdims=True)


def _pure_col(fires):
    def pure(order, ew, col, y, m=None):
        assert (G.EW_COL_MAX_ROWS, G.EW_COL_MIN_COLS) == (8, 512)
        rs = fwd_nodes(y, "reduce")
        assert len(rs) == 2
        if fires:
            c = col[rs[0].id]
            assert col[rs[1].id] is c and col[y.node.id] is c
        else:
            assert not col
    return pure


def _check_col(fires):
    def check(plan, tr):
        _pure_col(fires)(None, None, plan._colclusters, tr.y)
        assert any(l.startswith("col_cluster[") for l in step_labels(plan)) == fires
    return check


spec("col_cluster_2_rows_512_columns", _softmax0, [(2, 512)], _check_col(True), pure=_pure_col(True))
spec("col_cluster_8_rows_512_columns", _softmax0, [(8, 512)], _check_col(True), pure=_pure_col(True))
spec("col_cluster_declines_511_columns", _softmax0, [(2, 511)], _check_col(False), pure=_pure_col(False))
spec("col_cluster_declines_9_rows", _softmax0, [(9, 512)], _check_col(False), pure=_pure_col(False))


def _check_col_off(plan, tr):
    assert not plan._colclusters and not any(l.startswith("col_cluster[") for l in step_labels(plan))
    assert G.cluster_columns(G.topo_order(tr.outputs), outputs=tr.outputs)      # (it would have formed one)


spec("col_cluster_switched_off", _softmax0, [(2, 512)], _check_col_off, runtime={"column_programs": False})


def _softmax_of_rows(x):
    return _softmax0(x[1:3])


def _softmax_of_rows_also_output(x):
    s = x[1:3]
    return _softmax0(s), s


def _pure_slice(in_place):
    def pure(order, ew, col, y, m=None):
        s = one(fwd_nodes(y, "strided"))
        assert G._col_strided_view(s, 2, 512) == ("full", 512, 512)
        assert col and (s.id in col) == in_place and y.node.id in col
    return pure


def _check_slice(in_place):
    def check(plan, tr):
        _pure_slice(in_place)(None, None, plan._colclusters, tr.y)
        # the forward slice is a copy launch exactly when it is not read in place (the gradient graph slices nothing)
        assert ("strided" in step_labels(plan)) == (not in_place)
    return check


spec("col_cluster_reads_a_row_block_in_place", _softmax_of_rows, [(4, 512)], _check_slice(True), pure=_pure_slice(True))
spec("col_cluster_row_block_that_is_an_output_is_copied", _softmax_of_rows_also_output, [(4, 512)], _check_slice(False),
     pure=_pure_slice(False))


# ---- lazy broadcast --------------------------------------------------------------------------------------------------
def _bcast_check(aliased):
    def check(plan, tr):
        b = one(fwd_nodes(tr.y, "bcast")).outputs[0]
        assert (plan.buf(b).numel() < b.size) == aliased
        assert plan.buf(b).numel() == (4 if aliased else 24)
    return check


spec("bcast_read_by_elementwise_ops_is_an_alias",
     lambda x, z: G.unary("TANH", G.broadcast_to(x, [4, 6])) * z + G.unary("EXP", G.broadcast_to(x, [4, 6])), [(4, 1), (4, 6)],
     _bcast_check(True))
spec("bcast_read_by_a_product_is_materialised",
     lambda x, z: G.matmul(G.broadcast_to(x, [4, 6]), z) + G.reduce_sum(G.unary("TANH", G.broadcast_to(x, [4, 6]))), [(4, 1), (6, 3)],
     _bcast_check(False))
spec("bcast_read_by_a_reduction_is_materialised",
     lambda x, z: G.reduce_max(G.broadcast_to(x, [4, 6]) , 0) * G.reduce_sum(G.unary("TANH", G.broadcast_to(x, [4, 6])) * z, 0), [(4, 1), (4, 6)],
     _bcast_check(False))


def _bcast_output(x, z):
    b = G.broadcast_to(x, [4, 6])
    return G.unary("TANH", b) * z, b


spec("bcast_that_is_an_output_is_materialised", _bcast_output, [(4, 1), (4, 6)], _bcast_check(False))


# ---- concatenation in place --------------------------------------------------------------------------------------------
def _two_programs(x):
    return G.unary("EXP", x) * 0.5, G.unary("TANH", x) + 1.0


def _placed(plan, t):
    """The part is written into the concatenation's buffer."""
    if t not in plan._place:
        return False
    cat = [n for n in plan._order if n.op == "concat" and any(i is t or (i.node.op == "reshape" and i.node.inputs[0] is t) for i in n.inputs)]
    dst = plan.buf(cat[0].outputs[0])
    lo, hi = dst.data_ptr(), dst.data_ptr() + dst.numel() * dst.element_size()
    assert lo <= plan.buf(t).data_ptr() < hi
    return True


def _pure_concat(expect, first=False):
    """expect: for each part of the forward concat, whether it must be written in place."""
    def pure(order, ew, col, y, m):
        cat = _concat_first(y) if first else one(fwd_nodes(y, "concat"))
        got = [G._through(t) in m.place for t in cat.inputs]
        assert got == list(expect), got
    return pure


def _concat_check(expect):
    """expect: for each part of the forward concat, whether it must be written in place."""
    def check(plan, tr):
        _pure_concat(expect)(None, None, None, tr.y, plan_decisions(plan))
        cat = one(fwd_nodes(tr.y, "concat"))
        got = []
        for t in cat.inputs:
            while t.node.op == "reshape":
                t = t.node.inputs[0]
            got.append(_placed(plan, t))
        assert got == list(expect), got
    return check


def _concat_plain(x):
    a, b = _two_programs(x)
    return G.concat([a, b], 1)


def _concat_two_consumers(x):
    a, b = _two_programs(x)
    return G.concat([a, b], 1) * G.concat([G.unary("SIGMOID", a), G.unary("SIGMOID", a)], 1)


def _concat_first(y):
    """The concat of two different parts (the other one takes the same tensor twice)."""
    return one([n for n in fwd_nodes(y, "concat") if n.inputs[0] is not n.inputs[1]])


def _concat_check_first(expect):
    def check(plan, tr):
        _pure_concat(expect, first=True)(None, None, None, tr.y, plan_decisions(plan))
        cat = _concat_first(tr.y)
        assert [_placed(plan, t) for t in cat.inputs] == list(expect)
    return check


def _concat_also_output(x):
    a, b = _two_programs(x)
    return G.concat([a, b], 1), a


def _concat_twice(x):
    a, _ = _two_programs(x)
    return G.concat([a, a], 1)


def _concat_reshaped(x):
    a, b = _two_programs(x)
    return G.concat([G.reshape(a, [6]), G.reshape(b, [6])], 0)


def _concat_leaf(x):
    _, b = _two_programs(x)
    return G.concat([x, b], 1)


def concat_spec(name, build, shapes, expect, first=False):
    spec(name, build, shapes, (_concat_check_first if first else _concat_check)(expect), pure=_pure_concat(expect, first))


concat_spec("concat_parts_from_programs_are_written_in_place", _concat_plain, [(1, 6)], [True, True])
concat_spec("concat_part_with_two_consumers_is_copied", _concat_two_consumers, [(1, 6)], [False, True], first=True)
concat_spec("concat_part_that_is_an_output_is_copied", _concat_also_output, [(1, 6)], [False, True])
concat_spec("concat_of_the_same_tensor_twice_is_copied", _concat_twice, [(1, 6)], [False, False])
# (_match_concat_placement looks through reshapes -- they are views -- so a reshaped part IS written in place)
concat_spec("concat_part_behind_a_reshape_is_written_in_place", _concat_reshaped, [(1, 6)], [True, True])
concat_spec("concat_below_a_non_unit_leading_axis_is_copied", _concat_plain, [(4, 6)], [False, False])
concat_spec("concat_part_that_is_a_leaf_is_copied", _concat_leaf, [(1, 6)], [False, True])


# ---- weight + bias gradient from one pass (hb_matmul_colsum) ---------------------------------------------------------
def _colsum_fires(x, g):
    gm = G.unary("TANH", g)
    return G.matmul(x, gm, transpose_a=True) + G.reduce_sum(gm, 0, keepdims=True)


def _colsum_read_early(x, g):
    gm = G.unary("TANH", g)
    return G.unary("EXP", G.reduce_sum(gm, 0, keepdims=True)) + G.matmul(x, gm, transpose_a=True)


_X84 = np.random.RandomState(5).randn(8, 4)


def _colsum_in_cluster(g):
    # (X is a constant: its gradient would be a second product reading gm, ordered before the sum, which would close
    # gm's program before the sum could join it)
    gm = G.unary("TANH", g) * 2.0
    return G.matmul(G.constant(_X84), gm, transpose_a=True) + G.reduce_sum(gm, 0, keepdims=True)


def _pure_colsum(fires, why=None):
    def pure(order, ew, col, y, m):
        mm = one([n for n in fwd_nodes(y, "matmul") if n.attrs["ta"]])
        r = one(fwd_nodes(y, "reduce"))
        if fires:
            assert m.colsum.get(mm.id) is r and r.id in m.fused_colsum
            assert any(f for p, _, f, _ in m.notes if p.startswith("weight + bias gradient from one pass"))
        else:
            assert mm.id not in m.colsum and r.id not in m.fused_colsum
        if why == "cluster":
            assert multi(ew.get(r.id))
        if why == "early":
            pos = {n.id: i for i, n in enumerate(order)}
            assert any(pos[c.id] < pos[mm.id] for c in G.consumer_map(order)[r.outputs[0]])
    return pure


def _colsum_check(fires, why=None):
    def check(plan, tr):
        _pure_colsum(fires, why)(plan._order, plan._clusters, None, tr.y, plan_decisions(plan))
        if why == "early":
            mm = one([n for n in fwd_nodes(tr.y, "matmul") if n.attrs["ta"]])
            pos = plan._order_pos
            assert any(pos[c.id] < pos[mm.id] for c in plan._consumers[one(fwd_nodes(tr.y, "reduce")).outputs[0]])
    return check


def colsum_spec(name, build, shapes, fires, why=None):
    spec(name, build, shapes, _colsum_check(fires, why), pure=_pure_colsum(fires, why))


colsum_spec("colsum_rides_in_the_product", _colsum_fires, [(8, 4), (8, 5)], True)
colsum_spec("colsum_read_before_the_product_is_a_launch", _colsum_read_early, [(8, 4), (8, 5)], False, "early")
colsum_spec("colsum_inside_a_program_stays_there", _colsum_in_cluster, [(8, 1)], False, "cluster")


# ---- the likelihood head's elementwise tail (hb_gauss_ll_post) -------------------------------------------------------
_Y8 = np.random.RandomState(7).randn(8)


def _gll_tail(f, s, v):
    return G.reduce_sum(hb.densities.gaussian(G.constant(_Y8), f * s, v))


def _gll_tail_read_twice(yy, f, s, v):
    return G.reduce_sum(hb.densities.gaussian(yy, f * s, v))


def _pure_gll(fires):
    def pure(order, ew, col, y, m):
        head = one([n for n in order if n.op == "gauss_ll"])
        assert len(head.inputs) == 4                       # (the scale was recognised: the tail is scale * (post * dmu))
        assert (head.id in m.tails) == fires
        assert [f for p, _, f, _ in m.notes if p.startswith("likelihood head writes")] == [fires]
        if fires:
            assert len(m.tails[head.id][2]) == 2 and all(x.id in m.absorbed for x in m.tails[head.id][2])
    return pure


def _gll_check(fires):
    def check(plan, tr):
        _pure_gll(fires)(plan._order, None, None, tr.y, plan_decisions(plan))
    return check


spec("gauss_ll_writes_its_elementwise_tail", _gll_tail, [(8,), (1,), (1,)], _gll_check(True), positive=True, pure=_pure_gll(True))
spec("gauss_ll_tail_read_twice_stays_elementwise", _gll_tail_read_twice, [(8,), (8,), (1,), (1,)], _gll_check(False), positive=True,
     pure=_pure_gll(False))


# ---- lazy column block ---------------------------------------------------------------------------------------------------
_U = np.random.RandomState(11).randn(6, 3)


def _halves_into_sampler(o):
    x, kl, _ = G.diag_sample_kl(o[:, :3], o[:, 3:], u=G.constant(_U))
    return x + kl


def _halves_one_read_elementwise(o):
    s = o[:, 3:]
    x, kl, _ = G.diag_sample_kl(o[:, :3], s, u=G.constant(_U))
    return x + kl + G.unary("TANH", s)


def _lazy_check(expect_mu, expect_s):
    def check(plan, tr):
        skl = one(fwd_nodes(tr.y, "diag_sample_kl"))
        mu, s = skl.inputs[0], skl.inputs[1]
        assert mu.node.op == "strided" and s.node.op == "strided"
        assert [mu in plan._lazy_cols, s in plan._lazy_cols] == [expect_mu, expect_s]
        assert step_labels(plan).count("strided") == [expect_mu, expect_s].count(False)
    return check


spec("column_halves_feed_the_sampler_in_place", _halves_into_sampler, [(6, 6)], _lazy_check(True, True))
spec("column_half_also_read_elementwise_is_copied", _halves_one_read_elementwise, [(6, 6)], _lazy_check(True, False))


# ---- strided views that are reshapes; scatters ------------------------------------------------------------------------------
def _check_transpose_column(plan, tr):
    assert not fwd_nodes(tr.y, "strided") and "strided" not in step_labels(plan) and "scatter_strided" not in step_labels(plan)


def _check_transpose_true(plan, tr):
    assert len(fwd_nodes(tr.y, "strided")) == 1 and "strided" in step_labels(plan)
    sc = one([n for n in plan._order if n.op == "scatter_strided"])
    assert int(np.prod(sc.attrs["shape"])) == int(np.prod(sc.attrs["xshape"]))      # a full cover: written without a fill


def _check_partial_scatter(plan, tr):
    sc = one([n for n in plan._order if n.op == "scatter_strided"])
    assert int(np.prod(sc.attrs["shape"])) == 8 and int(np.prod(sc.attrs["xshape"])) == 24 and sc.attrs["offset"] == 1


spec("transpose_of_a_column_is_a_reshape", lambda x: G.unary("TANH", G.transpose(x, [1, 0])), [(5, 1)], _check_transpose_column,
     pure=lambda order, ew, col, y, m=None: _check_pure_no_strided(y))
spec("true_transpose_is_a_copy_and_its_gradient_a_full_scatter", lambda x: G.unary("TANH", G.transpose(x, [1, 0])), [(3, 4)],
     _check_transpose_true)
spec("slice_gradient_is_a_fill_and_a_partial_scatter", lambda x: G.unary("TANH", x[:, 1:3]), [(4, 6)], _check_partial_scatter)


def _check_pure_no_strided(y):
    assert not fwd_nodes(y, "strided") and one(fwd_nodes(y, "reshape")).outputs[0].shape == (1, 5)
