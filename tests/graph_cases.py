"""TEST INFRASTRUCTURE: the graphs the planner tests run, shared by the CPU half (tests/test_graph_lowering_cpu.py:
every graph traces, differentiates and evaluates) and the device half (tests/test_graph_device_gpu.py: every graph goes
through tests/graph_device.py).

CATALOGUE  : one small graph per op and attribute combination -- every `_check_vjp` case of tests/test_graph_cpu.py and
             the ops that otherwise reach the device in no test or in one model-specific shape.
generated  : `generated(seed)` draws a graph of at most GEN_MAX_NODES ops over a fixed set of leaf shapes.  It only
             builds what traces (operands are chosen by shape; no tracing error is caught anywhere) and keeps the
             operands of log / sqrt / div positive by construction (square(x) + 0.5).
"""
from collections import namedtuple

import numpy as np

import henbun_amd as hb
from henbun_amd import graph as G

tf = hb.tf

Case = namedtuple("Case", "name build shapes positive kinds")


def case(name, build, shapes, positive=False, kinds=None):
    return Case(name, build, [tuple(s) for s in shapes], positive, kinds)


def trace_graph(build, leaves, rng, weighted=True):
    """y = build(*leaves) (a builder may return (y, extra outputs...)), loss = reduce_sum(y * w) with w drawn from `rng`,
    and the gradient of the loss with respect to every leaf: (y, loss, gradients, [y, loss] + extras + gradients)."""
    res = build(*leaves)
    extras = [G.as_tensor(t) for t in res[1:]] if isinstance(res, (tuple, list)) else []
    y = G.as_tensor(res[0] if isinstance(res, (tuple, list)) else res)
    if weighted:
        w = rng.randn(*y.shape) if y.shape else rng.randn()
        loss = G.reduce_sum(G.mul(y, G.constant(w)))
    elif weighted is None:
        loss = G.reshape(y, [])       # a one-element y IS the objective (what Optimizer._trace does with a model's)
    else:
        loss = G.reduce_sum(y)
    grads = G.gradients(loss, list(leaves))
    return y, loss, grads, [y, loss] + extras + [g for g in grads if g is not None]


def _spd_chol(a):
    return G.cholesky(G.add_eye(G.matmul(a, a, transpose_b=True), 2.0))


def _halves(x):
    return G.unary("EXP", x[:, 3:]) * 2.0 + G.unary("TANH", x[:, :3])


def _col_softmax(x):
    e = G.unary("EXP", x - G.reduce_max(x, 0, keepdims=True))
    return e / G.reduce_sum(e, 0, keepdims=True)


def _concat_of_two_programs(x):
    return G.concat([G.unary("EXP", x) * 0.5, G.unary("TANH", x) + 1.0], 1)


CATALOGUE = [
    # ---- tests/test_graph_cpu.py::test_vjp_shape_ops
    case("transpose_201", lambda x: G.transpose(x, [2, 0, 1]), [(2, 3, 4)]),
    case("slice_ellipsis", lambda x: x[1:, ..., :2], [(3, 2, 4)]),
    case("getitem_row", lambda x: x[0], [(3, 4)]),
    case("concat_axis1", lambda x, y: G.concat([x, y], 1), [(2, 3), (2, 5)]),
    case("stack_last", lambda x, y: G.stack([x, y], -1), [(2, 3), (2, 3)]),
    case("tile_2x2", lambda x: G.tile(x, [2, 3]), [(2, 2)]),
    case("broadcast_3d", lambda x: G.broadcast_to(x, [4, 3, 5]), [(3, 1)]),
    case("expand_squeeze", lambda x: G.expand_dims(G.squeeze(x, 1), 0), [(3, 1, 2)]),
    case("diag_part", lambda x: G.diag_part(x), [(2, 4, 4)]),
    # ---- ::test_vjp_slices_that_tile_their_source_pack_into_a_concat
    case("halves_into_concat", _halves, [(5, 6)]),
    case("three_slices_out_of_order",
         lambda x: G.reduce_sum(x[:, 4:] * 3.0, 1) + G.reduce_sum(x[:, :1], 1) * G.reduce_sum(G.unary("EXP", x[:, 1:4]), 1), [(4, 6)]),
    case("partial_cover", lambda x: G.reduce_sum(x[:, :2] * 2.0, 1) + G.reduce_sum(x[:, 3:] * 3.0, 1), [(4, 6)]),
    # ---- ::test_mlp_backward_fuses_the_activation_gradient_into_the_dx_gemm
] + [
    case("mlp_actgrad_" + act, lambda x, w1, b1, w2, act=act: G.matmul(G.matmul(x, w1, bias=b1, act=act), w2),
         [(7, 4), (4, 5), (1, 5), (5, 3)]) for act in ("sigmoid", "tanh", "relu")
] + [
    # ---- ::test_vjp_reductions_and_broadcast
    case("reduce_sum_02", lambda x: G.reduce_sum(x, [0, 2]), [(3, 4, 5)]),
    case("reduce_sum_keepdims", lambda x: G.reduce_sum(x, 1, keepdims=True), [(3, 4, 5)]),
    case("reduce_mean_all", lambda x: G.reduce_mean(x), [(3, 4)]),
    case("reduce_max_last", lambda x: G.reduce_max(x, -1), [(3, 4)]),
    case("broadcast_arith", lambda x, y: x * y + x / y - y, [(3, 1, 4), (2, 1)], positive=True),
    case("log_sum_exp_mid", lambda x: hb.tf_wraps.log_sum_exp(x, 1), [(3, 4, 2)]),
    case("max_min", lambda x, y: tf.maximum(x, y) + tf.minimum(x, y) * 2.0, [(3, 4), (4,)]),
    # ---- ::test_vjp_elementwise
] + [
    case("unary_" + f, lambda x, f=f: G.unary(f, x), [(3, 4)]) for f in ("EXP", "SQUARE", "SIGMOID", "TANH", "SOFTPLUS", "NEG", "ABS", "RELU")
] + [
    case("unary_" + f, lambda x, f=f: G.unary(f, x), [(3, 4)], positive=True) for f in ("LOG", "SQRT", "RECIP", "RSQRT", "LGAMMA", "LOG1P")
] + [
    case("powc_recip_affine", lambda x: x ** 3.0 + 2.0 / x - (1.5 - x), [(5,)], positive=True),
    case("gaussian_broadcast", lambda x, mu, v: hb.densities.gaussian(x, mu, v), [(4, 1), (1, 3), (1,)], positive=True),
    case("student_t", lambda x, mu, s: hb.densities.student_t(x, mu, s, 3.0), [(4, 3), (3,), (1,)], positive=True),
    case("clip_by_value", lambda x: tf.clip_by_value(x, -0.5, 0.5), [(4, 4)]),
    # ---- ::test_vjp_linalg
    case("matmul", lambda a, b: G.matmul(a, b), [(3, 4), (4, 5)]),
    case("matmul_tt", lambda a, b: G.matmul(a, b, transpose_a=True, transpose_b=True), [(4, 3), (5, 4)]),
    case("matmul_batched_left", lambda a, b: G.matmul(a, b), [(2, 3, 4), (4, 5)]),
    case("matmul_batched_right_t", lambda a, b: G.matmul(a, b, transpose_b=True), [(3, 4), (2, 5, 4)]),
    case("matmul_batched_bias_sigmoid", lambda a, b, c: G.matmul(a, b, bias=c, act="sigmoid"), [(2, 3, 4), (2, 4, 5), (2, 1, 5)]),
    case("matmul_bias_relu", lambda a, b, c: G.matmul(a, b, bias=c, act="relu"), [(6, 4), (4, 5), (5,)]),
    case("band_part", lambda a: G.band_part(a, -1, 0), [(2, 4, 4)]),
    case("cholesky", _spd_chol, [(4, 4)]),
    case("cholesky_batched", _spd_chol, [(2, 3, 3)]),
    case("trinv", lambda a: G.trinv(_spd_chol(a)), [(4, 4)]),
    case("triangular_solve", lambda a, b: G.triangular_solve(_spd_chol(a), b), [(4, 4), (4, 3)]),
    case("gram_rbf", lambda x, x2, l: G.gram(x, x2, l, "rbf"), [(5, 2), (4, 2), (2,)], positive=True),
    case("gram_csym_rbf", lambda x, l: G.gram(x, x, l, "csym_rbf"), [(3, 5, 2), (1,)], positive=True),
    case("gram_sqdist", lambda x, x2, l: G.gram(x, x2, l, "sqdist"), [(3, 5, 2), (4, 2), (1,)], positive=True),
    # ---- ops that reach the device in no other test, or in one model-specific shape
    case("where_2d", lambda x, y: G.where(G.binary("GT", x, y), x * 2.0, y - 1.0), [(3, 4), (3, 4)]),
    case("where_broadcast", lambda x, y: G.where(G.binary("GT", x, y), x * 2.0, y - 1.0), [(3, 4), (4,)]),
    case("tile_2x5", lambda x: G.tile(x, [2, 3]), [(2, 5)]),
    case("stack_axis1", lambda x, y: G.stack([x, y], 1), [(2, 3), (2, 3)]),
    case("matrix_diag", lambda x: G.matrix_diag(x), [(2, 4)]),
    case("triangular_solve_adjoint", lambda a, b: G.triangular_solve(_spd_chol(a), b, adjoint=True), [(4, 4), (4, 3)]),
    case("reduce_mean_middle", lambda x: G.reduce_mean(x, 1), [(3, 5, 7)]),
    case("reduce_max_axis0_wide", lambda x: G.reduce_max(x, 0), [(3, 600)]),
    case("column_softmax", _col_softmax, [(4, 600)]),
    case("stop_gradient_times_x", lambda x: G.stop_gradient(x) * x, [(3, 4)]),
    case("matmul_broadcast_batch", lambda a, b: G.matmul(G.broadcast_to(a, [2, 3, 4]), b), [(3, 4), (2, 4, 5)]),
    case("concat_programs_in_place", _concat_of_two_programs, [(1, 6)]),
    case("concat_programs_copied", _concat_of_two_programs, [(4, 6)]),
    case("pow_tensor", lambda x, y: tf.pow(x, y), [(3, 4), (4,)], positive=True),
    case("log_sum_exp_axis1", lambda x: hb.tf_wraps.log_sum_exp(x, 1), [(3, 4)]),
    case("vec_to_tri", lambda v: G.vec_to_tri(v), [(2, 10)]),
    case("tri_to_vec", lambda t: G.tri_to_vec(t), [(2, 4, 4)]),
]

assert len({c.name for c in CATALOGUE}) == len(CATALOGUE)

# the modes every catalogue graph runs in; the two that only differ in HOW the same plan is launched (no chains,
# captured) run on this subset, which holds one graph of each kind of step a chain or a captured graph can contain
LAUNCH_MODE_SUBSET = ("halves_into_concat", "three_slices_out_of_order", "mlp_actgrad_sigmoid", "log_sum_exp_mid", "student_t",
                      "cholesky_batched", "triangular_solve", "gram_rbf", "where_broadcast", "matrix_diag", "column_softmax",
                      "matmul_broadcast_batch", "concat_programs_in_place", "concat_programs_copied", "vec_to_tri")
assert set(LAUNCH_MODE_SUBSET) <= {c.name for c in CATALOGUE}


# ------------------------------------------------------------------------------
# generated graphs
# ------------------------------------------------------------------------------
GEN_SEEDS = tuple(range(32))
GEN_MAX_NODES = 12
GEN_LEAF_SHAPES = ((4, 6), (6,), (1, 6), (4, 1), (2, 600))
_UNARY = ("TANH", "SIGMOID", "SOFTPLUS", "NEG", "ABS", "RELU", "LOG+", "SQRT+")
_BINARY = ("ADD", "SUB", "MUL", "MAX", "MIN", "DIV+")


def _positive(x):
    return G.square(x) + 0.5


def _broadcastable(a, b):
    try:
        np.broadcast_shapes(a, b)
        return True
    except ValueError:
        return False


class _Gen:
    """Draws ops until the budget is spent.  `pool`: every value so far; `sinks`: the ones nothing reads yet -- operands
    come from the sinks first, so that the graph stays one piece and every leaf reaches the result."""

    def __init__(self, rng, leaves):
        self.rng, self.pool, self.sinks = rng, list(leaves), list(leaves)

    def pick(self, ok):
        c = [t for t in self.sinks if ok(t)] or [t for t in self.pool if ok(t)]
        return c[self.rng.randint(len(c))] if c else None

    def emit(self, t, used, cost=None):
        for u in used:
            if u in self.sinks:
                self.sinks.remove(u)
        self.pool.append(t)
        self.sinks.append(t)

    def closed(self):
        """The loose ends joined into one result: added where they broadcast, else summed first."""
        out = self.sinks[0]
        for t in self.sinks[1:]:
            out = G.add(out, t) if _broadcastable(t.shape, out.shape) else G.add(out, G.reduce_sum(t))
        return out

    # every method returns False when its operands do not exist in the pool (nothing is built then)
    def unary(self):
        x = self.pick(lambda t: True)
        f = _UNARY[self.rng.randint(len(_UNARY))]
        if f.endswith("+"):
            self.emit(G.unary(f[:-1], _positive(x)), [x], 3)
        else:
            self.emit(G.unary(f, x), [x], 1)
        return True

    def binary(self):
        a = self.pick(lambda t: True)
        b = self.pick(lambda t: t is not a and _broadcastable(t.shape, a.shape))
        if b is None:
            return False
        f = _BINARY[self.rng.randint(len(_BINARY))]
        if f == "DIV+":
            self.emit(G.div(a, _positive(b)), [a, b], 3)
        elif f == "MUL":
            self.emit(G.mul(a, G.unary("SIGMOID", b)), [a, b], 2)     # (bounded factor: products do not compound)
        else:
            self.emit(G.binary(f, a, b), [a, b], 1)
        return True

    def where(self):
        a = self.pick(lambda t: True)
        b = self.pick(lambda t: t is not a and _broadcastable(t.shape, a.shape))
        if b is None:
            return False
        self.emit(G.where(G.binary("GT", a, b), G.unary("TANH", a), b), [a, b], 3)
        return True

    def slice(self):
        x = self.pick(lambda t: len(t.shape) >= 1 and t.shape[-1] >= 2)
        if x is None:
            return False
        d = x.shape[-1]
        lo = self.rng.randint(0, d - 1)
        hi = self.rng.randint(lo + 1, d + 1)
        if (lo, hi) == (0, d):
            hi = d - 1
        self.emit(x[..., lo:hi], [x], 1)
        return True

    def transpose(self):
        x = self.pick(lambda t: len(t.shape) == 2)
        if x is None:
            return False
        self.emit(G.transpose(x, [1, 0]), [x], 1)
        return True

    def concat(self):
        a = self.pick(lambda t: len(t.shape) >= 1)
        if a is None:
            return False
        ax = self.rng.randint(len(a.shape))
        same = lambda t: (t is not a and len(t.shape) == len(a.shape)
                          and all(p == q for i, (p, q) in enumerate(zip(t.shape, a.shape)) if i != ax))
        b = self.pick(same)
        if b is None:
            b, cost, used = G.unary("TANH", a), 2, [a]
        else:
            cost, used = 1, [a, b]
        self.emit(G.concat([a, b], ax), used, cost)
        return True

    def broadcast(self):
        x = self.pick(lambda t: tuple(t.shape) in ((6,), (1, 6), (4, 1)))
        if x is None:
            return False
        self.emit(G.broadcast_to(x, [4, 6]), [x], 1)
        return True

    def reduce(self):
        x = self.pick(lambda t: len(t.shape) >= 1 and t.size > 1)
        if x is None:
            return False
        f = G.reduce_sum if self.rng.randint(2) else G.reduce_max
        ax = self.rng.randint(len(x.shape) + 1)
        self.emit(f(x) if ax == len(x.shape) else f(x, ax), [x], 1)
        return True

    def reshape(self):
        x = self.pick(lambda t: len(t.shape) == 2 and t.shape[0] > 1 and t.shape[1] > 1)
        if x is None:
            return False
        r, c = x.shape
        self.emit(G.reshape(x, [r * c] if self.rng.randint(2) else [c, r]), [x], 1)
        return True

    def matmul(self):
        a = self.pick(lambda t: len(t.shape) == 2 and t.size <= 36)
        if a is None:
            return False
        b = self.pick(lambda t: t is not a and len(t.shape) == 2 and t.size <= 36 and (t.shape[0] == a.shape[1] or t.shape[1] == a.shape[1]))
        if b is None:
            self.emit(G.matmul(a, G.unary("TANH", a), transpose_b=True), [a], 2)
        else:
            self.emit(G.matmul(a, b, transpose_b=b.shape[0] != a.shape[1]), [a, b], 1)
        return True


_GEN_OPS = ("unary", "unary", "binary", "binary", "binary", "where", "slice", "transpose", "concat", "broadcast", "reduce", "reshape", "matmul")


def generated(seed):
    """(build, shapes): build(*leaves) traces the graph of `seed`; the same seed always gives the same graph."""
    rng = np.random.RandomState(1000 + seed)
    k = 2 + rng.randint(2)
    shapes = [GEN_LEAF_SHAPES[i] for i in rng.choice(len(GEN_LEAF_SHAPES), k, replace=False)]
    child = rng.randint(1 << 30)

    def build(*leaves):
        r = np.random.RandomState(child)
        g = _Gen(r, leaves)
        out = g.closed()
        for _ in range(64):
            # one more op, kept while the joined result stays within the budget (a graph node that is not kept is
            # reachable from nothing)
            pool, sinks = list(g.pool), list(g.sinks)
            if not getattr(g, _GEN_OPS[r.randint(len(_GEN_OPS))])():
                continue
            nxt = g.closed()
            if op_count(nxt) > GEN_MAX_NODES:
                g.pool, g.sinks = pool, sinks
                break
            out = nxt
        return out

    return build, shapes


def op_count(y):
    """Ops of a traced graph: its nodes that are neither leaves nor reshapes (views: no launch)."""
    return sum(1 for n in G.topo_order([y]) if not n.op.startswith("leaf:") and n.op != "reshape")
