"""The elementwise op table on the device against the exact reference (tests/ew_ref.py, tests/golden/ew_table_ref.npz),
and the launch logic of the small plumbing kernels (hb_ewise, hb_copy_nd, hb_fill, hb_gather_rows, hb_matutil).

Every HB_EW_* op, in float32 and float64, through three forms that must each agree with the reference on their own:
H.ewise (ew_kernel), a one-instruction EwiseProgram interpreted (ew_prog_image_kernel), and the same program compiled
at run time (hb_ewise_jit_*).

  class A (NEG SQRT SQUARE ABS SIGN RELU RECIP RSQRT STEP AFFINE CLIP CLIPMASK COPY, ADD..EQ without POW, SIGMOID_GRAD
           TANH_GRAD RELU_GRAD CLIP_GRAD, WHERE FMA): bit-equal to the C expression evaluated by numpy in the dtype (one
           mpmath rounding for FMA AFFINE SQRT DIV) wherever the result is normal or zero.
  class B (EXP LOG SIGMOID SOFTPLUS TANH LGAMMA POWC LOG1P DIGAMMA POW SOFTPLUS_GRAD GAUSS_LOGPDF GAUSS_LOGPDF_GRAD):
           within the forward error bound that ew_ref.py derives point by point from the op's own operation sequence.
  both:    a non-finite reference is matched in kind and sign, a subnormal one within the smallest normal.
"""
import itertools

import numpy as np
import pytest
import torch

import ew_ref as R

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f64": torch.float64}
BIG = 2048 * 256 + 77     # one element more than the capped grid covers in a single trip, and then some


@pytest.fixture(scope="module")
def H():
    from henbun_amd import hip_ops

    assert torch.cuda.is_available()
    return hip_ops


@pytest.fixture(scope="module")
def table():
    return R.load_fixture()


def dev(a):
    return torch.from_numpy(np.asarray(a).copy()).cuda()       # (a C-ordered copy that keeps a 0-d array 0-d)


def _ewise_mode(mode):
    """settings override selecting the compiled (hiprtc) or the interpreted form of a fused elementwise program"""
    import henbun_amd as hb

    cfg = hb.settings.get_settings()
    cfg.runtime.ewise = mode
    return hb.settings.temp_settings(cfg)


def run_form(H, form, op, p, ins):
    """[nout, n] numpy result of `op` on 1-D device inputs through one of the three forms"""
    nin, nout, params, _ = R.OPS[op]
    n = ins[0].numel()
    if form == "ewise":
        out = H.ewise(op, ins, nout=nout, params=list(params))
        outs = list(out) if nout > 1 else [out]
    else:
        outs = [torch.empty(n, dtype=DT[p], device="cuda") for _ in range(nout)]
        pr = [float(v) for v in params] + [0.0, 0.0]
        if op == "GAUSS_LOGPDF_GRAD":
            pr[0] = 3.0      # the register of the 4th operand
        code = [[H.EW[op], nin, 0, min(1, nin - 1), min(2, nin - 1)]]
        with _ewise_mode(form):
            prog = H.EwiseProgram(code, [pr[:2]], ins, [[1]] * nin, outs, [nin + k for k in range(nout)], [[1]] * nout, [n])
        assert (prog.image is None) == (form == "jit")      # the form asked for is the one that runs
        prog.launch()
    torch.cuda.synchronize()
    return np.stack([o.cpu().numpy() for o in outs])


@pytest.mark.parametrize("form", ["ewise", "interpret", "jit"])
@pytest.mark.parametrize("p", ["f32", "f64"])
@pytest.mark.parametrize("op", list(R.OPS))
def test_op_against_the_exact_reference(H, table, op, p, form):
    ins = [dev(c) for c in table["%s/%s/in" % (p, op)]]
    tol = table["%s/%s/tol" % (p, op)] if R.OPS[op][3] == "B" else None
    got = run_form(H, form, op, p, ins)
    R.check(p, op, got, table["%s/%s/exp" % (p, op)], tol, "%s %s %s" % (op, p, form))


@pytest.mark.parametrize("p", ["f32", "f64"])
def test_nan_operands_do_what_the_c_expressions_do(H, p):
    """ew_apply writes MAX, MIN, CLIP and the comparisons as C conditionals; a comparison with a NaN is false, so

        MAX(NaN, b) = b      MAX(a, NaN) = NaN        (a > b ? a : b)
        MIN(NaN, b) = b      MIN(a, NaN) = NaN        (a < b ? a : b)
        CLIP(NaN) = NaN      CLIPMASK(NaN) = 0        RELU(NaN) = STEP(NaN) = SIGN(NaN) = 0
        GT GE LT LE EQ with a NaN on either side = 0
        WHERE(NaN, b, c) = b (NaN != 0)               RELU_GRAD(NaN, g) = CLIP_GRAD(NaN, g) = 0
        ABS(-0) = -0 (x < 0 ? -x : x)

    which is not what torch.maximum / minimum / clamp return (they propagate the NaN from either side)."""
    T = R.NP[p]
    nan = T(np.nan)
    a = dev(np.array([nan, 2.0, nan, -0.0], dtype=T))
    b = dev(np.array([3.0, nan, nan, 1.0], dtype=T))
    c = dev(np.array([7.0, 7.0, 7.0, 7.0], dtype=T))
    get = lambda op, ins, params=None: H.ewise(op, ins, params=params).cpu().numpy()
    U = np.uint32 if p == "f32" else np.uint64

    def eq(got, exp):
        exp = np.asarray(exp, dtype=T)
        m = ~np.isnan(exp)
        return np.array_equal(np.isnan(got), ~m) and np.array_equal(got[m].view(U), exp[m].view(U))

    assert eq(get("MAX", [a, b]), np.array([3.0, nan, nan, 1.0]))
    assert eq(get("MIN", [a, b]), np.array([3.0, nan, nan, -0.0]))
    assert eq(get("CLIP", [a], [-0.5, 0.7]), np.array([nan, 0.7, nan, -0.0]))
    assert eq(get("CLIPMASK", [a], [-0.5, 0.7]), np.array([0.0, 0.0, 0.0, 1.0]))
    for op in ("RELU", "STEP", "SIGN"):
        assert eq(get(op, [a])[[0, 2]], np.array([0.0, 0.0])), op
    for op in ("GT", "GE", "LT", "LE", "EQ"):
        assert eq(get(op, [a, b])[:3], np.array([0.0, 0.0, 0.0])), op
    assert eq(get("WHERE", [a, b, c]), np.array([3.0, nan, nan, 7.0]))
    assert eq(get("RELU_GRAD", [a, c])[[0, 2]], np.array([0.0, 0.0]))
    assert eq(get("CLIP_GRAD", [a, c], [-0.5, 0.7])[[0, 2]], np.array([0.0, 0.0]))
    assert eq(get("ABS", [a])[3:], np.array([-0.0]))


# ------------------------------------------------------------------------------------------------------ launch logic
def bits_equal(got, exp):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    return np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(exp).view(np.uint8))


@pytest.mark.parametrize("p", ["f32", "f64"])
def test_grid_stride_loops_take_a_second_trip(H, p):
    """hb_ewise, hb_copy_nd, hb_fill and hb_gather_rows cap the grid at 2048 x 256 threads and stride: BIG elements need
    the second trip.  FMA on small integers times small integers (the product is exact, so numpy's two steps round
    once like the fused one), WHERE, a strided copy, a fill and a gather."""
    T = R.NP[p]
    r = np.random.RandomState(3)
    a, b = r.randint(-1000, 1000, BIG).astype(T), r.randint(-1000, 1000, BIG).astype(T)
    c = r.randn(BIG).astype(T)
    assert bits_equal(H.ewise("FMA", [dev(a), dev(b), dev(c)]), a * b + c)
    m = (r.rand(BIG) < 0.5).astype(T)
    assert bits_equal(H.ewise("WHERE", [dev(m), dev(a), dev(c)]), np.where(m != 0, a, c))
    # 524365 = 5 * 104873: a transposing copy over the whole range, then a flat one
    src = c.reshape(5, BIG // 5)
    out = torch.empty(BIG // 5, 5, dtype=DT[p], device="cuda")
    H.copy_nd(dev(src), [1, BIG // 5], out, [5, 1], [BIG // 5, 5])
    assert bits_equal(out, np.ascontiguousarray(src.T))
    flat = torch.empty(BIG, dtype=DT[p], device="cuda")
    H.copy_nd(dev(c), [1], flat, [1], [BIG])
    assert bits_equal(flat, c)
    assert bits_equal(H.fill(torch.empty(BIG, dtype=DT[p], device="cuda"), 0.1), np.full(BIG, T(0.1)))
    n, row, nsrc = 4099, 129, 611           # n * row = 528771 > BIG
    tab = r.randn(nsrc, row).astype(T)
    idx, perm = r.randint(0, nsrc, n), r.permutation(nsrc)
    assert bits_equal(H.gather_rows(dev(tab), dev(idx), dev(perm)), tab[perm[idx]])
    assert bits_equal(H.gather_rows(dev(tab), dev(idx)), tab[idx])


EW_BROADCASTS = {
    "contiguous: every dim merges": [(4, 5, 6), (4, 5, 6), (4, 5, 6)],
    "[R,n] [1,n] [R,1]": [(7, 33), (1, 33), (7, 1)],
    "six dims, size-1 dims interleaved, nothing merges": [(3, 1, 4, 1, 5, 1), (1, 2, 1, 3, 1, 2), (3, 2, 1, 1, 5, 2)],
    "six dims of which the size-1 ones drop out and the rest merge": [(2, 1, 3, 1, 4, 1)] * 3,
    "operand 0 could merge dims 0 and 1, operand 1 could not": [(4, 5, 6), (4, 1, 6), (4, 5, 6)],
    "operand 1 could merge dims 1 and 2, operand 0 could not": [(4, 5, 1), (4, 5, 6), (1, 1, 6)],
    "a 0-d operand": [(7, 9), (), (7, 9)],
    "all operands 0-d": [(), (), ()],
}


@pytest.mark.parametrize("p", ["f32", "f64"])
@pytest.mark.parametrize("case", list(EW_BROADCASTS))
def test_ewise_broadcast_and_dim_merging(H, p, case):
    """hb_ewise drops size-1 dims and merges dim d into d-1 only when EVERY operand allows it"""
    T = R.NP[p]
    r = np.random.RandomState(7)
    shapes = EW_BROADCASTS[case]
    a, b, c = [np.asarray(r.randint(-50, 50, s) if k < 2 else r.standard_normal(s)).astype(T) for k, s in enumerate(shapes)]
    got = H.ewise("FMA", [dev(a), dev(b), dev(c)])       # integer factors: the product is exact
    assert bits_equal(got, np.asarray(a * b + c, dtype=T))
    got = H.ewise("SUB", [dev(a), dev(c)])
    assert bits_equal(got, np.asarray(a - c, dtype=T))


def _strides(shape):
    st, acc = [], 1
    for s in reversed(shape):
        st.insert(0, acc)
        acc *= s
    return st


@pytest.mark.parametrize("p", ["f32", "f64"])
def test_copy_nd_permutations_slices_broadcast_and_concat(H, p):
    T, dt = R.NP[p], DT[p]
    r = np.random.RandomState(9)
    cases = [((3, 4, 5), perm) for perm in itertools.permutations(range(3))]
    cases.append(((2, 3, 2, 3, 2, 3), (5, 3, 1, 4, 2, 0)))
    cases.append(((2, 1, 3, 1, 2, 5), (4, 5, 0, 1, 2, 3)))      # size-1 dims, and dims that merge after the permutation
    for shape, perm in cases:
        x = r.randn(*shape).astype(T)
        oshape = [shape[k] for k in perm]
        out = torch.empty(*oshape, dtype=dt, device="cuda")
        st = _strides(shape)
        H.copy_nd(dev(x), [st[k] for k in perm], out, _strides(oshape), oshape)
        assert bits_equal(out, np.ascontiguousarray(np.transpose(x, perm))), (shape, perm)
    # slice: x[1:3, 2:5] of a [4,6] into y[2:4, 1:4] of a [5,7]; everything else stays
    x, y = r.randn(4, 6).astype(T), r.randn(5, 7).astype(T)
    Y = dev(y)
    H.copy_nd(dev(x), [6, 1], Y, [7, 1], [2, 3], src_off=1 * 6 + 2, dst_off=2 * 7 + 1)
    exp = y.copy()
    exp[2:4, 1:4] = x[1:3, 2:5]
    assert bits_equal(Y, exp)
    # broadcast: a source stride of 0 repeats a row
    row = r.randn(33).astype(T)
    out = torch.empty(70, 33, dtype=dt, device="cuda")
    H.copy_nd(dev(row), [0, 1], out, [33, 1], [70, 33])
    assert bits_equal(out, np.broadcast_to(row, (70, 33)).copy())
    # concat placement: [5,3] and [5,4] side by side in a [5,7]
    u, v = r.randn(5, 3).astype(T), r.randn(5, 4).astype(T)
    out = torch.empty(5, 7, dtype=dt, device="cuda")
    H.copy_nd(dev(u), [3, 1], out, [7, 1], [5, 3])
    H.copy_nd(dev(v), [4, 1], out, [7, 1], [5, 4], dst_off=3)
    assert bits_equal(out, np.concatenate([u, v], axis=1))
    # 0-d and empty
    out = torch.zeros(1, dtype=dt, device="cuda")
    H.copy_nd(dev(row), [], out, [], [], src_off=4)
    assert bits_equal(out, row[4:5])
    H.copy_nd(dev(row), [1, 1], out, [1, 1], [0, 3])
    assert bits_equal(out, row[4:5])


def _matutil_ref(x, mode, lower, upper, alpha):
    T = x.dtype.type
    B, Rr, C = x.shape
    i, j = np.arange(Rr)[:, None], np.arange(C)[None, :]
    if mode == 0:
        keep = ((lower < 0) | (i - j <= lower)) & ((upper < 0) | (j - i <= upper))
        return np.where(keep[None], x, T(0))
    if mode == 1:
        return np.where((i == j)[None], x + T(alpha), x)
    if mode == 2:
        return np.where((i > j)[None], x, np.where((i == j)[None], T(0.5) * x, T(0)))
    xt = np.transpose(x, (0, 2, 1))
    if mode == 3:
        return T(0.5) * (x + xt)
    return T(0.5) * np.where((i >= j)[None], x, xt)


@pytest.mark.parametrize("p", ["f32", "f64"])
def test_matutil_every_mode_rectangular_banded_and_in_place(H, p):
    T = R.NP[p]
    r = np.random.RandomState(13)
    bands = [(-1, 0), (0, -1), (2, 1), (0, 0)]
    for B in (1, 3):
        for Rr, C in [(1, 1), (5, 5), (33, 70), (70, 33), (130, 130)]:
            x = r.randn(B, Rr, C).astype(T)
            jobs = [(0, lo, up, 0.0) for lo, up in bands] + [(1, -1, -1, 0.3), (2, -1, -1, 0.0)]
            if Rr == C:
                jobs += [(3, -1, -1, 0.0), (4, -1, -1, 0.0)]
            for mode, lo, up, alpha in jobs:
                exp = np.asarray(_matutil_ref(x, mode, lo, up, alpha), dtype=T)
                X = dev(x)
                got = H.matutil(X, mode, lower=lo, upper=up, alpha=alpha)
                assert bits_equal(got, exp), (B, Rr, C, mode, lo, up)
                assert bits_equal(X, x)          # out of place: the input stays
                if mode <= 2:
                    H.matutil(X, mode, lower=lo, upper=up, alpha=alpha, out=X)
                    assert bits_equal(X, exp), ("in place", B, Rr, C, mode, lo, up)
