"""Exact reference for the elementwise op table (csrc/ew_apply.cuh, csrc/ew_math.cuh) and its input sets.

    python tests/ew_ref.py --write     regenerates tests/golden/ew_table_ref.npz

For every HB_EW_* op and for float32 and float64 the fixture holds a few hundred deterministic input points, the
expected output and, for the ops that go through the device math library, the allowed error at each point.

Two classes of op (the GPU test asserts them differently):

  class A   selects, compares and single IEEE operations.  Expected = the C expression of ew_apply evaluated step by
            step by numpy in the dtype (SEQ below); for FMA, AFFINE, SQRT and DIV = the mpmath value rounded once.
            Bit-equal wherever the result is normal or zero.
  class B   ops through the math library.  Expected = the mpmath value (EXACT below) of the op on the exact rational
            value of the dtype-rounded inputs, rounded once to the dtype.  Allowed error = the first-order forward
            error bound of the op's own operation sequence,
                sum_i |d out / d t_i| * |t_i| * u_i * eps          (eps = spacing of the dtype at 1)
            over the sequence's intermediates t_i, each taken from the exact evaluation: class Tracker below carries
            value and accumulated bound through the sequence (u_i = 0.5 for an IEEE operation, the documented bound for
            a math-library call), plus half an ulp for the rounding of the reference itself and, for DIGAMMA, the
            truncation error of its asymptotic series (|sequence in exact arithmetic - digamma|).

Points whose inputs are not finite, or lie outside the op's real domain, take their expected value from SEQ in the
dtype: those values are fixed by IEEE 754 / C Annex F (NaN, infinities, exact 0 or 1) and are compared by kind and sign,
finite ones exactly.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "ew_table_ref.npz")

NP = {"f32": np.float32, "f64": np.float64}

# op -> (number of inputs, number of outputs, params, class)
OPS = {
    "NEG": (1, 1, (), "A"), "EXP": (1, 1, (), "B"), "LOG": (1, 1, (), "B"), "SQRT": (1, 1, (), "A"),
    "SQUARE": (1, 1, (), "A"), "ABS": (1, 1, (), "A"), "SIGN": (1, 1, (), "A"), "SIGMOID": (1, 1, (), "B"),
    "RELU": (1, 1, (), "A"), "SOFTPLUS": (1, 1, (), "B"), "TANH": (1, 1, (), "B"), "RECIP": (1, 1, (), "A"),
    "RSQRT": (1, 1, (), "A"), "STEP": (1, 1, (), "A"), "AFFINE": (1, 1, (2.5, -1.0), "A"),
    "CLIP": (1, 1, (-0.5, 0.7), "A"), "CLIPMASK": (1, 1, (-0.5, 0.7), "A"), "LGAMMA": (1, 1, (), "B"),
    "POWC": (1, 1, (1.7,), "B"), "LOG1P": (1, 1, (), "B"), "COPY": (1, 1, (), "A"), "DIGAMMA": (1, 1, (), "B"),
    "ADD": (2, 1, (), "A"), "SUB": (2, 1, (), "A"), "MUL": (2, 1, (), "A"), "DIV": (2, 1, (), "A"),
    "MAX": (2, 1, (), "A"), "MIN": (2, 1, (), "A"), "POW": (2, 1, (), "B"), "GT": (2, 1, (), "A"),
    "GE": (2, 1, (), "A"), "LT": (2, 1, (), "A"), "LE": (2, 1, (), "A"), "EQ": (2, 1, (), "A"),
    "SIGMOID_GRAD": (2, 1, (), "A"), "TANH_GRAD": (2, 1, (), "A"), "RELU_GRAD": (2, 1, (), "A"),
    "SOFTPLUS_GRAD": (2, 1, (), "B"), "CLIP_GRAD": (2, 1, (-0.5, 0.7), "A"),
    "WHERE": (3, 1, (), "A"), "FMA": (3, 1, (), "A"), "GAUSS_LOGPDF": (3, 1, (), "B"),
    "GAUSS_LOGPDF_GRAD": (4, 3, (), "B"),
}
# class-A ops whose expected value is the mpmath single rounding (numpy has no fma; sqrt and divide are one IEEE
# operation each, so the exact value rounded once is the specification itself)
SINGLE_ROUNDING = ("FMA", "AFFINE", "SQRT", "DIV")

# Error bounds of the device math library in ulp.  ROCm documents its device math functions in "HIP math API" (ROCm
# HIP documentation, reference section); OCML, the library behind them, follows the table "ULP values for
# single/double precision built-in math functions" of the OpenCL specification (7.4, full profile): exp 3, log 3,
# log1p 2, tanh 5, tan 5, pow 16.  The hardware transcendentals of the fp32 sigmoid are documented in the CDNA
# instruction set reference: V_EXP_F32 and V_RCP_F32, 1 ulp each.
# lgamma has no documented bound ("undefined" in the OpenCL table).  Its yardstick is measured:
# 4 * (largest error, in ulp of the result, of the host's torch.lgamma in the dtype against mpmath on the LGAMMA points
# of this file); tests/test_ewise_table_cpu.py::test_lgamma_yardstick recomputes it and compares it with this entry.
# The factor 4: two independent libms may each sit at their own bound, on opposite sides.
ULP = {"exp": 3.0, "log": 3.0, "log1p": 2.0, "tanh": 5.0, "tan": 5.0, "pow": 16.0, "v_exp_f32": 1.0, "v_rcp_f32": 1.0}
LGAMMA_HOST_ULP = {"f32": 0.482, "f64": 0.465}     # measured (see above): the device is allowed 1.93 and 1.86 ulp

MAX_LEFT_OUT = 0.15     # share of an op's points whose reference is non-finite or subnormal (class B)


def _mp():
    import mpmath

    mpmath.mp.prec = 240
    return mpmath


def finfo(p):
    f = np.finfo(NP[p])
    return dict(eps=float(f.eps), tiny=float(f.tiny), max=float(f.max), sub=float(f.smallest_subnormal))


# --------------------------------------------------------------------------------------------------------------------
# input sets
# --------------------------------------------------------------------------------------------------------------------
def specials(p):
    f = finfo(p)
    v = [0.0, -0.0, np.inf, -np.inf, np.nan, f["tiny"], -f["tiny"], f["max"], -f["max"], 5 * f["sub"], -5 * f["sub"]]
    return np.array(v, dtype=NP[p])


def sweep(p, lo, hi, n, signs=(1,)):
    """n log-spaced magnitudes in [lo, hi] (irrational mantissas: every one rounds), each with the given signs"""
    m = np.exp(np.linspace(np.log(lo), np.log(hi), n))
    return np.concatenate([s * m for s in signs]).astype(NP[p])


def _near(p, xs, width=1):
    """xs with `width` neighbours in the dtype on both sides"""
    xs = np.asarray(xs, dtype=NP[p])
    out = [xs]
    lo = hi = xs
    for _ in range(width):
        lo = np.nextafter(lo, NP[p](-np.inf))
        hi = np.nextafter(hi, NP[p](np.inf))
        out += [lo, hi]
    return np.concatenate(out)


def _sat(p):
    big = [20, 60, 87, 88.5, 89, 104] + ([700, 710, 750] if p == "f64" else [])
    return np.array([s * b for b in big for s in (1, -1)], dtype=NP[p])


def unary_inputs(op, p):
    wide = 1e30 if p == "f32" else 1e300
    both = sweep(p, 1 / wide, wide, 120, (1, -1))
    pos = sweep(p, 1 / wide, wide, 200)
    if op in ("SQRT", "RSQRT", "LOG"):
        x = np.concatenate([pos, sweep(p, 1e-3, 1e3, 4, (-1,)), _near(p, [1.0], 2)])
    elif op == "EXP":
        edge = [88.7, -88.7, 87.3, -87.3, 103.0, -103.9] + ([709.7, -709.7, -708.3, -745.0] if p == "f64" else [])
        x = np.concatenate([sweep(p, 1e-10, 80.0 if p == "f32" else 700.0, 110, (1, -1)), _near(p, edge, 2)])
    elif op in ("SIGMOID", "SOFTPLUS"):
        x = np.concatenate([sweep(p, 1e-10, 86.0 if p == "f32" else 700.0, 110, (1, -1)), _sat(p)])
    elif op == "TANH":
        x = np.concatenate([sweep(p, 1e-10, 30.0, 110, (1, -1)), _sat(p)])
    elif op == "LOG1P":
        x = np.concatenate([pos, -sweep(p, 1 / wide, 0.999, 80), np.array([-1.0, -1.5], dtype=NP[p]), _near(p, [-1.0], 1)])
    elif op == "LGAMMA":
        x = sweep(p, 1e-30, 1e30, 241)        # 10^(k/4): 1 is a point, 2 is not
        x = np.concatenate([x, np.array([2.0, 3.0, 0.5, 1.5, 2.5, 7.0, 10.5], dtype=NP[p])])
    elif op == "DIGAMMA":
        ints = np.arange(1.0, 8.0)
        negs = -(np.arange(0, 20)[:, None] + np.array([0.03125, 0.25, 0.4609375, 0.5, 0.75, 0.96875])[None, :]).ravel()
        x = np.concatenate([sweep(p, 1e-30, 1e30, 161), _near(p, ints, 1), _near(p, [6.0], 2),
                            negs.astype(NP[p]), sweep(p, 1e-30, 1e-2, 12, (-1,)),
                            -np.arange(1.0, 21.0).astype(NP[p]), np.array([-1e5 - 0.5, -2.0 ** 23, -2.0 ** 60, -1e30], dtype=NP[p])])
    elif op == "POWC":
        x = np.concatenate([sweep(p, 1e-12, 1e12, 200), sweep(p, 1e-3, 1e3, 4, (-1,))])
    else:
        x = both
    return [np.concatenate([x, specials(p)])]


def _cross(*sets):
    g = np.meshgrid(*sets, indexing="ij")
    return [a.ravel() for a in g]


def _with_specials(p, regular, companions):
    """the cross product of the regular sets, then every special value in every slot against the companions of the other
    slots, then all slots equal to the same special"""
    cols = _cross(*regular)
    sp = specials(p)
    extra = [[] for _ in regular]
    for k in range(len(regular)):
        sets = [sp if j == k else np.asarray(companions[j], dtype=NP[p]) for j in range(len(regular))]
        for j, c in enumerate(_cross(*sets)):
            extra[j].append(c)
    for j in range(len(regular)):
        extra[j].append(sp)
    return [np.concatenate([cols[j]] + extra[j]).astype(NP[p]) for j in range(len(regular))]


def multi_inputs(op, p):
    T = NP[p]
    sp = specials(p)
    gen = np.concatenate([sweep(p, 1e-4, 1e4, 7, (1, -1)), np.array([1.0, -1.0, 0.5], dtype=T)])      # 17 regular values
    if op == "POW":
        base = np.concatenate([sweep(p, 1e-6, 1e6, 17), np.array([1.0, 2.0, 10.0], dtype=T)])
        expo = np.concatenate([sweep(p, 1e-3, 30.0, 8, (1, -1)), np.array([1.0, 2.0, -1.0, 0.5, 3.0], dtype=T)])
        reg = _with_specials(p, [base, expo], [[2.0, 0.7], [3.0, -0.5]])
        # negative bases: integer exponents are in the domain, others are not
        nb = _cross(np.array([-2.0, -0.3], dtype=T), np.array([2.0, 3.0, -1.0, 0.5], dtype=T))
        return [np.concatenate([reg[j], nb[j]]) for j in range(2)]
    if op == "SOFTPLUS_GRAD":
        a = np.concatenate([sweep(p, 1e-6, 80.0, 9, (1, -1)), _sat(p)])
        return _with_specials(p, [a, gen[:10]], [[0.3, -2.0], [1.5, -0.25]])
    if op == "GAUSS_LOGPDF":
        xs = np.array([0.3, -1.7, 12.5, -1e3, 1e-3, 2.0 ** -40, 0.0], dtype=T)
        mus = np.array([0.25, -1.7, 3.0, 1e3, -1e-2, 7e4, 0.0], dtype=T)
        var = np.array([1.0, 0.37, 1e-4, 1e4, 2.5, 1e-9, 3e7], dtype=T)
        return _with_specials(p, [xs, mus, var], [[0.3], [-1.7, 2.0], [0.37, 2.5]])
    if op == "GAUSS_LOGPDF_GRAD":
        xs = np.array([0.3, -1.7, 12.5, -1e3, 1e-3], dtype=T)
        mus = np.array([0.25, -1.7, 1e3, -1e-2, 0.0], dtype=T)
        var = np.array([1.0, 0.37, 1e-4, 1e4], dtype=T)
        g = np.array([1.0, -0.7, 3e3], dtype=T)
        return _with_specials(p, [xs, mus, var, g], [[0.3], [-1.7], [0.37, 2.5], [-0.7]])
    if OPS[op][0] == 2:
        if op in ("SIGMOID_GRAD", "TANH_GRAD"):       # a is an activation's output
            a = np.concatenate([np.linspace(-1.0, 1.0, 9), [1e-8, 1 - 2.0 ** -20, 3.0]]).astype(T)
            if op == "SIGMOID_GRAD":                  # and the saturation points as operands all the same
                a = np.concatenate([a, _sat(p)])
            s = np.concatenate([a, sp])
            return _cross(s, np.concatenate([gen[:12] if op == "TANH_GRAD" else gen[:10], sp]))
        if op in ("RELU_GRAD", "CLIP_GRAD"):
            a = np.concatenate([gen[:10], _near(p, [-0.5, 0.7], 1)])
            return _cross(np.concatenate([a, sp]), np.concatenate([gen[:8], sp]))
        s = np.concatenate([gen, sp])            # 28 values: every pair, equal pairs included
        return _cross(s, s)
    # WHERE, FMA
    s = np.concatenate([np.array([1.5, -0.3, 1e4, -2.0 ** -30], dtype=T), sp[:5], sp[7:8], sp[9:10]])
    cols = _cross(s, s, s)
    if op == "FMA":
        # products that cancel against the addend: the single rounding differs from two roundings
        r = np.random.RandomState(5)
        a, b = r.randn(120).astype(T), r.randn(120).astype(T)
        c = (-(a * b)).astype(T)
        c[::3] = r.randn(40).astype(T)
        cols = [np.concatenate([cols[0], a]), np.concatenate([cols[1], b]), np.concatenate([cols[2], c])]
    return cols


def inputs(op, p):
    return unary_inputs(op, p) if OPS[op][0] == 1 else multi_inputs(op, p)


# --------------------------------------------------------------------------------------------------------------------
# SEQ: the C expression of ew_apply, step by step in the dtype (numpy)
# --------------------------------------------------------------------------------------------------------------------
def _digamma_seq(x):
    """hb_digamma in numpy, step for step"""
    from math import pi
    T = x.dtype.type
    x = x.copy()
    refl = np.zeros_like(x)
    neg = x < 0
    y = -x
    fr = y - np.floor(y)
    pole = neg & ~(fr > 0)
    fr = np.where(fr > T(0.5), fr - T(1), fr)
    refl = np.where(neg, T(pi) / np.tan(T(pi) * fr), T(0))
    x = np.where(neg, T(1) + y, x)
    r = np.zeros_like(x)
    for _ in range(6):
        go = x < 6
        r = np.where(go, r - T(1) / x, r)
        x = np.where(go, x + T(1), x)
    f = T(1) / (x * x)
    v = r + np.log(x) - T(0.5) / x - f * (T(1.0 / 12) - f * (T(1.0 / 120) - f * (T(1.0 / 252) - f * (T(1.0 / 240) - f * T(1.0 / 132)))))
    return np.where(pole, T(np.nan), v + refl)


def _sigmoid_seq(a):
    T = a.dtype.type
    if T is np.float32:
        return T(1) / (T(1) + np.exp(-a))
    e = np.exp(-np.abs(a))
    return np.where(a >= 0, T(1) / (T(1) + e), e / (T(1) + e))


def seq(op, p, ins):
    """ew_apply's expression for `op` on dtype arrays, operation by operation.  NaN operands do what the C comparisons
    do (every comparison with a NaN is false), which is NOT numpy's / torch's maximum, minimum or clip."""
    import math

    def gammaln(v):      # C's lgamma: +inf at the poles and at both infinities
        def one_(t):
            try:
                return math.lgamma(t)
            except (ValueError, OverflowError):
                return math.inf
        return np.array([one_(float(t)) for t in v])

    T = NP[p]
    a = ins[0]
    b = ins[1] if len(ins) > 1 else None
    c = ins[2] if len(ins) > 2 else None
    d = ins[3] if len(ins) > 3 else None
    pr = [T(v) for v in OPS[op][2]] + [T(0), T(0)]
    one, zero = T(1), T(0)
    W = np.where
    with np.errstate(all="ignore"):
        if op == "NEG": r = -a
        elif op == "EXP": r = np.exp(a)
        elif op == "LOG": r = np.log(a)
        elif op == "SQRT": r = np.sqrt(a)
        elif op == "SQUARE": r = a * a
        elif op == "ABS": r = W(a < 0, -a, a)
        elif op == "SIGN": r = W(a > 0, one, W(a < 0, -one, zero))
        elif op == "SIGMOID": r = _sigmoid_seq(a)
        elif op == "RELU": r = W(a > 0, a, zero)
        elif op == "SOFTPLUS": r = W(a > 0, a, zero) + np.log1p(np.exp(-W(a < 0, -a, a)))
        elif op == "TANH": r = np.tanh(a)
        elif op == "RECIP": r = one / a
        elif op == "RSQRT": r = one / np.sqrt(a)
        elif op == "STEP": r = W(a > 0, one, zero)
        elif op == "AFFINE": r = pr[0] * a + pr[1]        # (two roundings: replaced by the single rounding in expected())
        elif op == "CLIP": r = W(a < pr[0], pr[0], W(a > pr[1], pr[1], a))
        elif op == "CLIPMASK": r = W((a >= pr[0]) & (a <= pr[1]), one, zero)
        elif op == "LGAMMA": r = gammaln(a).astype(T)
        elif op == "POWC": r = np.power(a, pr[0])
        elif op == "LOG1P": r = np.log1p(a)
        elif op == "COPY": r = a.copy()
        elif op == "DIGAMMA": r = _digamma_seq(a)
        elif op == "ADD": r = a + b
        elif op == "SUB": r = a - b
        elif op == "MUL": r = a * b
        elif op == "DIV": r = a / b
        elif op == "MAX": r = W(a > b, a, b)
        elif op == "MIN": r = W(a < b, a, b)
        elif op == "POW": r = np.power(a, b)
        elif op == "GT": r = W(a > b, one, zero)
        elif op == "GE": r = W(a >= b, one, zero)
        elif op == "LT": r = W(a < b, one, zero)
        elif op == "LE": r = W(a <= b, one, zero)
        elif op == "EQ": r = W(a == b, one, zero)
        elif op == "SIGMOID_GRAD": r = b * a * (one - a)
        elif op == "TANH_GRAD": r = b * (one - a * a)
        elif op == "RELU_GRAD": r = W(a > 0, b, zero)
        elif op == "SOFTPLUS_GRAD": r = b * _sigmoid_seq(a)
        elif op == "CLIP_GRAD": r = W((a >= pr[0]) & (a <= pr[1]), b, zero)
        elif op == "WHERE": r = W(a != 0, b, c)
        elif op == "FMA": r = a * b + c                   # (two roundings: replaced by the single rounding in expected())
        elif op == "GAUSS_LOGPDF":
            dlt = b - a
            r = T(-0.91893853320467274178) - T(0.5) * np.log(c) - T(0.5) * dlt * dlt / c
        elif op == "GAUSS_LOGPDF_GRAD":
            dlt = b - a
            iv = one / c
            return [np.asarray(v, dtype=T) for v in (d * dlt * iv, -d * dlt * iv, d * (T(-0.5) * iv + T(0.5) * dlt * dlt * iv * iv))]
        else:
            raise KeyError(op)
    return [np.asarray(r, dtype=T)]


# --------------------------------------------------------------------------------------------------------------------
# EXACT: mpmath definition of every op on exact rationals (None where the point is outside the op's real domain)
# --------------------------------------------------------------------------------------------------------------------
def exact(op, p, x):
    """x: tuple of mpf (finite).  Returns a list of mpf, or None where the op has no finite real value there (the caller
    takes SEQ's IEEE answer instead)."""
    mp = _mp()
    T = NP[p]
    a = x[0]
    b = x[1] if len(x) > 1 else None
    c = x[2] if len(x) > 2 else None
    d = x[3] if len(x) > 3 else None
    pr = [mp.mpf(float(T(v))) for v in OPS[op][2]] + [mp.mpf(0)] * 2
    one = mp.mpf(1)
    tf = lambda cond: one if cond else mp.mpf(0)
    if op == "NEG": return [-a]
    if op == "EXP": return [mp.exp(a)]
    if op == "LOG": return [mp.log(a)] if a > 0 else None
    if op == "SQRT": return [mp.sqrt(a)] if a >= 0 else None
    if op == "SQUARE": return [a * a]
    if op == "ABS": return [abs(a)]
    if op == "SIGN": return [mp.sign(a)]
    if op == "SIGMOID": return [one / (one + mp.exp(-a))]
    if op == "RELU": return [a if a > 0 else mp.mpf(0)]
    if op == "SOFTPLUS": return [max(a, 0) + mp.log1p(mp.exp(-abs(a)))]
    if op == "TANH": return [mp.tanh(a)]
    if op == "RECIP": return [one / a] if a != 0 else None
    if op == "RSQRT": return [one / mp.sqrt(a)] if a > 0 else None
    if op == "STEP": return [tf(a > 0)]
    if op == "AFFINE":
        with mp.workprec(4600):      # exact: the addend may sit 2000 binary places below the product
            return [pr[0] * a + pr[1]]
    if op == "CLIP": return [min(max(a, pr[0]), pr[1])]
    if op == "CLIPMASK": return [tf(pr[0] <= a <= pr[1])]
    if op == "LGAMMA":
        if a > 0: return [mp.loggamma(a)]
        if -1 < a < 0: return [mp.log(abs(mp.gamma(a)))]
        return None
    if op == "POWC": return [mp.power(a, pr[0])] if a > 0 else None
    if op == "LOG1P": return [mp.log1p(a)] if a > -1 else None
    if op == "COPY": return [a]
    if op == "DIGAMMA":
        if a == 0 or (a < 0 and a == mp.floor(a)): return None
        return [mp.digamma(a)]
    if op == "ADD": return [a + b]
    if op == "SUB": return [a - b]
    if op == "MUL": return [a * b]
    if op == "DIV": return [a / b] if b != 0 else None
    if op == "MAX": return [max(a, b)]
    if op == "MIN": return [min(a, b)]
    if op == "POW":
        if a > 0: return [mp.power(a, b)]
        if a < 0 and b == mp.floor(b) and abs(b) < 1000: return [mp.power(a, int(b))]
        return None
    if op == "GT": return [tf(a > b)]
    if op == "GE": return [tf(a >= b)]
    if op == "LT": return [tf(a < b)]
    if op == "LE": return [tf(a <= b)]
    if op == "EQ": return [tf(a == b)]
    if op == "SIGMOID_GRAD": return [b * a * (one - a)]
    if op == "TANH_GRAD": return [b * (one - a * a)]
    if op == "RELU_GRAD": return [b if a > 0 else mp.mpf(0)]
    if op == "SOFTPLUS_GRAD": return [b / (one + mp.exp(-a))]
    if op == "CLIP_GRAD": return [b if pr[0] <= a <= pr[1] else mp.mpf(0)]
    if op == "WHERE": return [b if a != 0 else c]
    if op == "FMA":
        with mp.workprec(4600):
            return [a * b + c]
    if op == "GAUSS_LOGPDF":
        if c <= 0: return None
        return [-mp.log(2 * mp.pi) / 2 - mp.log(c) / 2 - (b - a) ** 2 / (2 * c)]
    if op == "GAUSS_LOGPDF_GRAD":
        if c == 0: return None
        dl = b - a
        return [d * dl / c, -d * dl / c, d * (-one / (2 * c) + dl * dl / (2 * c * c))]
    raise KeyError(op)


# --------------------------------------------------------------------------------------------------------------------
# forward error bound of the op's sequence
# --------------------------------------------------------------------------------------------------------------------
class V:
    __slots__ = ("v", "e", "ovf")

    def __init__(self, v, e=0, ovf=False):
        self.v, self.e, self.ovf = v, e, ovf


class Tracker:
    """Carries (exact value, first-order bound on the accumulated absolute error) through a sequence of operations.
    A step's own rounding is u * eps * |value|, never less than u subnormal spacings (gradual underflow); a hardware
    transcendental (flush=True) may return 0 for a subnormal result: the smallest normal.  An intermediate above the
    largest finite value sets `ovf`; a quotient by it is 0 on the device, so its whole (tiny) value becomes error and
    the flag clears.  Any other use leaves the flag standing and the point outside the sequence's range."""

    def __init__(self, p):
        self.mp = _mp()
        f = finfo(p)
        self.p, self.T = p, NP[p]
        self.eps, self.tiny, self.max = (self.mp.mpf(f[k]) for k in ("eps", "tiny", "max"))

    def inp(self, x): return V(x)

    def const(self, exact_value, literal):
        """a literal of the source: the device holds T(literal), the mathematics means exact_value"""
        return V(exact_value, abs(self.mp.mpf(float(self.T(literal))) - exact_value))

    def _r(self, v, e, u, ovf=False, flush=False):
        floor = self.tiny if flush else u * self.eps * self.tiny
        return V(v, e + max(u * self.eps * abs(v), floor), ovf or abs(v) > self.max)

    def neg(self, a): return V(-a.v, a.e, a.ovf)
    def add(self, a, b): return self._r(a.v + b.v, a.e + b.e, 0.5, a.ovf or b.ovf)
    def sub(self, a, b): return self._r(a.v - b.v, a.e + b.e, 0.5, a.ovf or b.ovf)
    def mul(self, a, b): return self._r(a.v * b.v, abs(b.v) * a.e + abs(a.v) * b.e, 0.5, a.ovf or b.ovf)

    def div(self, a, b):
        v = a.v / b.v
        if b.ovf and not a.ovf:
            return V(v, abs(v) + self.tiny)
        return self._r(v, a.e / abs(b.v) + abs(v) * b.e / abs(b.v), 0.5, a.ovf or b.ovf)

    def fn(self, name, a, f, df, flush=False):
        v = f(a.v)
        if a.ovf and name == "v_rcp_f32":      # 1 / inf = 0 on the device: as in div
            return V(v, abs(v) + self.tiny)
        return self._r(v, abs(df(a.v)) * a.e, ULP[name] if name != "lgamma" else 4 * LGAMMA_HOST_ULP[self.p], a.ovf, flush)

    def pow(self, a, b):
        mp = self.mp
        v = mp.power(a.v, b.v) if a.v > 0 else mp.power(a.v, int(b.v))
        da = abs(b.v * v / a.v)
        db = abs(v * mp.log(abs(a.v)))
        return self._r(v, da * a.e + db * b.e, ULP["pow"], a.ovf or b.ovf)


def _sigmoid_bound(t, x):
    """hb_sigmoid: fp64 = the two-branch IEEE form; fp32 = v_rcp_f32(1 + v_exp_f32(log2e_f32 * -x))"""
    mp = t.mp
    one = V(mp.mpf(1))
    if t.p == "f32":
        log2e = t.const(1 / mp.log(2), float.fromhex("0x1.715476p+0"))   # __expf: the float literal of the compiler header
        arg = t.mul(log2e, t.neg(x))
        e = t.fn("v_exp_f32", arg, lambda v: mp.power(2, v), lambda v: mp.log(2) * mp.power(2, v), flush=True)
        s = t.add(one, e)
        return t.fn("v_rcp_f32", s, lambda v: 1 / v, lambda v: 1 / (v * v), flush=True)
    if x.v >= 0:
        e = t.fn("exp", t.neg(x), mp.exp, mp.exp)
        return t.div(one, t.add(one, e))
    e = t.fn("exp", x, mp.exp, mp.exp)
    return t.div(e, t.add(one, e))


def _digamma_bound(t, x):
    mp = t.mp
    one = V(mp.mpf(1))
    refl = None
    if x.v < 0:
        y = -x.v
        fr = y - mp.floor(y)
        if fr > mp.mpf(0.5):
            fr -= 1
        pi = t.const(mp.pi, 3.14159265358979323846)
        tn = t.fn("tan", t.mul(pi, V(fr)), mp.tan, lambda v: 1 + mp.tan(v) ** 2)
        refl = t.div(pi, tn)
        x = t.add(one, V(y))
    # the trips are decided by the ROUNDED argument (3.9999999999999996 + 1 is 5 in the dtype: one trip fewer than in
    # exact arithmetic, and the series then starts at 6, where its truncation error is largest)
    xt = t.T(float(x.v))
    r = V(mp.mpf(0))
    for _ in range(6):
        if not xt < 6:
            break
        r = t.sub(r, t.div(one, x))
        x = t.add(x, one)
        xt = xt + t.T(1)
    f = t.div(one, t.mul(x, x))
    cs = [t.const(mp.mpf(1) / k, 1.0 / k) for k in (12, 120, 252, 240, 132)]
    s = t.mul(f, cs[4])
    for k in (3, 2, 1, 0):
        s = t.mul(f, t.sub(cs[k], s))
    v = t.sub(t.sub(t.add(r, t.fn("log", x, mp.log, lambda z: 1 / z)), t.div(V(mp.mpf(0.5)), x)), s)
    return t.add(v, refl) if refl is not None else v


def bound(op, p, x):
    """list of (sequence value in exact arithmetic, error bound, overflow flag), one per output"""
    t = Tracker(p)
    mp = t.mp
    X = [t.inp(v) for v in x]
    a = X[0]
    one, half = V(mp.mpf(1)), V(mp.mpf(0.5))
    pr = [V(mp.mpf(float(t.T(v)))) for v in OPS[op][2]]
    if op == "EXP": r = [t.fn("exp", a, mp.exp, mp.exp)]
    elif op == "LOG": r = [t.fn("log", a, mp.log, lambda z: 1 / z)]
    elif op == "SIGMOID": r = [_sigmoid_bound(t, a)]
    elif op == "SOFTPLUS":
        e = t.fn("exp", V(-abs(a.v)), mp.exp, mp.exp)
        l = t.fn("log1p", e, mp.log1p, lambda z: 1 / (1 + z))
        r = [t.add(V(max(a.v, 0)), l)]
    elif op == "TANH": r = [t.fn("tanh", a, mp.tanh, lambda z: 1 - mp.tanh(z) ** 2)]
    elif op == "LGAMMA":
        lg = (lambda z: mp.loggamma(z)) if a.v > 0 else (lambda z: mp.log(abs(mp.gamma(z))))
        r = [t.fn("lgamma", a, lg, mp.digamma)]
    elif op == "POWC": r = [t.pow(a, pr[0])]
    elif op == "LOG1P": r = [t.fn("log1p", a, mp.log1p, lambda z: 1 / (1 + z))]
    elif op == "DIGAMMA": r = [_digamma_bound(t, a)]
    elif op == "POW": r = [t.pow(a, X[1])]
    elif op == "SOFTPLUS_GRAD": r = [t.mul(X[1], _sigmoid_bound(t, a))]
    elif op == "GAUSS_LOGPDF":
        dlt = t.sub(X[1], a)
        k = t.const(-mp.log(2 * mp.pi) / 2, -0.91893853320467274178)
        lg = t.mul(half, t.fn("log", X[2], mp.log, lambda z: 1 / z))
        q = t.div(t.mul(t.mul(half, dlt), dlt), X[2])
        r = [t.sub(t.sub(k, lg), q)]
    elif op == "GAUSS_LOGPDF_GRAD":
        dlt = t.sub(X[1], a)
        iv = t.div(one, X[2])
        g = X[3]
        o0 = t.mul(t.mul(g, dlt), iv)
        o1 = t.mul(t.mul(t.neg(g), dlt), iv)
        o2 = t.mul(g, t.add(t.mul(V(mp.mpf(-0.5)), iv), t.mul(t.mul(t.mul(t.mul(half, dlt), dlt), iv), iv)))
        r = [o0, o1, o2]
    else:
        raise KeyError(op)
    return [(v.v, v.e, v.ovf) for v in r]


# --------------------------------------------------------------------------------------------------------------------
# expected values and tolerances
# --------------------------------------------------------------------------------------------------------------------
def round_to(p, v):
    """one rounding of an mpf to the dtype (overflow -> +-inf)"""
    mp = _mp()
    from mpmath.libmp import mpf_pos, round_nearest

    # (float(mpf) alone truncates: the mantissa is rounded to nearest here, and the conversion is then exact)
    r = float(mp.mpf(mpf_pos(v._mpf_, 24 if p == "f32" else 53, round_nearest)))
    with np.errstate(over="ignore"):
        return NP[p](r)


def table(op, p):
    """(inputs [nin][n], expected [nout][n], tol [nout][n] (class B; NaN where the point is not compared by value))"""
    mp = _mp()
    f = finfo(p)
    nin, nout, _, cls = OPS[op]
    ins = inputs(op, p)
    n = ins[0].size
    exp = [e.copy() for e in seq(op, p, ins)]
    tol = np.full((nout, n), np.nan)
    use_exact = cls == "B" or op in SINGLE_ROUNDING
    dropped = np.zeros(n, dtype=bool)
    if use_exact:
        for i in range(n):
            x = [float(c[i]) for c in ins]
            if not all(np.isfinite(x)):
                if op in ("FMA", "AFFINE"):
                    # fused: a finite product cannot overflow before the addend comes in (SEQ's two steps can)
                    fa, fb, fc = (x[0], x[1], x[2]) if op == "FMA" else (float(NP[p](OPS[op][2][0])), x[0], float(NP[p](OPS[op][2][1])))
                    with np.errstate(all="ignore"):
                        exp[0][i] = fc if (np.isfinite(fa) and np.isfinite(fb)) else np.float64(fa) * np.float64(fb) + np.float64(fc)
                # IEEE / Annex F answers: kind and sign; finite ones (0, 1, a copied operand) exactly
                for k in range(nout):
                    tol[k, i] = 0.0
                continue
            xm = tuple(mp.mpf(v) for v in x)
            ex = exact(op, p, xm)
            if ex is None:
                for k in range(nout):
                    tol[k, i] = 0.0
                continue
            if cls == "B":
                bd = bound(op, p, xm)
            seq_kind = [float(exp[k][i]) for k in range(nout)]
            for k in range(nout):
                if ex[k] != 0:       # an exact zero keeps the sign IEEE 754 gives it in SEQ
                    exp[k][i] = round_to(p, ex[k])
                elif exp[k][i] != 0:
                    exp[k][i] = 0.0
                if cls == "B":
                    sv, se, ovf = bd[k]
                    if ovf and (np.isfinite(exp[k][i]) or np.isnan(seq_kind[k])):
                        # an intermediate of the sequence leaves the dtype's range on the way to a finite value, or
                        # turns an overflowing one into inf - inf: the point is outside the sequence's range
                        dropped[i] = True
                    ulp_ref = max(abs(ex[k]), mp.mpf(f["tiny"])) * f["eps"] / 2
                    tol[k, i] = float(se + abs(sv - ex[k]) + ulp_ref)
    keep = ~dropped
    return [c[keep] for c in ins], [e[keep] for e in exp], tol[:, keep], int(dropped.sum())


def left_out(p, exp):
    """points a class-B comparison leaves to the kind-and-sign check: reference not finite, or subnormal"""
    tiny = finfo(p)["tiny"]
    e = np.asarray(exp, dtype=np.float64)
    return ~np.isfinite(e) | ((e != 0) & (np.abs(e) < tiny))


def check(p, op, got, exp, tol, what):
    """The assertion of the CPU and the GPU test.  got, exp: [nout, n] in the dtype; tol: [nout, n] (class B) or None (class A)."""
    f = finfo(p)
    cls = OPS[op][3]
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape)
    g64, e64 = got.astype(np.float64), exp.astype(np.float64)
    out = left_out(p, exp)
    # reference not finite: the same kind and sign
    nan = np.isnan(e64)
    assert np.all(np.isnan(g64[nan])), "%s: %d points should be NaN" % (what, int((~np.isnan(g64[nan])).sum()))
    inf = np.isinf(e64)
    assert np.array_equal(g64[inf], e64[inf]), "%s: infinities differ" % what
    # reference subnormal: within the smallest normal (a flushed result is as good as a gradual one)
    sub = out & ~nan & ~inf
    assert np.all(np.abs(g64[sub] - e64[sub]) <= f["tiny"]), "%s: subnormal results" % what
    ok = ~out
    if cls == "A":
        U = np.uint32 if p == "f32" else np.uint64
        bad = ok & (got.view(U) != exp.view(U))
        assert not bad.any(), "%s: %d of %d results differ in their bits, first at point %s: got %r, expected %r" % (
            what, int(bad.sum()), int(ok.sum()), np.argwhere(bad)[0], got[bad][0], exp[bad][0])
        return
    assert out.any(0).mean() <= MAX_LEFT_OUT, "%s: %.0f %% of the points have no finite normal reference" % (what, 100 * out.any(0).mean())
    with np.errstate(invalid="ignore"):
        err = np.abs(g64 - e64)
        bad = ok & ~(err <= tol)
    if bad.any():
        k = np.argwhere(bad)[np.argmax((err / np.maximum(tol, 1e-300))[bad])]
        raise AssertionError("%s: %d of %d points over the bound; worst output %d point %d: got %r, expected %r, allowed %.3g"
                             % (what, int(bad.sum()), int(ok.sum()), k[0], k[1], got[tuple(k)], exp[tuple(k)], tol[tuple(k)]))


DROPPED = {}     # (dtype, op) -> points left out of the set because the sequence leaves the dtype's range (filled by build_fixture)


def build_fixture():
    out = {}
    for p in ("f32", "f64"):
        for op in OPS:
            ins, exp, tol, dropped = table(op, p)
            DROPPED[p, op] = dropped
            out["%s/%s/in" % (p, op)] = np.stack(ins)
            out["%s/%s/exp" % (p, op)] = np.stack(exp)
            if OPS[op][3] == "B":
                out["%s/%s/tol" % (p, op)] = tol
    return out


def load_fixture():
    return np.load(FIXTURE)


if __name__ == "__main__":
    if "--write" in sys.argv:
        np.savez_compressed(FIXTURE, **build_fixture())
        print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
    else:
        print(__doc__)
