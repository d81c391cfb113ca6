"""Gram kernels (hb_gram_fwd, hb_gram_bwd) swept over the paths the small tests never reach: d above HB_GRAM_MAXD (the
chunk loop over k0), more than one trip of the 256-thread loop over the other side, the squared-distance VJP, float32,
shared and per-batch operands, the one-pass symmetric form, and a forward with more entries than one trip of the capped
grid covers.  Reference: tests/gram_ref.py (float64 numpy) on inputs that are exact in float32.

Tolerances.  float64: TOL["f64"] of tests/test_kernels_gpu.py.  float32: |err| <= k * 2^-24 * S.  S comes from the
reference: the sum of the magnitudes of an entry's terms, in which a difference a - b of the rounded scaled coordinates
counts as |a| + |b| (its error does not shrink with it) and the squared distance accordingly as
c = sum_k |a_k - b_k| (|a_k| + |b_k|).  k is counted from gram_value / gram_bwd_side_kernel, in units of one rounding
(2^-24 relative):
    squared distance  per dimension, relative to |a-b| (|a|+|b|): 1/ell (it scales a - b, which is squared: 2), x*il and
                      x2*il (together 2^-24 (|a|+|b|) in a - b, which is squared: 2), a - b (squared: 2), the square (1)
                      -> 7; the d chained adds -> d.  Through exp(-r^2/2) this is weighted by c/2, which S carries.
    exp               3 ulp = 6 roundings (the product -0.5 * r2 is exact)
    point summand     kb*km (1); 1/ell (in a - b and as the last factor: 2), x*il and x2*il (1), a - b (1), * gm (1),
                      the subtraction of the E+ term (1), * il (1), the add into the accumulator (1) -> 9
    lengthscale       kb*km (1); a - b squared, each factor with 1/ell, x*il and x2*il, and its subtraction (6), the
    summand           square (1), * em (1), the add of the E+ term (1), 1/ell as the last factor (1), * il (1), the add
                      into the accumulator (1) -> 13
    summation depth   ceil(other / 256) sequential adds per thread + 12 levels of block_sum (two wave_sums);
                      a gradient summed over the batch (shared operand): + B; the lengthscale fold: + ceil(rows*d / 256) + 12
  Per kind, only what the kind computes: CSYM as above; RBF has no E+ term, so the subtraction resp. add of it is
  exact (summands 8 and 12); SQDIST has E- := -2, a constant: no squared distance and no exp in its VJP, kb * -2 exact
  (summands 7 and 11), and its forward is the squared distance alone.
    forward  SQDIST 7 + d;  RBF (7 + d) + 6;  CSYM (7 + d) + 6 + 1 (the add of the two exponentials)
    VJP      SQDIST summand + depth;  RBF, CSYM (7 + d) + 6 + summand + depth
  Counted, not fitted to what the kernels return."""
import functools

import numpy as np
import pytest
import torch

import gram_ref as G

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f64": torch.float64}
TOL = {"f64": dict(rtol=1e-9, atol=1e-10)}
KINDS = {"rbf": G.RBF, "csym": G.CSYM, "sqdist": G.SQDIST}
U32 = 2.0 ** -24


@pytest.fixture(scope="module")
def H():
    from henbun_amd import hip_ops

    assert torch.cuda.is_available()
    return hip_ops


def dev(a, p):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=DT[p]).cuda()


def host(t):
    return t.detach().cpu().double().numpy()


def close(got, exp, S, p, k, what):
    got = host(got).reshape(exp.shape)
    err = np.abs(got - exp)
    bound = (TOL["f64"]["atol"] + TOL["f64"]["rtol"] * np.abs(exp)) if p == "f64" else k * U32 * S
    bad = ~(err <= bound)
    assert not bad.any(), "%s: %d of %d entries over the bound, worst err %.3e (allowed %.3e)" % (
        what, int(bad.sum()), bad.size, err[bad].max(), bound[bad][np.argmax(err[bad])])


def k_fwd(kind, d):
    return (7 + d) + {G.SQDIST: 0, G.RBF: 6, G.CSYM: 6 + 1}[kind]


def k_bwd(kind, d, other, extra=0, ell=False):
    value = 0 if kind == G.SQDIST else (7 + d) + 6                   # E-, E+ as factors of the summand
    summand = {G.SQDIST: 7, G.RBF: 8, G.CSYM: 9}[kind] + (4 if ell else 0)
    return value + summand + -(-other // 256) + 12 + extra


def k_ell(kind, d, other, rows):
    return k_bwd(kind, d, other, -(-rows // 256) + 12, ell=True)


# (d, n, n2, ard, B, second operand shared 2-D, lengthscales per batch entry): every value of every list of the issue
# appears with every kind and dtype
CONFIGS = [
    (1, 1, 1, False, 1, False, False),
    (3, 7, 300, True, 3, True, False),
    (8, 300, 7, True, 3, False, True),
    (9, 257, 513, False, 1, False, False),
    (17, 7, 300, True, 1, False, False),
    (17, 300, 7, False, 3, True, True),
]


@functools.lru_cache(maxsize=None)
def case(kind, cfg):
    """inputs (float64 values that are exact in float32) and the float64 reference, computed once for both dtypes"""
    d, n, n2, ard, B, x2_shared, ell_batched = cfg
    r = np.random.RandomState(1000 * d + n)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    X = f32(r.randn(B, n, d))
    X2 = f32(r.randn(1 if x2_shared else B, n2, d))
    ell = f32(np.exp(0.3 * r.randn(B if ell_batched else 1, d if ard else 1)) * np.sqrt(d))
    Kbar = f32(r.randn(B, n, n2))
    K, SK = G.gram(kind, X, X2, ell)
    (gx, gx2, gl), (sx, sx2, sl) = G.gram_vjp(kind, X, X2, ell, Kbar)
    if x2_shared:
        gx2, sx2 = gx2.sum(0, keepdims=True), sx2.sum(0, keepdims=True)
    if not ell_batched:
        gl, sl = gl.sum(0, keepdims=True), sl.sum(0, keepdims=True)
    if not ard:
        gl, sl = gl.sum(1, keepdims=True), sl.sum(1, keepdims=True)
    return X, X2, ell, Kbar, K, SK, (gx, gx2, gl), (sx, sx2, sl)


@pytest.mark.parametrize("p", ["f32", "f64"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "d%d-n%d-n2_%d-%s-B%d%s%s" % (c[0], c[1], c[2], "ard" if c[3] else "iso", c[4],
                                                                                  "-x2shared" if c[5] else "", "-ellbatch" if c[6] else ""))
def test_gram_forward_and_vjp(H, cfg, kind, p):
    d, n, n2, ard, B, x2_shared, ell_batched = cfg
    X, X2, ell, Kbar, K, SK, g, S = case(KINDS[kind], cfg)
    tX = dev(X if B > 1 else X[0], p)
    tX2 = dev(X2[0] if (x2_shared or B == 1) else X2, p)
    tl = dev(ell if ell_batched else ell[0], p)
    what = "%s %s %s" % (kind, p, cfg)
    got = H.gram_fwd(tX, tX2, tl, kind=KINDS[kind])
    close(got, K, SK, p, k_fwd(KINDS[kind], d), what + " K")
    tK = dev(Kbar if B > 1 else Kbar[0], p)
    xb, x2b, lb = H.gram_bwd(tX, tX2, tl, tK, kind=KINDS[kind])
    torch.cuda.synchronize()
    close(xb, g[0], S[0], p, k_bwd(KINDS[kind], d, n2), what + " Xbar")
    close(x2b, g[1], S[1], p, k_bwd(KINDS[kind], d, n, B if x2_shared else 0), what + " X2bar")
    rows = (n if ell_batched else B * n) * (1 if ard else d)
    close(lb, g[2], S[2], p, k_ell(KINDS[kind], d, n2, rows), what + " ellbar")


@pytest.mark.parametrize("p", ["f32", "f64"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("kbar_symmetric", [False, True])
def test_gram_vjp_one_pass_symmetric_form(H, kind, p, kbar_symmetric):
    """X2 is X and X2bar is Xbar: the total point gradient in one pass (the transposed entry of Kbar read, or -- with
    KERN_KBAR_SYMMETRIC -- taken to be the entry itself); the lengthscale gradient counts every pair once."""
    n, d, B = 300, 9, 1
    r = np.random.RandomState(5)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    X = f32(r.randn(B, n, d))
    ell = f32(np.exp(0.3 * r.randn(1, d)) * 3.0)
    Kbar = f32(r.randn(B, n, n))
    if kbar_symmetric:
        Kbar = f32(0.5 * (Kbar + np.transpose(Kbar, (0, 2, 1))))
    (gx, gx2, gl), (sx, sx2, sl) = G.gram_vjp(KINDS[kind], X, X, ell, Kbar)
    tX, tl, tK = dev(X[0], p), dev(ell[0], p), dev(Kbar[0], p)
    xbar = torch.empty(B, n, d, dtype=DT[p], device="cuda")
    ellbar = torch.empty(d, dtype=DT[p], device="cuda")
    ws = H.workspace(DT[p], tX.device, B * n * d)
    flags = KINDS[kind] | (H.KERN_KBAR_SYMMETRIC if kbar_symmetric else 0)
    H.gram_bwd_raw(flags, tX, 0, tX, 0, tl, 0, d, tK, xbar, xbar, ellbar, B, n, n, d, ws)
    torch.cuda.synchronize()
    what = "%s %s symmetric=%s" % (kind, p, kbar_symmetric)
    close(xbar, gx + gx2, sx + sx2, p, k_bwd(KINDS[kind], d, n) + 1, what + " Xbar")       # + 1: kb + Kbar[j,i]
    close(ellbar, gl.sum(0), sl.sum(0), p, k_ell(KINDS[kind], d, n, n), what + " ellbar")


@pytest.mark.parametrize("p", ["f32", "f64"])
def test_gram_edges_empty_side_rectangular_jitter_and_a_second_grid_trip(H, p):
    r = np.random.RandomState(8)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    # n2 = 0: zeros for the gradients of the side that exists and of the lengthscales (the empty operands are passed as
    # one-element buffers: an empty tensor has no address)
    B, n, d = 2, 5, 3
    X, ell = dev(r.randn(B, n, d), p), dev(np.ones(d), p)
    dummy = torch.ones(1, dtype=DT[p], device="cuda")
    xbar = torch.full((B, n, d), 7.0, dtype=DT[p], device="cuda")
    ellbar = torch.full((d,), 7.0, dtype=DT[p], device="cuda")
    ws = H.workspace(DT[p], X.device, B * n * d)
    H.gram_bwd_raw(H.KERN_RBF, X, n * d, dummy, 0, ell, 0, d, dummy, xbar, None, ellbar, B, n, 0, d, ws)
    torch.cuda.synchronize()
    assert not xbar.any() and not ellbar.any()
    # diag_add on a rectangular K touches i == j only
    for n, n2 in [(7, 12), (12, 7)]:
        A, C = f32(r.randn(n, 2)), f32(r.randn(n2, 2))
        l = np.array([[1.5]])
        K, S = G.gram(G.RBF, A[None], C[None], l)
        K = K[0] + 0.25 * np.eye(n, n2)
        close(H.gram_fwd(dev(A, p), dev(C, p), dev(l[0], p), diag_add=0.25), K, S[0] + 0.25 * np.eye(n, n2), p, k_fwd(G.RBF, 2) + 1, "diag_add")
    # 3 x 420 x 420 = 529200 entries: more than the 2048 x 256 threads of the capped grid
    B, n, d = 3, 420, 2
    A, l = f32(r.randn(B, n, d)), f32(np.exp(0.2 * r.randn(1, d)))
    for kind in (G.RBF, G.CSYM, G.SQDIST):
        K, S = G.gram(kind, A, A, l)
        close(H.gram_fwd(dev(A, p), dev(A, p), dev(l[0], p), kind=kind), K, S, p, k_fwd(kind, d), "large forward kind %d" % kind)
