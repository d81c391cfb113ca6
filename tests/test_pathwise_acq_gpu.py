"""Batch acquisition from function draws on the GPU: hb_sgp_pathwise_acq against the numpy restatement
tests/pathwise_acq_ref.py (pinned on the host by tests/test_pathwise_acq_cpu.py), and PathwiseDraws.acquisition /
select_batch through SVGP.suggest_batch and ExactGPR.suggest_batch.

The kernel's values F = hb_sgp_pathwise(...) are READ BACK and the restatement is taken of them, so every comparison
isolates the new epilogue: the reduction over the draws and the arg-max.  Bounds:
  PI              value is (T)(count / S) bit for bit: a count of draws is exact in double whatever the order.
  EI float64      |value - ref| <= (2S + 4) 2^-53 ref: both are sums of the same S non-negative doubles (each one rounded
                  difference of the same two numbers) in some order, relative error at most (S - 1) 2^-53 each to first
                  order, and a division.
  EI float32      at most one float32 ulp from fl32(ref): the double sum, divided, is rounded once; it differs from the
                  rounded reference only where the two doubles straddle a rounding boundary.
  arg-max         np.argmax of the entry's OWN value and the value there, bit for bit.
Everything said to be the same is compared bit for bit.  Every figure is printed before it is asserted."""
import ctypes

import numpy as np
import pytest
import torch

from henbun_amd import _lib
from henbun_amd import hip_ops as H
from henbun_amd.models import SVGP, ExactGPR, svgp_data

import pathwise_acq_ref as AR
import pathwise_ref as PR
import sites_ref as SR

pytestmark = pytest.mark.gpu

TORCH = {"float64": torch.float64, "float32": torch.float32}
NP = {"float64": np.float64, "float32": np.float32}
SCALE = 1.7


def dev(a, dt):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def ei_bound(S, ref):
    return (2 * S + 4) * 2.0 ** -53 * ref


# ------------------------------------------------------------------------------------------------ 1. the kernel
# (n, L, M, d, S): one point, one draw, M = 0; a strip of 128 and the 64 draws of a workgroup crossed; a row tile of 16
# crossed with a ragged K-step; d = 5, the path that re-reads the coordinates; three tiles of draws
SHAPES = [(1, 1, 0, 1, 1), (130, 8, 8, 1, 65), (257, 33, 40, 2, 17), (300, 16, 40, 5, 2), (1000, 20, 24, 3, 130)]
_CASE = {}


def _case(shape, dtype):
    """Operands on the device, the values F hb_sgp_pathwise stores for them (numpy) and the per-draw incumbents, the
    median of each row of F: computed once."""
    key = (shape, dtype)
    if key not in _CASE:
        n, L, M, d, S = shape
        dl = d if d > 1 else 1
        ops = tuple(dev(a, TORCH[dtype]) for a in PR.kernel_case(n, L, M, d, S, dl, 8.0, seed=n + L + M + d + S))
        F = H.sgp_pathwise(*ops, scale=SCALE).cpu().numpy()
        b = np.median(F, axis=1).astype(NP[dtype])
        _CASE[key] = (ops, F, b)
    return _CASE[key]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-L%d-M%d-d%d-S%d" % s)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_acq_kernel_against_the_restatement(dtype, shape):
    """Both kinds, largest and smallest, incumbent[s] = the median of draw s over the candidates (for odd n a value of
    the draw itself: the difference is then exactly 0 there and must not count as an improvement).  values=False returns
    the same (best, idx), leaves a sentinel-filled `out` untouched and writes nothing of the workspace past
    sgp_pathwise_acq_ws_elems.  Observed on MI355X: see DESIGN.md 3, "Batch acquisition from function draws"."""
    dt, npt = TORCH[dtype], NP[dtype]
    ops, F, b = _case(shape, dtype)
    n, L, M, d, S = shape
    bd = dev(b, dt)
    need = H.sgp_pathwise_acq_ws_elems(n, S)
    assert need == 2 * ((n + 127) // 128) + (0 if S <= 64 else ((S + 63) // 64) * n)
    for kind in ("ei", "pi"):
        for largest in (True, False):
            value, best, idx = H.sgp_pathwise_acq(*ops, bd, scale=SCALE, acq=kind, largest=largest)
            sentinel = torch.full((n,), -7.25, dtype=dt, device="cuda")
            ws = torch.full((need + 64,), -7.25, dtype=torch.float64, device="cuda")
            none, best2, idx2 = H.sgp_pathwise_acq(*ops, bd, scale=SCALE, acq=kind, largest=largest, values=False, out=sentinel, ws=ws)
            torch.cuda.synchronize()
            assert value.shape == (n,) and value.dtype == dt and best.shape == (1,) and best.dtype == dt
            assert idx.shape == (1,) and idx.dtype == torch.int64
            got = value.cpu().numpy()
            ref = AR.mc_acq(F, b, kind, largest)
            assert np.all(np.isfinite(got)) and np.all(got >= 0)
            if kind == "pi":
                want = (AR.pi_count(F, b, largest) / S).astype(npt)
                print("sgp_pathwise_acq %s pi largest=%s %s: %d of %d columns differ from (T)(count / S)"
                      % (dtype, largest, shape, int((got != want).sum()), n))
                assert np.array_equal(got, want)
            elif dtype == "float64":
                err = np.abs(got - ref)
                print("sgp_pathwise_acq float64 ei largest=%s %s: max |value - ref| / ref %.3e, bound %.3e"
                      % (largest, shape, (err / np.where(ref > 0, ref, 1.0)).max(), ei_bound(S, 1.0)))
                assert np.all(err <= ei_bound(S, ref))
            else:
                want = ref.astype(np.float32)
                err = np.abs(got.astype(np.float64) - want.astype(np.float64))
                print("sgp_pathwise_acq float32 ei largest=%s %s: %.4f of the columns differ from fl32(ref), the largest by %.2f ulp"
                      % (largest, shape, float((got != want).mean()), float((err / np.spacing(np.abs(want)).astype(np.float64)).max())))
                assert np.all(err <= np.spacing(np.abs(want)).astype(np.float64))
            j = int(np.argmax(got))
            assert int(idx.cpu()[0]) == j and best.cpu().numpy()[0] == got[j]
            assert none is None and torch.equal(best2, best) and torch.equal(idx2, idx)
            assert bool((sentinel == -7.25).all()) and bool((ws[need:] == -7.25).all())


# ------------------------------------------------------------------------------------------------ 2. a function too
@pytest.mark.parametrize("S", [5, 65])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_an_acquisition_is_a_function_too(dtype, S):
    """x [300, 2] whole, twice, and in pieces of 1, 37, 128 and 134 points: the same bits of `value` (one tile of draws
    and two).  Then the maximiser's row is written a second time at a lower row (row 0; the last row if the maximiser is
    row 0 itself): the two values tie exactly and the lower row is reported."""
    dt = TORCH[dtype]
    ops = tuple(dev(a, dt) for a in PR.kernel_case(300, 40, 50, 2, S, 2, 8.0, seed=11))
    x, rest = ops[0], ops[1:]
    F = H.sgp_pathwise(*ops, scale=SCALE).cpu().numpy()
    bd = dev(np.quantile(F, 0.7, axis=1), dt)
    value, best, idx = H.sgp_pathwise_acq(*ops, bd, scale=SCALE)
    value2, best2, idx2 = H.sgp_pathwise_acq(*ops, bd, scale=SCALE)
    cuts = (0, 1, 38, 166, 300)
    pieces = [H.sgp_pathwise_acq(x[a:b].contiguous(), *rest, bd, scale=SCALE)[0] for a, b in zip(cuts[:-1], cuts[1:])]
    torch.cuda.synchronize()
    assert torch.equal(value, value2) and torch.equal(best, best2) and torch.equal(idx, idx2)
    assert torch.equal(value, torch.cat(pieces))
    assert float(value.max()) > 0.0
    j = int(idx.cpu()[0])
    other = 0 if j > 0 else 299
    x2 = x.clone()
    x2[other] = x[j]
    v2, b2, i2 = H.sgp_pathwise_acq(x2, *rest, bd, scale=SCALE)
    v2 = v2.cpu().numpy()
    print("tie %s S=%d: rows %d and %d -> %d" % (dtype, S, j, other, int(i2.cpu()[0])))
    assert v2[other] == v2[j] and v2[j] == value.cpu().numpy()[j]
    assert int(i2.cpu()[0]) == min(j, other) == int(np.argmax(v2)) and b2.cpu().numpy()[0] == v2[j]


# ------------------------------------------------------------------------------------------------ 3. edges
@pytest.mark.parametrize("S", [17, 130])
def test_acq_edges(S):
    """Incumbents above every value: value is 0 everywhere, idx 0, best 0.  One NaN row of x: that column is NaN, no
    other is, and it is never chosen.  Every row NaN: idx = -1 and best = -inf."""
    ops, F, b = _case((257, 33, 40, 2, 17) if S == 17 else (1000, 20, 24, 3, 130), "float64")
    x, rest = ops[0], ops[1:]
    n = x.shape[0]
    for kind in ("ei", "pi"):
        for largest, top in ((True, F.max() + 1.0), (False, F.min() - 1.0)):
            value, best, idx = H.sgp_pathwise_acq(*ops, dev(np.full(S, top), torch.float64), scale=SCALE, acq=kind, largest=largest)
            assert bool((value == 0).all()) and int(idx.cpu()[0]) == 0 and float(best.cpu()[0]) == 0.0
    bd = dev(b, torch.float64)
    value, _, idx = H.sgp_pathwise_acq(*ops, bd, scale=SCALE)
    j = int(idx.cpu()[0])
    xn = x.clone()
    xn[j, 0] = float("nan")
    vn, bn, jn = H.sgp_pathwise_acq(xn, *rest, bd, scale=SCALE)
    vn, ok = vn.cpu().numpy(), np.arange(n) != j
    assert np.isnan(vn[j]) and np.array_equal(vn[ok], value.cpu().numpy()[ok])
    assert int(jn.cpu()[0]) == int(np.nanargmax(vn)) != j and bn.cpu().numpy()[0] == np.nanmax(vn)
    va, ba, ja = H.sgp_pathwise_acq(torch.full_like(x, float("nan")), *rest, bd, scale=SCALE)
    assert bool(torch.isnan(va).all()) and int(ja.cpu()[0]) == -1 and float(ba.cpu()[0]) == -np.inf


def test_acq_refusals():
    """Unknown acq, kind = KERN_SQDIST, a NULL incumbent, NULL outputs and a NULL workspace are return codes of the entry
    (the outputs stay untouched); an unknown acq, a short or mistyped workspace, an incumbent of another shape and no
    candidates are ValueError in the wrapper."""
    dt = torch.float64
    ops = tuple(dev(a, dt) for a in PR.kernel_case(130, 8, 8, 1, 5, 1, 8.0, seed=3))
    x, omega, z, ell, coef = ops
    bd = dev(np.zeros(5), dt)
    value = torch.full((130,), -7.25, dtype=dt, device="cuda")
    best = torch.full((1,), -7.25, dtype=dt, device="cuda")
    idx = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ws = torch.zeros(H.sgp_pathwise_acq_ws_elems(130, 5), dtype=dt, device="cuda")
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    fn = _lib.lib().raw("hb_sgp_pathwise_acq_f64")

    def rc(kind=H.KERN_RBF, acq=0, inc=bd, val=value, bst=best, ix=idx, w=ws):
        return fn(kind, p(x), p(omega), p(z), p(ell), 1, p(coef), 1.0, acq, 1, p(inc), p(val), p(bst), p(ix), 130, 8, 8, 1, 5, p(w),
                  H.stream())

    for bad in (dict(acq=2), dict(acq=-1), dict(kind=H.KERN_SQDIST), dict(inc=None), dict(val=None, bst=None, ix=None),
                dict(ix=None), dict(w=None)):
        assert rc(**bad) != 0, bad
        assert _lib.lib().last_error()
    torch.cuda.synchronize()
    assert bool((value == -7.25).all()) and float(best.cpu()[0]) == -7.25 and int(idx.cpu()[0]) == -7
    assert rc() == 0 and rc(val=None) == 0 and rc(bst=None, ix=None) == 0
    for kw in (dict(acq="ucb"), dict(acq=7), dict(ws=ws[:1]), dict(ws=ws.float())):
        with pytest.raises(ValueError, match="sgp_pathwise_acq"):
            H.sgp_pathwise_acq(*ops, bd, **kw)
    for inc in (bd[:4].contiguous(), bd.reshape(5, 1), None):
        with pytest.raises(ValueError, match="incumbent"):
            H.sgp_pathwise_acq(*ops, inc)
    with pytest.raises(ValueError, match="candidate"):
        H.sgp_pathwise_acq(x[:0].contiguous(), omega, z, ell, coef, bd)


# ------------------------------------------------------------------------------------------------ 4. through the models
CAND = np.linspace(0.5, 15.5, 300)[:, None]
NS, Q = 65, 4
_MODEL = {}


def _model(kind, dtype):
    """A fitted 1-D model with N = 400, built once: SVGP (M = 32, q(u) from fit_q) or ExactGPR."""
    key = (kind, dtype)
    if key not in _MODEL:
        if kind == "svgp":
            X, y, Z = SR.problem(SR.GAUSSIAN, N=400)
            m = SVGP(X=X, Y=y, Z=Z, dtype=dtype)
            m.var = np.ones(1) * 0.09
            m.gp.kern.lengthscales = SR.ELL.copy()
            m.k_var = np.ones(1) * SR.K_VAR
            m.initialize()
            m.fit_q()
        else:
            X, Y, _ = svgp_data(400, 32, 0)
            m = ExactGPR(X=X, Y=Y, dtype=dtype)
            m.gp.kern.lengthscales = np.ones(1) * 1.2
            m.k_var = np.ones(1) * 0.8
            m.var = np.ones(1) * 0.09
            m.fit()
        _MODEL[key] = (m, X)
    return _MODEL[key]


@pytest.mark.parametrize("kind", ["svgp", "exact"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_models_suggest_a_batch(dtype, kind):
    """suggest_batch(300 candidates, q = 4, 65 draws of 64 features), steps = 0 and steps = 5."""
    m, Xtrain = _model(kind, dtype)
    cand = CAND.astype(NP[dtype])
    X, gains, info = m.suggest_batch(cand, Q, num_samples=NS, num_features=64, seed=2)
    draws, best, idx = info["draws"], info["best"], info["idx"]
    mean = m.predict_f(Xtrain, var=False)[0] if kind == "exact" else m.posterior().predict(Xtrain)[0]
    print("%s %s: incumbent %.6f, batch rows %s, gains %s" % (kind, dtype, best, idx, gains))
    assert best == float(np.max(mean)) and draws.num_samples == NS
    assert X.shape == (Q, 1) and gains.shape == (Q,) and gains.dtype == np.float64 and idx.dtype == np.int64
    assert np.array_equal(X, cand[idx]) and len(set(idx.tolist())) == Q
    assert np.all(np.diff(gains) <= 0.0) and np.all(gains > 0.0)
    F = draws(cand)
    assert gains[0] == draws.acquisition(cand, best=best).max()
    assert draws.acquisition_argmax(cand, best=best) == (idx[0], gains[0])
    jt = AR.joint(draws(X), best)
    bound = Q * ei_bound(NS, jt) + (Q * 2.0 ** -24 * gains[0] if dtype == "float32" else 0.0)
    print("%s %s: sum of gains %.17g, joint %.17g, difference %.3e, bound %.3e" % (kind, dtype, gains.sum(), jt, abs(gains.sum() - jt), bound))
    assert info["joint"] == float(np.sum(gains)) and abs(info["joint"] - jt) <= bound
    assert np.array_equal(info["incumbents"], np.maximum(NP[dtype](best), F[:, idx].max(1)))
    assert np.all(draws.acquisition(cand, best=info["incumbents"])[idx] == 0.0)       # a chosen point is worth nothing afterwards

    # steps = 5: every point is refined from its starting candidate
    X5, g5, info5 = m.suggest_batch(cand, Q, num_samples=NS, num_features=64, seed=2, steps=5)
    d5 = info5["draws"]
    assert X5.shape == (Q, 1) and X5.dtype == NP[dtype] and np.all(X5 >= cand.min()) and np.all(X5 <= cand.max())
    b = np.full(NS, best, NP[dtype])
    for k in range(Q):
        a = d5.acquisition(cand, best=b)
        start = a[info5["idx"][k]]
        fk = d5(X5[k:k + 1])[:, 0]
        ref = float(AR.mc_acq(fk[:, None], b)[0])
        # float32: the kernel's value is the double sum rounded once, half an ulp; the refined one is a float64 mean
        tol = ei_bound(NS, ref) + (0.5 * float(np.spacing(np.float32(ref))) if dtype == "float32" else 0.0)
        print("%s %s steps=5 point %d: start %.9g at row %d, gain %.9g, restated %.9g (difference %.3e, bound %.3e)"
              % (kind, dtype, k, start, info5["idx"][k], g5[k], ref, abs(g5[k] - ref), tol))
        assert info5["idx"][k] == int(np.argmax(a)) and g5[k] >= start
        assert abs(g5[k] - ref) <= tol
        b = np.maximum(b, fk)
    assert np.array_equal(info5["incumbents"], b)
