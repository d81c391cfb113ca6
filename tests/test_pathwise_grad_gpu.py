"""Maximising pathwise function draws on the GPU: hb_sgp_pathwise_grad and hb_sgp_pathwise_argmax against the numpy
restatements tests/pathwise_ref.py and tests/pathwise_grad_ref.py (pinned on the host by tests/test_pathwise_cpu.py and
tests/test_pathwise_grad_cpu.py), and PathwiseDraws.grad / argmax / maximise through the models.

fp64 bounds are fixed: 1e-11 of grad_scale[k] (pathwise_grad_ref.grad_scale bounds every partial sum of derivative k) for
the kernel -- the pathwise kernel's own bound carried over with the derivative's scale.  fp32 bounds are not constants: the
device's error against float64 arithmetic on the same rounded inputs is held to 4 x the error the float32 restatement
makes (as tests/test_pathwise_gpu.py does).  Everything said to be the same is compared bit for bit.  Every figure is
printed before it is asserted."""
import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd import hip_ops as H
from henbun_amd.models import SVGP, ExactGPR, svgp_data

import pathwise_grad_ref as GR
import pathwise_ref as PR
import sites_ref as SR

pytestmark = pytest.mark.gpu

TORCH = {"float64": torch.float64, "float32": torch.float32}
NP = {"float64": np.float64, "float32": np.float32}
SCALE = 1.7


def dev(a, dt):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


# ------------------------------------------------------------------------------------------------ 1. the gradient kernel
# (n, L, M, d, S): the shapes of tests/test_pathwise_grad_cpu.py -- one point; M = 0; ragged n, L and M against the strip of
# 128 and the K-step of 32 rows; d = 5 takes the dimensions in two groups; S = 17 crosses a row tile of 16 -- and S = 65,
# which crosses the 32 draws of a workgroup twice
SHAPES = [(1, 1, 0, 1, 1), (70, 33, 0, 1, 3), (257, 64, 96, 2, 5), (1000, 130, 160, 3, 17), (300, 16, 40, 5, 2), (130, 8, 8, 1, 65)]
CASES = [s + (dl,) for s in SHAPES for dl in sorted({1, s[3]})]
_CASE = {}


def _case(shape, dtype):
    """Inputs rounded to the dtype, the float64 gradient on them, its scale and (float32) the restatement's error per
    dimension: computed once."""
    key = (shape, dtype)
    if key not in _CASE:
        n, L, M, d, S, dl = shape
        arrs = PR.kernel_case(n, L, M, d, S, dl, 8.0, seed=n + L + M + d + S + dl)
        x, omega, z, ell, coef = (None if a is None else a.astype(NP[dtype]) for a in arrs)
        ref = GR.grad(x, omega, z, ell, coef, SCALE)
        gs = GR.grad_scale(x, omega, z, ell, coef, SCALE)
        rerr = None
        if dtype == "float32":
            rerr = np.abs(GR.grad(x, omega, z, ell, coef, SCALE, dtype=np.float32) - ref).max((0, 1))
        _CASE[key] = (x, omega, z, ell, coef, ref, gs, rerr)
    return _CASE[key]


@pytest.mark.parametrize("shape", CASES, ids=lambda s: "n%d-L%d-M%d-d%d-S%d-dl%d" % s)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_grad_kernel_against_the_restatement(dtype, shape):
    """hb_sgp_pathwise_grad_f64 / _f32 with scale = 1.7 and a mixed-sign coef whose trailing M entries are about 1e3; its
    `out` is hb_sgp_pathwise's bit for bit; values=False leaves a sentinel-filled out untouched and returns the same
    grad.  Observed on MI355X: see DESIGN.md 3, "Maximising function draws"."""
    dt = TORCH[dtype]
    x, omega, z, ell, coef, ref, gs, rerr = _case(shape, dtype)
    n, L, M, d, S, dl = shape
    xd, od, zd, ed, cd = (dev(a, dt) for a in (x, omega, z, ell, coef))
    out, grad = H.sgp_pathwise_grad(xd, od, zd, ed, cd, scale=SCALE)
    want = H.sgp_pathwise(xd, od, zd, ed, cd, scale=SCALE)
    sentinel = torch.full((S, n), -7.25, dtype=dt, device="cuda")
    none, grad2 = H.sgp_pathwise_grad(xd, od, zd, ed, cd, scale=SCALE, out=sentinel, values=False)
    torch.cuda.synchronize()
    assert grad.shape == (S, n, d) and grad.dtype == dt and out.shape == (S, n)
    assert torch.equal(out, want)
    assert none is None and torch.equal(grad2, grad) and bool((sentinel == -7.25).all())
    got = grad.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got))
    err = np.abs(got - ref).max((0, 1))
    if dtype == "float64":
        print("sgp_pathwise_grad float64 %s: max error per dimension %s of grad_scale %s" % (shape, err / gs, gs))
        assert np.all(err <= 1e-11 * gs)
        return
    print("sgp_pathwise_grad float32 %s: device %s, float32 restatement %s (%s x); grad_scale %s"
          % (shape, err, rerr, err / np.maximum(rerr, 1e-300), gs))
    assert np.all(err <= 4.0 * rerr)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_a_gradient_is_a_function_too(dtype):
    """x [300, 2] whole, twice, in pieces of 1, 37, 128 and 134 points, and with draws 3 and 1 alone: the same bits of
    `out` and `grad` -- strip boundaries, ragged tails and row tiles fall elsewhere in every form."""
    dt = TORCH[dtype]
    arrs = PR.kernel_case(300, 40, 50, 2, 5, 2, 8.0, seed=11)
    xd, od, zd, ed, cd = (dev(a, dt) for a in arrs)
    out, grad = H.sgp_pathwise_grad(xd, od, zd, ed, cd, scale=SCALE)
    out2, grad2 = H.sgp_pathwise_grad(xd, od, zd, ed, cd, scale=SCALE)
    cuts = (0, 1, 38, 166, 300)
    pieces = [H.sgp_pathwise_grad(xd[a:b].contiguous(), od, zd, ed, cd, scale=SCALE) for a, b in zip(cuts[:-1], cuts[1:])]
    sub = torch.as_tensor([3, 1], device="cuda")
    outs, grads = H.sgp_pathwise_grad(xd, od, zd, ed, cd[sub].contiguous(), scale=SCALE)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(grad, grad2)
    assert torch.equal(out, torch.cat([p[0] for p in pieces], dim=1)) and torch.equal(grad, torch.cat([p[1] for p in pieces], dim=1))
    assert torch.equal(outs, out[sub]) and torch.equal(grads, grad[sub])
    assert float(grad.abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------ 2. arg-max
_AM = {}


def _am_case(n, S, dtype):
    """Candidates on the device and the values hb_sgp_pathwise stores for them (numpy): computed once."""
    key = (n, S, dtype)
    if key not in _AM:
        dt = TORCH[dtype]
        ops = tuple(dev(a, dt) for a in PR.kernel_case(n, 33, 40, 2, S, 2, 8.0, seed=n + S))
        _AM[key] = (ops, H.sgp_pathwise(*ops, scale=SCALE).cpu().numpy())
    return _AM[key]


@pytest.mark.parametrize("S", [1, 17, 65])
@pytest.mark.parametrize("n", [1, 127, 129, 1000, 4099])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_argmax_is_numpys_on_the_values_of_evaluate(dtype, n, S):
    """n on both sides of one strip of 128 and over 33 strips; S crossing a row tile and the 64 draws of a workgroup.
    idx is np.argmax of the [S, n] values hb_sgp_pathwise writes, best the value there, bit for bit; largest=False
    mirrors np.argmin; two calls return the same bits."""
    ops, F = _am_case(n, S, dtype)
    for largest, arg in ((True, np.argmax), (False, np.argmin)):
        best, idx = H.sgp_pathwise_argmax(*ops, scale=SCALE, largest=largest)
        best2, idx2 = H.sgp_pathwise_argmax(*ops, scale=SCALE, largest=largest)
        torch.cuda.synchronize()
        assert best.shape == (S,) and idx.shape == (S,) and idx.dtype == torch.int64 and best.dtype == TORCH[dtype]
        want = arg(F, axis=1)
        assert np.array_equal(idx.cpu().numpy(), want)
        assert np.array_equal(best.cpu().numpy(), F[np.arange(S), want])
        assert torch.equal(best, best2) and torch.equal(idx, idx2)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_argmax_ties_go_to_the_lowest_column(dtype):
    """n = 1000, S = 17: the candidate at which draw 0 is largest is written a second time into another strip -- before
    the original if that sits beyond the first strip, behind it otherwise -- and the same for draw 1's minimum.  A draw
    is a function, so the two copies tie exactly: the lower row is reported, as np.argmax does."""
    ops, F = _am_case(1000, 17, dtype)
    x = ops[0].clone()
    for largest, arg, s in ((True, np.argmax, 0), (False, np.argmin, 1)):
        j = int(arg(F[s]))
        other = 5 if j >= 128 else 900
        x2 = x.clone()
        x2[other] = x[j]
        F2 = H.sgp_pathwise(x2, *ops[1:], scale=SCALE).cpu().numpy()
        assert F2[s, other] == F2[s, j] and other // 128 != j // 128
        best, idx = H.sgp_pathwise_argmax(x2, *ops[1:], scale=SCALE, largest=largest)
        idx, best = idx.cpu().numpy(), best.cpu().numpy()
        print("tie %s: draw %d rows %d and %d -> %d" % (dtype, s, j, other, idx[s]))
        assert idx[s] == min(j, other)
        assert np.array_equal(idx, arg(F2, axis=1)) and np.array_equal(best, F2[np.arange(17), idx])


def test_argmax_never_chooses_a_nan():
    """A NaN coordinate makes every draw NaN at that candidate: it is passed over; with nothing else to choose from the
    draw reports idx = -1 and best = -inf (largest) / +inf."""
    ops, F = _am_case(129, 17, "float64")
    x = ops[0].clone()
    j = int(np.argmax(F[0]))
    x[j, 0] = float("nan")
    F2 = H.sgp_pathwise(x, *ops[1:], scale=SCALE).cpu().numpy()
    assert np.all(np.isnan(F2[:, j]))
    best, idx = H.sgp_pathwise_argmax(x, *ops[1:], scale=SCALE)
    assert np.array_equal(idx.cpu().numpy(), np.nanargmax(F2, axis=1)) and np.array_equal(best.cpu().numpy(), np.nanmax(F2, axis=1))
    for largest, inf in ((True, -np.inf), (False, np.inf)):
        best, idx = H.sgp_pathwise_argmax(x[j:j + 1].contiguous(), *ops[1:], scale=SCALE, largest=largest)
        assert np.all(idx.cpu().numpy() == -1) and np.all(best.cpu().numpy() == inf)


# ------------------------------------------------------------------------------------------------ 3. through the models
_MODEL = {}


def _draws(kind, dtype):
    """S = 5 draws with 64 features of a fitted 1-D model, built once: SVGP (Gaussian, M = 32, mean-field q from fit_q,
    the case of tests/test_pathwise_gpu.py) or ExactGPR (N = 400: the case of test_exact_gpr_predicts_in_data_units)."""
    key = (kind, dtype)
    if key not in _MODEL:
        if kind == "svgp":
            X, y, Z = SR.problem(SR.GAUSSIAN)
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
        _MODEL[key] = (m, m.sample_functions(5, num_features=64, seed=2))
    return _MODEL[key]


def _ref_ops(draws):
    return tuple(np.asarray(a, np.float64) for a in (draws.omega, draws.z, draws.lengthscales, draws.coef)) + (draws.scale,)


CAND = np.linspace(0.5, 15.5, 41)[:, None]
FD_H = 1e-4


@pytest.mark.parametrize("kind", ["svgp", "exact"])
def test_model_gradients_are_the_derivatives_of_the_draws(kind):
    """float64: draws.grad(X) against central differences of draws(X) with h = 1e-4, within 1e-6 max|grad|.  Both come
    from the restatement on the same case: the truncation is h^2 / 6 |f'''|, about 1e-8 of max|grad| for frequencies
    and inverse lengthscales of order 1 to 3, and the rounding 2^-53 sum|coef| / h stays below 1e-7 of it while the
    update's coefficients are below 1e5; the restatement's own central difference, printed beside the device's, shows
    both.  grad also is the restatement's gradient to 1e-11 grad_scale (the kernel's bound)."""
    m, draws = _draws(kind, "float64")
    assert isinstance(draws, hb.gp.PathwiseDraws)
    omega, z, ell, coef, scale = _ref_ops(draws)
    g = draws.grad(CAND)
    f, gd = draws.evaluate_grad(CAND)
    assert g.shape == (5, 41, 1) and np.array_equal(g, gd.cpu().numpy()) and np.array_equal(f.cpu().numpy(), draws(CAND))
    fd = (draws(CAND + FD_H) - draws(CAND - FD_H)) / (2.0 * FD_H)
    ref = GR.grad(CAND, omega, z, ell, coef, scale)
    rfd = (PR.evaluate(CAND + FD_H, omega, z, ell, coef, scale) - PR.evaluate(CAND - FD_H, omega, z, ell, coef, scale)) / (2.0 * FD_H)
    gmax, gs = np.abs(ref).max(), GR.grad_scale(CAND, omega, z, ell, coef, scale)[0]
    e_fd, e_rfd, e_ref = np.abs(fd - g[:, :, 0]).max(), np.abs(rfd - ref[:, :, 0]).max(), np.abs(g - ref).max()
    print("%s float64: grad against central differences %.3e of max|grad| %.3e (the restatement's own: %.3e); against the "
          "restatement %.3e of grad_scale %.3e; max|coef| %.3e"
          % (kind, e_fd / gmax, gmax, e_rfd / gmax, e_ref / gs, gs, np.abs(coef).max()))
    assert e_rfd <= 1e-6 * gmax
    assert e_fd <= 1e-6 * gmax
    assert e_ref <= 1e-11 * gs


@pytest.mark.parametrize("kind", ["svgp", "exact"])
def test_model_maximise_follows_the_restatement(kind):
    """float64, 41 candidates on [0.5, 15.5]: argmax is np.argmax of draws(X); maximise (defaults, then a box that cuts
    the domain, then the minimum) reproduces the restatement's x_best within 1e-8; f_best >= start_value, f_best is the
    diagonal of evaluate(x_best) bit for bit, x_best lies in the box; steps=0 returns the arg-max candidate itself."""
    m, draws = _draws(kind, "float64")
    ops = _ref_ops(draws)
    F = draws(CAND)
    idx, val = draws.argmax(CAND)
    assert idx.dtype == np.int64 and np.array_equal(idx, F.argmax(1)) and np.array_equal(val, F.max(1))
    idx_min, val_min = draws.argmax(CAND, largest=False)
    assert np.array_equal(idx_min, F.argmin(1)) and np.array_equal(val_min, F.min(1))
    x0, f0, info = draws.maximise(CAND, steps=0)
    assert np.array_equal(x0, CAND[idx]) and np.array_equal(f0, val) and info["steps"] == 0
    assert np.array_equal(info["start_idx"], idx) and np.array_equal(info["start_value"], val)
    for bounds, largest in ((None, True), ((np.array([4.0]), np.array([9.0])), True), (None, False)):
        X = CAND if bounds is None else CAND[(CAND[:, 0] >= 4.0) & (CAND[:, 0] <= 9.0)]
        xb, fb, info = draws.maximise(X, bounds=bounds, largest=largest)
        rx, rf, ridx = GR.maximise(X, *ops, steps=50, lr=0.05, bounds=bounds, largest=largest)
        sign = 1.0 if largest else -1.0
        lo, hi = (X.min(0), X.max(0)) if bounds is None else bounds
        print("%s maximise(bounds=%s, largest=%s): x_best within %.3e of the restatement's, f_best within %.3e; gain over "
              "the candidates %s" % (kind, bounds is not None, largest, np.abs(xb - rx).max(), np.abs(fb - rf).max(),
                                     sign * (fb - info["start_value"])))
        assert xb.shape == (5, 1) and fb.shape == (5,) and info["steps"] == 50
        assert np.array_equal(info["start_idx"], ridx)
        assert np.abs(xb - rx).max() <= 1e-8
        assert np.all(sign * fb >= sign * info["start_value"])
        assert np.all(xb >= lo) and np.all(xb <= hi)
        diag = draws.evaluate(xb).cpu().numpy()[np.arange(5), np.arange(5)]
        assert np.array_equal(fb, diag)
    # a box that excludes the peak: two candidates strictly inside [7, 7.15], a seventh of a lengthscale wide, on which a
    # draw is monotone unless an extremum happens to fall inside.  The ascent runs into a face, the projection holds
    # every further iterate there, and the best point seen IS the face, exactly -- for every draw for which the
    # restatement says so (at least one must)
    lo, hi = np.array([7.0]), np.array([7.15])
    X = np.array([[7.05], [7.1]])
    xb, fb, info = draws.maximise(X, bounds=(lo, hi))
    rx, rf, _ = GR.maximise(X, *ops, steps=50, lr=0.05, bounds=(lo, hi))
    on = ((rx == lo) | (rx == hi))[:, 0]
    print("%s maximise in a box without the peak: x_best %s, on a face %s, within %.3e of the restatement's"
          % (kind, xb[:, 0], on, np.abs(xb - rx).max()))
    assert on.any() and np.array_equal(xb[on], rx[on])
    assert np.abs(xb - rx).max() <= 1e-8 and np.all(xb >= lo) and np.all(xb <= hi)
    assert np.all(fb >= info["start_value"])


def test_maximise_in_a_float32_session():
    """One float32 run (SVGP): finite, never worse than the start, and f_best is evaluate(x_best) on the diagonal."""
    m, draws = _draws("svgp", "float32")
    xb, fb, info = draws.maximise(CAND)
    print("float32 maximise: gain over the candidates %s" % (fb - info["start_value"]))
    assert xb.dtype == np.float32 and fb.dtype == np.float32
    assert np.all(np.isfinite(xb)) and np.all(np.isfinite(fb)) and np.all(fb >= info["start_value"])
    assert np.array_equal(fb, draws.evaluate(xb).cpu().numpy()[np.arange(5), np.arange(5)])
    assert np.all(xb >= CAND.min()) and np.all(xb <= CAND.max())


def test_maximise_refuses_bad_arguments():
    m, draws = _draws("svgp", "float64")
    for kw in (dict(steps=-1), dict(lr=0.0), dict(lr=-0.1), dict(bounds=(np.zeros(2), np.ones(2))), dict(bounds=(np.zeros(1),)),
               dict(bounds=(np.array([2.0]), np.array([1.0])))):
        with pytest.raises(ValueError, match="maximise"):
            draws.maximise(CAND, **kw)
    for fn in (draws.maximise, draws.argmax, draws.grad, draws.evaluate_grad):
        with pytest.raises(ValueError):
            fn(np.zeros((4, 2)))
