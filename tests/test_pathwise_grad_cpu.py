"""Maximising pathwise function draws on the host: the new C entries exist, are bound, wrapped and validate their arguments
before any launch, and the numpy restatement the GPU tests lean on (tests/pathwise_grad_ref.py) is pinned twice -- its
gradient against central differences of pathwise_ref.evaluate, its maximise on a single bump whose peak is known.  No HIP
kernel runs here.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import pathwise_grad_ref as GR
import pathwise_ref as PR

NEW = ("hb_sgp_pathwise_grad_f32", "hb_sgp_pathwise_grad_f64", "hb_sgp_pathwise_argmax_f32", "hb_sgp_pathwise_argmax_f64",
       "hb_sgp_pathwise_argmax_ws_elems")


# ---------------------------------------------------------------- C ABI
def test_pathwise_grad_symbols_are_exported_bound_and_wrapped():
    import os

    import henbun_amd as hb
    from henbun_amd import _lib, hip_ops as H

    names = _lib.declared_symbols()
    lib = _lib.lib()
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "henbun_hip.h")).read()
    for n in NEW:
        assert n in names and n + "(" in header
        assert lib.raw(n) is not None
    assert lib.raw("hb_version")() == 2
    for f in ("sgp_pathwise_grad", "sgp_pathwise_argmax", "sgp_pathwise_argmax_ws_elems"):
        assert callable(getattr(H, f))
    for m in ("evaluate_grad", "grad", "argmax", "maximise"):
        assert callable(getattr(hb.gp.PathwiseDraws, m))
    # in elements of the dtype, O(S n / 128)
    ws = lib.raw("hb_sgp_pathwise_argmax_ws_elems")
    assert ws(1, 1) >= 1 and ws(1000000, 64) <= 4 * 64 * (1000000 // 128 + 1)


def _grad_call(lib, suffix, **bad):
    a = dict(kind=0, x=1, omega=1, z=1, ell=1, dl=1, coef=1, scale=1.0, out=1, grad=1, n=100, L=8, M=4, d=1, S=2)
    a.update(bad)
    return lib.raw("hb_sgp_pathwise_grad" + suffix)(a["kind"], a["x"], a["omega"], a["z"], a["ell"], a["dl"], a["coef"], a["scale"],
                                                    a["out"], a["grad"], a["n"], a["L"], a["M"], a["d"], a["S"], None)


def _argmax_call(lib, suffix, **bad):
    a = dict(kind=0, x=1, omega=1, z=1, ell=1, dl=1, coef=1, scale=1.0, largest=1, best=1, idx=1, n=100, L=8, M=4, d=1, S=2, ws=1)
    a.update(bad)
    return lib.raw("hb_sgp_pathwise_argmax" + suffix)(a["kind"], a["x"], a["omega"], a["z"], a["ell"], a["dl"], a["coef"],
                                                      a["scale"], a["largest"], a["best"], a["idx"], a["n"], a["L"], a["M"],
                                                      a["d"], a["S"], a["ws"], None)


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
@pytest.mark.parametrize("bad, word", [
    (dict(kind=1), "UnitRBF"),
    (dict(L=0), "extents"),
    (dict(S=0), "extents"),
    (dict(n=-1), "extents"),
    (dict(dl=2, d=3), "lengthscales"),
    (dict(grad=None), "NULL"),
    (dict(coef=None), "NULL"),
    (dict(n=1 << 20, S=1 << 9, d=4), "too large"),       # S n below 2^31, S n d not
])
def test_grad_entry_points_reject_bad_arguments(suffix, bad, word):
    """(the pointers are the integer 1: any launch would fault -- every case must return before one)"""
    from henbun_amd import _lib

    lib = _lib.lib()
    rc = _grad_call(lib, suffix, **bad)
    assert rc < 0 and word in lib.last_error() and "hb_sgp_pathwise_grad" in lib.last_error(), (rc, lib.last_error())


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
@pytest.mark.parametrize("bad, word", [
    (dict(kind=1), "UnitRBF"),
    (dict(L=0), "extents"),
    (dict(S=0), "extents"),
    (dict(n=-1), "extents"),
    (dict(n=0), "extents"),
    (dict(dl=2, d=3), "lengthscales"),
    (dict(best=None), "NULL"),
    (dict(idx=None), "NULL"),
    (dict(ws=None), "workspace"),
])
def test_argmax_entry_points_reject_bad_arguments(suffix, bad, word):
    from henbun_amd import _lib

    lib = _lib.lib()
    rc = _argmax_call(lib, suffix, **bad)
    assert rc < 0 and word in lib.last_error() and "hb_sgp_pathwise_argmax" in lib.last_error(), (rc, lib.last_error())


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
def test_grad_of_no_points_is_not_an_error_and_not_a_launch(suffix):
    from henbun_amd import _lib

    assert _grad_call(_lib.lib(), suffix, n=0, M=0, z=None) == 0
    assert _grad_call(_lib.lib(), suffix, n=0, out=None) == 0


# ---------------------------------------------------------------- the restatement
SHAPES = [(1, 1, 0, 1, 1), (70, 33, 0, 1, 3), (257, 64, 96, 2, 5), (1000, 130, 160, 3, 17), (300, 16, 40, 5, 2)]
CASES = [s + (dl,) for s in SHAPES for dl in sorted({1, s[3]})]


@pytest.mark.parametrize("shape", CASES, ids=lambda s: "n%d-L%d-M%d-d%d-S%d-dl%d" % s)
def test_the_gradient_of_the_restatement_is_the_derivative_of_the_value(shape):
    """Central differences (h = 1e-5) of pathwise_ref.evaluate in float64, one coordinate at a time, against
    pathwise_grad_ref.grad within 1e-9 grad_scale[k]: the truncation h^2 / 6 |f'''| and the rounding 2^-53 |f| / h are
    both of order 1e-11 of the scale.  Observed worst over the cases: 4.6e-11."""
    n, L, M, d, S, dl = shape
    x, omega, z, ell, coef = PR.kernel_case(n, L, M, d, S, dl, 8.0, seed=n + L + M + d + S + dl)
    scale, h = 1.7, 1e-5
    g = GR.grad(x, omega, z, ell, coef, scale)
    gs = GR.grad_scale(x, omega, z, ell, coef, scale)
    assert g.shape == (S, n, d) and gs.shape == (d,)
    for k in range(d):
        e = np.zeros(d)
        e[k] = h
        fd = (PR.evaluate(x + e, omega, z, ell, coef, scale) - PR.evaluate(x - e, omega, z, ell, coef, scale)) / (2.0 * h)
        err = float(np.abs(fd - g[:, :, k]).max())
        print("restatement gradient %s k=%d: %.3e = %.3e of grad_scale %.3e; max|grad| %.3e"
              % (shape, k, err, err / gs[k], gs[k], np.abs(g[:, :, k]).max()))
        assert np.abs(g[:, :, k]).max() <= gs[k]
        assert err <= 1e-9 * gs[k]


def test_the_float32_restatement_follows_the_float64_one():
    """The float32 form (operands and blocked sum in float32) against float64 on the rounded inputs: an error of float32
    size, 1e-5 of grad_scale at most -- it is the yardstick of the device's float32 error, not a second implementation."""
    x, omega, z, ell, coef = (a.astype(np.float32) for a in PR.kernel_case(257, 64, 96, 2, 5, 2, 8.0, seed=3))
    g64, g32 = GR.grad(x, omega, z, ell, coef, 1.7), GR.grad(x, omega, z, ell, coef, 1.7, dtype=np.float32)
    gs = GR.grad_scale(x, omega, z, ell, coef, 1.7)
    err = np.abs(g32 - g64).max((0, 1)) / gs
    print("float32 restatement of the gradient: %s of grad_scale" % err)
    assert np.all(err > 0) and np.all(err <= 1e-5)


@pytest.mark.parametrize("steps", [50, 100])
@pytest.mark.parametrize("ell", [0.8, 1.3])
def test_the_restatements_maximise_climbs_a_single_bump(ell, steps):
    """M = 1, all trig coefficients 0, coef = 2.5: f(x) = 2.5 exp(-(x - z0)^2 / (2 ell^2)) with its maximum at z0 = 4.
    From one candidate at z0 + off ell, |off| <= 0.5, in the box [0, 8], x_best ends within 0.025 ell of z0 (half a step
    of lr = 0.05) and f_best is f(x_best) >= the start's value.  Simulated worst: 0.0031 ell."""
    z0 = 4.0
    omega, z, coef = np.ones((1, 1)), np.array([[z0]]), np.array([[0.0, 0.0, 2.5]])
    worst = 0.0
    for off in (-0.5, -0.3, -0.05, 0.0, 0.2, 0.5):
        x = np.array([[z0 + off * ell]])
        xb, fb, idx = GR.maximise(x, omega, z, np.array([ell]), coef, 1.0, steps=steps, lr=0.05, bounds=(np.zeros(1), 8.0 * np.ones(1)))
        worst = max(worst, abs(xb[0, 0] - z0) / ell)
        assert idx[0] == 0 and fb[0] >= 2.5 * np.exp(-0.5 * off * off) and fb[0] <= 2.5
        assert fb[0] == PR.evaluate(xb, omega, z, np.array([ell]), coef, 1.0)[0, 0]
    print("single bump, ell = %.1f, %d steps: x_best within %.4f ell of the maximum" % (ell, steps, worst))
    assert worst <= 0.025


def test_the_restatements_maximise_keeps_the_start_and_the_box():
    """steps = 0 returns the best candidate of every draw; largest=False mirrors it; a box that excludes the peak holds
    the iterate on its face."""
    x, omega, z, ell, coef = PR.kernel_case(50, 8, 6, 2, 3, 2, 4.0, seed=9)
    F = PR.evaluate(x, omega, z, ell, coef)
    xb, fb, idx = GR.maximise(x, omega, z, ell, coef, steps=0)
    assert np.array_equal(idx, F.argmax(1)) and np.array_equal(xb, x[idx]) and np.array_equal(fb, F.max(1))
    xb, fb, idx = GR.maximise(x, omega, z, ell, coef, steps=0, largest=False)
    assert np.array_equal(idx, F.argmin(1)) and np.array_equal(fb, F.min(1))
    xb, fb, idx = GR.maximise(x, omega, z, ell, coef, steps=30)
    assert np.all(fb >= F.max(1)) and np.all(xb >= x.min(0)) and np.all(xb <= x.max(0))
    bump = (np.ones((1, 1)), np.array([[4.0]]), np.array([1.0]), np.array([[0.0, 0.0, 2.5]]))
    xb, fb, _ = GR.maximise(np.array([[3.0]]), *bump, steps=60, bounds=(np.array([2.0]), np.array([3.5])))
    assert xb[0, 0] == 3.5
