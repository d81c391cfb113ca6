"""Input gradient of the collapsed bound on the host: the numpy restatement the GPU tests lean on
(tests/kgrad_x_ref.py) against torch.autograd in float64, its translation invariance against the z gradient, and the
four new C entries: declared, exported, bound, and refusing bad arguments before any launch.  No HIP kernel runs here.

Bounds.  Restatement against autograd: xbar carries the weights Q = 2 W^T G W, R = W^T g^T, hence W = Lm^-1 twice, whose
rounding error is of relative order eps cond(Kmm) <= eps M / jitter and enters every term at the term's own size: 8 eps
(M / jitter) x the sum of the absolute terms (kgrad_x_ref.abs_scale) -- the rule of test_collapsed_grad_cpu.py.
Observed: <= 3.3e-14 of that sum.  Translation invariance: K depends on z - x alone, so sum_j xbar_j = -sum_i
zbar_streamed_i up to the rounding of two sums of N M terms: 4 (N + M) 2^-53 x the sum of all absolute terms."""
import numpy as np
import pytest

import collapsed_grad_ref as C
import elbo_grad_ref as E
import kgrad_x_ref as KX

JITTER = 1e-5
CASES = [(residual, N, M, d, P) for residual in ("diagonal", "neglected")
         for N, M, d, P in ((1, 32, 1, 1), (97, 32, 3, 2), (97, 50, 1, 2), (4099, 96, 3, 1))]


@pytest.mark.parametrize("residual, N, M, d, P", CASES)
def test_restatement_against_autograd_and_translation_invariance(residual, N, M, d, P):
    X, Y, z, ell = C.case(N, M, d, P, seed=N + M + d + P)
    r = C.bound_and_grad(X, Y, z, ell, JITTER, 0.09, 1.3, residual)
    xb = KX.streamed_x(X, Y, z, ell, r["Q"], r["R"])
    xa = KX.bound_autograd_x(X, Y, z, ell, JITTER, 0.09, 1.3, residual)
    sc = KX.abs_scale(X, Y, z, ell, r["Q"], r["R"])
    assert xb.shape == (N, d) and xa.shape == (N, d)
    gap, scale = np.abs(xb - xa).max(), sc.max()
    inv = np.abs(xb.sum(0) + r["z_streamed"].sum(0)).max()
    print("%s N=%d M=%d d=%d P=%d: max|xbar| %.3e, gap to autograd %.3e (%.1e of the abs-scale %.3e); |sum_j xbar_j + "
          "sum_i zbar_i| %.3e (sum of all absolute terms %.3e)" % (residual, N, M, d, P, np.abs(xa).max(), gap, gap / scale,
                                                                 scale, inv, sc.sum(0).max()))
    assert gap <= 8.0 * np.finfo(np.float64).eps * M / JITTER * scale
    assert inv <= 4.0 * (N + M) * 2.0 ** -53 * sc.sum(0).max()


def test_weighted_restatement_against_the_fixed_weight_surrogate():
    """streamed_x_w against autograd of the surrogate whose dK is Kbar, for drawn w (both signs, exact zeros) and r; with
    w = 1, r = Y it is streamed_x.  Both sides use the SAME Q, R: 4 gamma x the abs-scale."""
    N, M, d = 97, 32, 3
    X, Y, z, ell = C.case(N, M, d, 1, seed=5)
    r = C.bound_and_grad(X, Y, z, ell, JITTER, 0.09, 1.0)
    w, rr = E.weights_case(N, 3)
    xb = KX.streamed_x_w(X, w, rr, z, ell, r["Q"], r["R"])
    xa = KX.surrogate_autograd_x(X, w, rr, z, ell, r["Q"], r["R"])
    scale = KX.abs_scale(X, rr[:, None], z, ell, r["Q"], r["R"], w=w).max()
    print("weighted: gap %.3e, abs-scale %.3e" % (np.abs(xb - xa).max(), scale))
    assert np.abs(xb - xa).max() <= 4.0 * KX.gamma(M, 1) * scale
    assert np.array_equal(KX.streamed_x_w(X, np.ones(N), Y[:, 0], z, ell, r["Q"], r["R"]),
                          KX.streamed_x(X, Y, z, ell, r["Q"], r["R"]))


# ---------------------------------------------------------------- C ABI
ENTRIES = ["hb_sgp_kgrad_x_f32", "hb_sgp_kgrad_x_f64", "hb_sgp_wkgrad_x_f32", "hb_sgp_wkgrad_x_f64"]


def test_kgrad_x_symbols_are_declared_exported_and_bound():
    import os

    from henbun_amd import _lib

    names = _lib.declared_symbols()
    lib = _lib.lib()
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "henbun_hip.h")).read()
    for n in ENTRIES:
        assert n in names and n + "(" in header
        assert lib.raw(n) is not None
    assert lib.raw("hb_version")() == 2


def _call(lib, entry, **kw):
    a = dict(kind=0, X=1, Y=1, w=1, r=1, z=1, ell=1, dl=1, Q=1, R=1, zbar=1, ellbar=1, xbar=1, N=100, M=64, d=1, P=1, ws=1 << 20)
    a.update(kw)
    if "wkgrad" in entry:
        return lib.raw(entry)(a["kind"], a["X"], a["w"], a["r"], a["z"], a["ell"], a["dl"], a["Q"], a["R"], a["zbar"],
                              a["ellbar"], a["xbar"], a["N"], a["M"], a["d"], a["ws"], None)
    return lib.raw(entry)(a["kind"], a["X"], a["Y"], a["z"], a["ell"], a["dl"], a["Q"], a["R"], a["zbar"], a["ellbar"],
                          a["xbar"], a["N"], a["M"], a["d"], a["P"], a["ws"], None)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("bad, word", [
    (dict(xbar=None), "NULL output"),
    (dict(zbar=None), "NULL output"),
    (dict(kind=1), "UnitRBF"),
    (dict(dl=2, d=3), "lengthscales"),
    (dict(dl=0), "lengthscales"),
    (dict(X=None), "NULL input"),
    (dict(N=0), "extents"),
    (dict(ws=None), "workspace"),
])
def test_kgrad_x_entry_points_reject_bad_arguments(entry, bad, word):
    """(the pointers are small integers: any launch would fault -- every case must return before one; the workspace
    pointer of the other cases is 16-byte aligned so that only the case that clears it trips that check)"""
    from henbun_amd import _lib

    lib = _lib.lib()
    rc = _call(lib, entry, **bad)
    assert rc < 0 and word in lib.last_error() and entry[:-4] in lib.last_error(), (rc, lib.last_error())
