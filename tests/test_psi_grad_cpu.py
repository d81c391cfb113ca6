"""Gradients of the psi statistics on the host: the new C entries exist and are bound, refuse bad arguments before any
launch and ask for a workspace that does not grow with N; and the numpy restatement the GPU tests lean on
(tests/psi_grad_ref.py) is pinned by an independent torch.autograd evaluation of the same bound, by the certain-input
streamed gradient at zero variance and by a central difference of the bound.  No HIP kernel runs here.

Observed (printed by the tests): against autograd, worst over the cases, value 3.6e-12, X_mean 8.8e-13, X_var 1.5e-12,
z 5.8e-10 (d = 1, P = 3, 'neglected': inducing points half a lengthscale apart; 1.3e-11 with 'diagonal', below 3e-12 in
d = 2, 3), lengthscales 5.2e-11, noise_var 7.8e-12, k_var 5.3e-11 relative; zero variance zbar 4.7e-14, ellbar 1.9e-14 of the
largest entry; central difference 2.9e-8 (without the KL) and 2.9e-9 (with it) relative."""
import numpy as np
import pytest

import collapsed_grad_ref as CG
import psi_grad_ref as PG

ENTRIES = ("hb_sgp_psi_grad_f32", "hb_sgp_psi_grad_f64", "hb_sgp_psi_grad_ws_elems")
JITTER = 1e-3


# ---------------------------------------------------------------- C ABI
def test_psi_grad_symbols_are_declared_exported_and_bound():
    from henbun_amd import _lib
    from henbun_amd import hip_ops as H

    names = _lib.declared_symbols()
    lib = _lib.lib()
    for n in ENTRIES:
        assert n in names
        assert lib.raw(n) is not None
    for w in ("sgp_psi_grad", "sgp_psi_grad_ws_elems"):
        assert callable(getattr(H, w))
    assert lib.raw("hb_version")() == 2


def _grad_call(lib, suffix, **kw):
    a = dict(kind=0, Xm=1, Xv=1, Y=1, z=1, ell=1, dl=1, Q=1, R=1, mubar=1, sbar=1, zbar=1, ellbar=1, N=100, M=64, d=1, P=1,
             ws=None)
    a.update(kw)
    return lib.raw("hb_sgp_psi_grad" + suffix)(a["kind"], a["Xm"], a["Xv"], a["Y"], a["z"], a["ell"], a["dl"], a["Q"], a["R"],
                                               a["mubar"], a["sbar"], a["zbar"], a["ellbar"], a["N"], a["M"], a["d"], a["P"],
                                               a["ws"], None)


@pytest.mark.parametrize("suffix", ["_f32", "_f64"])
@pytest.mark.parametrize("bad, word", [
    (dict(kind=1), "UnitRBF"),
    (dict(kind=7), "UnitRBF"),
    (dict(N=0), "extents"),
    (dict(N=-3), "extents"),
    (dict(M=0), "extents"),
    (dict(d=0), "extents"),
    (dict(d=1536, dl=1536), "extents"),
    (dict(P=0), "extents"),
    (dict(dl=2, d=3), "lengthscales"),
    (dict(Xm=None), "NULL input"),
    (dict(Xv=None), "NULL input"),
    (dict(Y=None), "NULL input"),
    (dict(z=None), "NULL input"),
    (dict(ell=None), "NULL input"),
    (dict(Q=None), "NULL input"),
    (dict(R=None), "NULL input"),
    (dict(mubar=None), "NULL output"),
    (dict(sbar=None), "NULL output"),
    (dict(zbar=None), "NULL output"),
    (dict(ellbar=None), "NULL output"),
    (dict(ws=None), "workspace"),
    (dict(M=46341, ws=16), "too large"),
])
def test_psi_grad_rejects_bad_arguments(suffix, bad, word):
    """(the pointers are the integer 1: any launch would fault -- every case must return before one)"""
    from henbun_amd import _lib

    lib = _lib.lib()
    rc = _grad_call(lib, suffix, **bad)
    assert rc < 0 and word in lib.last_error(), (rc, lib.last_error())


def test_psi_grad_workspace_does_not_grow_with_N():
    from henbun_amd import _lib

    f = _lib.lib().raw("hb_sgp_psi_grad_ws_elems")
    for M, d, P, b in [(512, 1, 1, 4), (1024, 2, 2, 4), (512, 4, 1, 8), (33, 3, 3, 4), (1, 1, 1, 8), (128, 6, 5, 4), (64, 40, 2, 8)]:
        w = [f(N, M, d, P, b) for N in (100000, 1000000, 10000000)]
        assert w[0] > 0 and w[0] == w[1] == w[2]
        assert f(1, M, d, P, b) == w[0]
        # the partials of at most 4096 workgroups of the pair passes (rows, columns, ellbar of a tile; a 64-block of the psi1
        # pass) and the 2^22 doubles of the point pass's budget (at least one wave of points: 64 (2 d G + 4 d + 2), G <= 16)
        pair = 4096 * (2 * 64 * d + d + 64 * d + d)
        point = max(1 << 22, 64 * (2 * d * 16 + 4 * d + 2))
        assert w[0] <= (8 // b) * (pair + point + 7 * 64)
    assert f(0, 512, 1, 1, 4) == 0
    assert f(100000, 512, 1, 1, 4) == 2 * f(100000, 512, 1, 1, 8)


# ---------------------------------------------------------------- the restatement against what defines it
CASES = [   # (N, M, d, P, scalar_ell, residual)
    (50, 10, 1, 1, False, "diagonal"),
    (50, 10, 1, 3, False, "neglected"),
    (40, 9, 2, 3, False, "diagonal"),
    (40, 9, 2, 1, True, "neglected"),
    (60, 12, 3, 3, False, "neglected"),
    (60, 12, 3, 1, True, "diagonal"),
]


def _case(N, M, d, P, scalar_ell, zero_rows=True):
    mu, s, Y, z, ell = PG.case(N, M, max(d, 1) if d != 2 else 3, P, seed=3, scalar_ell=scalar_ell, zero_rows=zero_rows)
    if d == 2:   # collapsed_grad_ref.case knows d = 1 and d = 3: d = 2 takes the first two columns of its d = 3 case
        mu, s, z = mu[:, :2], s[:, :2], z[:, :2]
        ell = ell if scalar_ell else ell[:2]
    return mu, s, Y, z, ell


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("with_kl", [False, True])
@pytest.mark.parametrize("N, M, d, P, scalar_ell, residual", CASES)
def test_restatement_agrees_with_autograd(N, M, d, P, scalar_ell, residual, with_kl):
    """Value and every gradient of psi_grad_ref.bound_and_grad within 1e-9 relative (to the largest entry of the array) of
    torch.autograd on the bound written from the definitions, at jitter 1e-3 with well-separated inducing points; with
    and without the KL term (then every variance is positive)."""
    mu, s, Y, z, ell = _case(N, M, d, P, scalar_ell, zero_rows=not with_kl)
    got = PG.bound_and_grad(mu, s, Y, z, ell, JITTER, 0.09, 1.3, residual, with_kl=with_kl)
    ref = PG.bound_autograd(mu, s, Y, z, ell, JITTER, 0.09, 1.3, residual, with_kl=with_kl)
    figs = {k: _rel(got[k], ref[k]) for k in ("value", "X_mean", "X_var", "z", "lengthscales", "noise_var", "k_var")}
    print("restatement against autograd:", {k: "%.1e" % v for k, v in figs.items()})
    assert got["lengthscales"].shape == (1 if scalar_ell or d == 1 else d,)
    assert all(v <= 1e-9 for v in figs.values()), figs


@pytest.mark.parametrize("N, M, d, P, scalar_ell", [(50, 10, 1, 2, False), (60, 12, 3, 3, False), (40, 9, 3, 1, True)])
def test_zero_variance_is_the_streamed_gradient(N, M, d, P, scalar_ell):
    """s = 0: zbar and ellbar of psi_grad are those of collapsed_grad_ref.streamed (the semantics of hb_sgp_kgrad) for the
    same weights, within 1e-12 of the largest entry."""
    mu, _, Y, z, ell = _case(N, M, d, P, scalar_ell)
    r = CG.bound_and_grad(mu, Y, z, ell, JITTER, 0.09, 1.3)
    got = PG.psi_grad(mu, np.zeros_like(mu), Y, z, ell, r["Q"], r["R"])
    zs, es = CG.streamed(mu, Y, z, ell, r["Q"], r["R"])
    ez, ee = _rel(got["zbar"], zs), _rel(got["ellbar"], es)
    print("zero variance: zbar %.1e ellbar %.1e" % (ez, ee))
    assert ez <= 1e-12 and ee <= 1e-12
    assert np.all(got["zbar_abs"] >= np.abs(got["zbar"])) and np.all(got["mubar_abs"] >= np.abs(got["mubar"]))


@pytest.mark.parametrize("with_kl", [False, True])
def test_central_difference_along_a_random_direction_of_q_x(with_kl):
    """The directional derivative of the bound along a random direction in (mu, log s) from the restatement's gradient
    against a central difference of the bound value, h = 1e-5: within 1e-6 relative (the difference's own truncation and
    cancellation error: h^2 times the third derivative, and 1e-16 |F| / h)."""
    mu, s, Y, z, ell = _case(40, 9, 2, 3, False, zero_rows=False)
    rng = np.random.RandomState(11)
    dm, dls = rng.randn(*mu.shape), rng.randn(*s.shape)
    r = PG.bound_and_grad(mu, s, Y, z, ell, JITTER, 0.09, 1.3, "diagonal", with_kl=with_kl)
    want = float((r["X_mean"] * dm).sum() + (r["X_var"] * s * dls).sum())                 # ds / dlog s = s
    f = lambda h: PG.bound_value(mu + h * dm, s * np.exp(h * dls), Y, z, ell, JITTER, 0.09, 1.3, "diagonal", with_kl)
    h = 1e-5
    fd = (f(h) - f(-h)) / (2.0 * h)
    print("central difference %.10g, gradient %.10g (%.1e relative)" % (fd, want, abs(fd / want - 1)))
    assert abs(fd - want) <= 1e-6 * abs(want)
