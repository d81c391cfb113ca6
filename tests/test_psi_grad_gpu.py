"""Gradients of the psi statistics on the GPU against the numpy restatement tests/psi_grad_ref.py (itself pinned on the host
by tests/test_psi_grad_cpu.py against torch.autograd): the raw kernels hb_sgp_psi_grad_* in both storage types, then
SparseGP.psi_bound_and_grad, SVGP.collapsed_bound_and_grad / fit_hyper with X_var= and models.BayesianGPLVM.

Bounds.  Raw kernels: every output entry within (8192 + 2 terms) 2^-52 (sum of |terms|) + 1e-280, the bound of
test_psi_gpu.py applied to the absolute term sum the restatement returns -- the gradients are cancelling sums (Q comes from
the tail at jitter 1e-3 and alternates in sign with entries ~ 1 / jitter), so the error of any order of summation scales
with the absolute sum, not with the result.  SparseGP.psi_bound_and_grad: value 1e-8 relative; each gradient 4 x max(CPU
gap between psi_grad_ref and autograd on the same inputs, 1e-10 x cancelling scale), the rule of
test_collapsed_grad_gpu.py; the cancelling scale is max|streamed part| + max|Kmm part| for z and the lengthscales and the
absolute term sums for X_mean, X_var and the scalars.  Model level: 4 x the error the same central difference makes on the
CPU restatement at the same h.  Every figure is printed before it is asserted.

The split and block rules of csrc/sgp_psi_grad.hip, restated here so that the cases below can be seen to cross them:
  pair passes   tiles T = nt (nt + 1) / 2, nt = ceil(M / 64); blocks of dimensions zb = 1 (d <= 4) or ceil(d / 4); at most
                S = max(1, 4096 // (T zb)) splits; points per split ks = ceil(N / S) rounded up to 64; splits = ceil(N / ks).
                N = 1500 at M = 33, d = 3: 24 splits, the last of 28 points; at M = 128, d = 5: T = 3, zb = 2, S = 682, 24
                splits; N = 257: 5 splits, one point in the last; M = 128: an off-diagonal tile; M = 33: a ragged tile.
  point pass    one point per lane of a 64-wide workgroup (N = 257: 5 workgroups, one lane in the last); row splits
                G = min(16, ceil(M (M + 1) / 2 / 512)): M = 1, 33 -> 1 and 2, M = 64 -> 5, M = 128 -> 16; d = 5 takes the loop
                form (one block of 8 dimensions).

Observed on MI355X: see the docstrings of the tests and profiles/sgp_psi_grad.txt."""
import functools

import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd import hip_ops as H
from henbun_amd.models import SVGP, BayesianGPLVM, svgp_data

import collapsed_grad_ref as CG
import optimal_q_ref as R
import psi_grad_ref as PG
import psi_ref as PR
from test_psi_gpu import _inputs, _settings, dev, JITTER

pytestmark = pytest.mark.gpu

DT = {"float64": (torch.float64, np.float64), "float32": (torch.float32, np.float32)}
OUT = ("mubar", "sbar", "zbar", "ellbar")


def pair_splits_of(N, M, d):
    nt = -(-M // 64)
    zb = 1 if d <= 4 else -(-d // 4)
    S = max(1, 4096 // (nt * (nt + 1) // 2 * zb))
    ks = -(-(-(-N // S)) // 64) * 64
    return -(-N // ks), ks


def groups_of(M):
    return min(16, -(-(M * (M + 1) // 2) // 512))


def test_the_cases_cross_the_split_rules():
    assert pair_splits_of(1500, 33, 3) == (24, 64) and 1500 - 23 * 64 == 28
    assert pair_splits_of(1500, 128, 5) == (24, 64) and 4096 // (3 * 2) == 682
    assert pair_splits_of(257, 64, 1) == (5, 64) and pair_splits_of(2, 1, 1) == (1, 64)
    assert [groups_of(M) for M in (1, 33, 64, 128)] == [1, 2, 5, 16]


def _weights(mu, s, Y, z, ell):
    """(Q, R) of the collapsed bound's tail at jitter 1e-3, noise variance 0.09, k_var 1: signs alternate as in use"""
    _, W = R.chol_factor(z, ell, JITTER)
    Phi, b, yy, _ = PR.stats(mu, s, Y, z, ell, W=W)
    _, _, G, g, _, _, _ = CG.tail(Phi, b, yy, mu.shape[0], 0.09, 1.0, "diagonal")
    return CG.weights(W, G, g)


@functools.lru_cache(maxsize=None)
def _grad_case(dtype, N, M, d, dl, P):
    """storage-rounded inputs of test_psi_gpu._inputs, the weights and the float64 reference, once per shape"""
    npdt = DT[dtype][1]
    mu, s, z, ell = _inputs(N, M, d, dl, npdt, seed=N + 7 * M + 31 * d + dl)
    rng = np.random.RandomState(N + M + P)
    Y = (np.sin(mu.astype(np.float64).sum(1, keepdims=True) + np.arange(P)[None, :]) + 0.3 * rng.randn(N, P)).astype(npdt)
    Q, Rw = _weights(mu, s, Y, z, ell)
    ref = PG.psi_grad(mu, s, Y, z, ell, Q, Rw)
    for a in (mu, s, Y, z, ell, Q, Rw):
        a.flags.writeable = False
    return (mu, s, Y, z, ell, Q, Rw), ref


def _worst(got, ref):
    """{name: worst |got - ref| / bound} over the four outputs"""
    out = {}
    for name, g in zip(OUT, got):
        bound = (8192 + 2 * ref[name + "_terms"]) * 2.0 ** -52 * ref[name + "_abs"] + 1e-280
        assert g.shape == ref[name].shape, name
        out[name] = float((np.abs(g - ref[name]) / bound).max())
    return out


def _run(args, dt):
    mu, s, Y, z, ell, Q, Rw = args
    return H.sgp_psi_grad(*[dev(a, dt) for a in (mu, s, Y, z, ell)], dev(Q, torch.float64), dev(Rw, torch.float64))


# ------------------------------------------------------------------------------------------------ 1. the raw kernels
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("d, dl", [(1, 1), (3, 1), (3, 3), (5, 5)])
@pytest.mark.parametrize("N", [1, 2, 257, 1500])
@pytest.mark.parametrize("M", [1, 33, 64, 128])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_psi_grad_against_the_restatement(dtype, M, N, d, dl, P):
    """hb_sgp_psi_grad_f64 / _f32: the four outputs entry by entry; finite; two calls bitwise equal; the far point's rows
    of mubar, sbar exactly zero; single points alone return the bits they have in the batch.
    Observed on MI355X over the 256 cases, worst fraction of the bound: mubar 0.0047, sbar 0.0041 (M = 1, N = 1500, d = 5),
    zbar 0.23 (float32, M = 128, N = 1, d = 3: one point, entries whose exponent is near the underflow; next 0.19, 0.17,
    0.10, then below 0.04), ellbar 0.0016."""
    dt = DT[dtype][0]
    args, ref = _grad_case(dtype, N, M, d, dl, P)
    out = _run(args, dt)
    out2 = _run(args, dt)
    torch.cuda.synchronize()
    for a, c in zip(out, out2):
        assert a.dtype == torch.float64 and torch.equal(a, c)
    got = [o.cpu().numpy() for o in out]
    assert all(np.all(np.isfinite(g)) for g in got)
    w = _worst(got, ref)
    print("psi_grad %s M=%d N=%d d=%d dl=%d P=%d: worst error / bound %s"
          % (dtype, M, N, d, dl, P, " ".join("%s %.4f" % kv for kv in w.items())))
    assert all(v <= 1.0 for v in w.values()), w
    if N > 5:   # the point 60 lengthscales from every z
        assert not got[0][5].any() and not got[1][5].any()
    mu, s, Y = args[:3]
    for j in sorted({0, N // 2, N - 1}):
        one = _run((mu[j:j + 1], s[j:j + 1], Y[j:j + 1]) + args[3:], dt)
        assert torch.equal(one[0], out[0][j:j + 1]) and torch.equal(one[1], out[1][j:j + 1])


def test_psi_grad_more_columns_of_Y_than_the_statistics_carry_per_pass():
    """P = 6 (hb_sgp_psi_stats carries 4 columns of Y per pass; rho is formed over all P here): the same bound.
    Observed on MI355X: mubar 5.6e-5, sbar 2.7e-5, zbar 9.0e-6, ellbar 1.6e-8 of the bound."""
    args, ref = _grad_case("float64", 300, 70, 2, 2, 6)
    w = _worst([o.cpu().numpy() for o in _run(args, torch.float64)], ref)
    print("psi_grad P=6: worst error / bound", w)
    assert all(v <= 1.0 for v in w.values()), w


def test_psi_grad_large_dimension_takes_two_blocks_of_dimensions():
    """d = 10: two blocks of 8 dimensions in the point pass, three of 4 in the pair passes (the common latent sizes).
    Observed on MI355X: mubar 8.6e-4, sbar 5.8e-4, zbar 1.3e-4, ellbar 1.1e-6 of the bound."""
    args, ref = _grad_case("float64", 200, 40, 10, 10, 2)
    out = _run(args, torch.float64)
    w = _worst([o.cpu().numpy() for o in out], ref)
    print("psi_grad d=10: worst error / bound", w)
    assert all(v <= 1.0 for v in w.values()), w
    assert all(torch.equal(a, c) for a, c in zip(out, _run(args, torch.float64)))


@pytest.mark.parametrize("d, dl, M, N", [(1, 1, 33, 257), (3, 3, 128, 1500), (3, 1, 64, 1500), (5, 5, 33, 300)])
def test_psi_grad_at_zero_variance_is_sgp_kgrad(d, dl, M, N):
    """Xvar = 0: zbar, ellbar agree with hb_sgp_kgrad_f64 on the same Q, R within 4 max(gap, 1e-10 scale), gap the CPU
    difference between psi_grad_ref and collapsed_grad_ref.streamed, scale the largest absolute term sum.
    Observed on MI355X (|psi_grad - kgrad| / CPU gap / bound): d = 1, M = 33: zbar 2.5e-11 / 5.1e-11 / 1.5e-4, ellbar 1.1e-10 /
    2.3e-11 / 1.9e-3; d = 3, M = 128: zbar 3.3e-10 / 2.7e-10 / 4.0e-3, ellbar 2.5e-9 / 1.8e-10 / 6.9e-2; d = 3, dl = 1, M = 64:
    1.7e-10 / 2.8e-10 / 1.3e-3, 3.8e-10 / 9.8e-10 / 4.6e-2; d = 5, M = 33: 1.3e-13 / 2.9e-13 / 6.2e-7, 9.1e-13 / 1.7e-13 / 6.2e-6."""
    mu, _, z, ell = _inputs(N, M, d, dl, np.float64, seed=3 + M + d)
    s = np.zeros_like(mu)
    Y = np.sin(mu.sum(1, keepdims=True) + np.arange(2)[None, :]) + 0.3 * np.random.RandomState(M).randn(N, 2)
    Q, Rw = _weights(mu, s, Y, z, ell)
    ref = PG.psi_grad(mu, s, Y, z, ell, Q, Rw)
    zs, es = CG.streamed(mu, Y, z, ell, Q, Rw)
    f64 = lambda a: dev(a, torch.float64)
    _, _, zb, eb = H.sgp_psi_grad(f64(mu), f64(s), f64(Y), f64(z), f64(ell), f64(Q), f64(Rw))
    zk, ek = H.sgp_kgrad(f64(mu), f64(Y), f64(z), f64(ell), f64(Q), f64(Rw))
    for name, got, want, gap, scale in (("zbar", zb, zk, np.abs(ref["zbar"] - zs).max(), ref["zbar_abs"].max()),
                                        ("ellbar", eb, ek, np.abs(ref["ellbar"] - es).max(), ref["ellbar_abs"].max())):
        err = float((got - want).abs().max().cpu())
        bound = 4.0 * max(gap, 1e-10 * scale)
        print("zero variance d=%d M=%d N=%d %s: |psi_grad - kgrad| %.3e, CPU gap %.3e, scale %.3e, bound %.3e"
              % (d, M, N, name, err, gap, scale, bound))
        assert err <= bound, name


# ------------------------------------------------------------------------------------------------ 2. SparseGP.psi_bound_and_grad
class _ARD(hb.model.Model):
    def setUp(self, Z, kern):
        self.gp = hb.gp.SparseGP(kern=kern, z=Z)


def _stored(m, a):
    return np.asarray(a, dtype=m._session.np_dtype).astype(np.float64)


def _stored_lengthscales(m, gp):
    """the lengthscales as the session holds them (the transform of the stored raw value, rounded), in double"""
    kern = object.__getattribute__(gp, "kern")
    return _stored(m, np.reshape(object.__getattribute__(kern, "lengthscales").value, -1))


def _bound(gap, scale):
    return 4.0 * max(gap, 1e-10 * scale)


def _check_bound_and_grad(tag, gp, m, mu, s, Y, z, ell, s2, k, residual):
    """psi_bound_and_grad on the device against the restatement and autograd on the stored inputs; returns the gradient"""
    val, g = gp.psi_bound_and_grad(mu, s, Y, s2, k, residual=residual)
    mus, ss, Ys, zs_ = (_stored(m, a) for a in (mu, s, Y, z))
    ells = _stored_lengthscales(m, gp)
    assert np.allclose(ells, ell, rtol=1e-6)
    r = PG.bound_and_grad(mus, ss, Ys, zs_, ells, JITTER, s2, k, residual)
    a = PG.bound_autograd(mus, ss, Ys, zs_, ells, JITTER, s2, k, residual)
    N, d = mu.shape
    assert isinstance(val, float) and g["X_mean"].shape == (N, d) and g["X_var"].shape == (N, d)
    assert g["z"].shape == z.shape and g["lengthscales"].shape == ells.shape and g["z"].dtype == np.float64
    assert isinstance(g["noise_var"], float) and isinstance(g["k_var"], float)
    scales = dict(X_mean=r["X_mean_abs"].max(), X_var=r["X_var_abs"].max(),
                  z=np.abs(r["z_streamed"]).max() + np.abs(r["z_kmm"]).max(),
                  lengthscales=np.abs(r["ell_streamed"]).max() + np.abs(r["ell_kmm"]).max(),
                  noise_var=r["noise_var_abs"], k_var=r["k_var_abs"])
    print("psi_bound_and_grad %s: value %.9f ref %.9f (rel %.2e)" % (tag, val, r["value"], abs(val / r["value"] - 1)))
    rows = []
    for name, scale in scales.items():
        err = float(np.abs(np.asarray(g[name]) - np.asarray(r[name])).max())
        gap = float(np.abs(np.asarray(r[name]) - np.asarray(a[name])).max())
        rows.append((name, err, _bound(gap, scale)))
        print("   %-12s device %.3e, CPU gap %.3e, cancelling scale %.3e (max|grad| %.3e), bound %.3e"
              % (name, err, gap, scale, np.abs(np.asarray(r[name])).max(), rows[-1][2]))
    assert abs(val - r["value"]) <= 1e-8 * abs(r["value"])
    for name, err, bound in rows:
        assert err <= bound, name
    return val, g, r


def _variances(N, d=1, seed=5, ell=0.9):
    s = np.random.RandomState(seed).uniform(0.0, 0.3, (N, d)) * ell ** 2
    s[::7] = 0.0
    return s


@pytest.mark.parametrize("dtype, residual", [("float64", "diagonal"), ("float64", "neglected"), ("float32", "diagonal"),
                                             ("float32", "neglected")])
def test_psi_bound_and_grad_against_the_restatement(dtype, residual):
    """N = 1500, M = 48, d = 1 (svgp_data), in a float64 and a float32 session: float64 arithmetic either way, so the same
    bounds hold.  Also: the value is collapsed_bound(stats=psi_statistics(..)) (float64 session); X_var = 0 reproduces
    collapsed_bound_and_grad's z, lengthscales and scalars; the [d] and scalar forms of X_var return the column sums.
    Observed on MI355X (device error / CPU gap / bound), float64 'diagonal': value 2.7e-15 relative; X_mean 2.7e-12 / 2.9e-12
    / 1.7e-7; X_var 5.4e-12 / 5.2e-12 / 3.2e-7; z 4.4e-11 / 2.4e-11 / 1.1e-8 (max|z gradient| 0.90, cancelling scale 27.9);
    lengthscales 3.8e-11 / 1.1e-10 / 7.0e-8; noise_var 1.1e-11 / 1.8e-11 / 4.3e-6; k_var 2.0e-12 / 4.2e-12 / 5.2e-7.
    'neglected': value 4.0e-13; z 5.3e-10 / 4.9e-10 / 2.0e-9 (the tightest: 0.27 of its bound).  float32 session,
    'diagonal': value 1.1e-14; z 2.2e-11 / 2.1e-11 / 1.1e-8; 'neglected': z 4.7e-10 / 5.0e-10 / 2.0e-9.  X_var = 0 against
    collapsed_bound_and_grad: z <= 1.7e-10 (bound 1.6e-9), lengthscales <= 4.0e-11, noise_var <= 1.6e-10, k_var <= 4.9e-11."""
    N, M = 1500, 48
    X, Y, Z = svgp_data(N, M, 0)
    s = _variances(N)
    with _settings():
        m = SVGP(X=X, Y=Y, Z=Z, q_shape="fullrank", residual=residual, dtype=dtype)
        m.gp.kern.lengthscales = np.ones(1) * 0.9
        m.initialize()
        gp = object.__getattribute__(m, "gp")
        ell = _stored_lengthscales(m, gp)
        val, g, _ = _check_bound_and_grad("%s %s d=1" % (dtype, residual), gp, m, X, s, Y, Z, ell, 0.4, 1.3, residual)
        if dtype == "float64":
            want = gp.collapsed_bound(X, Y, 0.4, 1.3, residual=residual, stats=gp.psi_statistics(X, s, Y))
            assert abs(val - want) <= 1e-8 * abs(val)
        # zero variance: the certain-input gradient
        v0, g0 = gp.psi_bound_and_grad(X, 0.0, Y, 0.4, 1.3, residual=residual)
        vc, gc = gp.collapsed_bound_and_grad(X, Y, 0.4, 1.3, residual=residual)
        Xs, Ys, Zs = _stored(m, X), _stored(m, Y), _stored(m, Z)
        r = CG.bound_and_grad(Xs, Ys, Zs, ell, JITTER, 0.4, 1.3, residual)
        a = CG.bound_autograd(Xs, Ys, Zs, ell, JITTER, 0.4, 1.3, residual)
        assert abs(v0 - vc) <= 1e-8 * abs(vc) and np.shape(g0["X_var"]) == ()
        for name, scale in (("z", np.abs(r["z_streamed"]).max() + np.abs(r["z_kmm"]).max()),
                            ("lengthscales", np.abs(r["ell_streamed"]).max() + np.abs(r["ell_kmm"]).max()),
                            ("noise_var", r["noise_var_abs"]), ("k_var", r["k_var_abs"])):
            err = float(np.abs(np.asarray(g0[name]) - np.asarray(gc[name])).max())
            bound = _bound(float(np.abs(np.asarray(r[name]) - np.asarray(a[name])).max()), scale)
            print("   X_var = 0 against collapsed_bound_and_grad: %-12s %.3e, bound %.3e" % (name, err, bound))
            assert err <= bound, name
        # the shared forms of X_var: the column sums of the [N, d] form
        _, gf = gp.psi_bound_and_grad(X, np.full((N, 1), 0.05), Y, 0.4, 1.3, residual=residual)
        _, gv = gp.psi_bound_and_grad(X, np.full((1,), 0.05), Y, 0.4, 1.3, residual=residual)
        _, gs = gp.psi_bound_and_grad(X, 0.05, Y, 0.4, 1.3, residual=residual)
        tol = 1e-12 * np.abs(gf["X_var"]).sum()
        assert gv["X_var"].shape == (1,) and np.shape(gs["X_var"]) == ()
        assert abs(gv["X_var"][0] - gf["X_var"].sum()) <= tol and abs(float(gs["X_var"]) - gf["X_var"].sum()) <= tol
        assert np.array_equal(gf["z"], gv["z"]) and np.array_equal(gf["z"], gs["z"])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_psi_bound_and_grad_three_dimensions_ard_two_outputs(dtype):
    """d = 3 with ARD lengthscales, P = 2, N = 600, M = 24, residual 'diagonal'.  The reference takes the lengthscales as
    the session holds them (in a float32 session the transform of the stored raw value is not the float32 rounding of the
    value assigned).  Observed on MI355X, float64 (device / CPU gap / bound): value 1.8e-15; X_mean 8.5e-13 / 1.1e-12 /
    5.1e-7; X_var 8.7e-13 / 1.1e-12 / 8.8e-7; z 6.1e-11 / 5.1e-11 / 5.6e-7; lengthscales 3.2e-11 / 1.9e-11 / 1.2e-6; noise_var
    1.0e-10 / 7.3e-11 / 5.7e-5; k_var 5.9e-12 / 2.7e-12 / 2.0e-6."""
    N, M, d, P = 600, 24, 3, 2
    mu, s, Y, z, ell = PG.case(N, M, d, P, seed=4)
    with _settings():
        m = _ARD(Z=z, kern=hb.gp.kernels.UnitRBF(ell), dtype=dtype)
        m.initialize()
        _check_bound_and_grad("%s diagonal d=3 ARD P=2" % dtype, m.gp, m, mu, s, Y, z, ell, 0.09, 1.3, "diagonal")


def test_psi_bound_and_grad_refuses_what_it_does_not_cover():
    X, Y, Z = svgp_data(200, 32, 0)
    m = SVGP(X=X, Y=Y, Z=Z, q_shape="fullrank", dtype="float64")
    m.initialize()
    gp = m.gp
    with pytest.raises(NotImplementedError, match="fullrank"):
        gp.psi_bound_and_grad(X, 0.1, Y, 0.4, residual="fullrank")
    with pytest.raises(ValueError):
        gp.psi_bound_and_grad(X, 0.1, Y, -1.0)
    with pytest.raises(ValueError, match="X_var"):
        gp.psi_bound_and_grad(X, -0.1, Y, 0.4)
    with pytest.raises(ValueError, match="X_var"):
        gp.psi_bound_and_grad(X, np.full((200, 1), np.nan), Y, 0.4)
    with pytest.raises(ValueError, match="X_var"):
        gp.psi_bound_and_grad(X, np.full((199, 1), 0.1), Y, 0.4)
    with pytest.raises(ValueError, match="do not match"):
        gp.psi_bound_and_grad(X[:-1], 0.1, Y, 0.4)
    with pytest.raises(ValueError):
        m.collapsed_bound_and_grad(X_var=-1.0)
    with pytest.raises(NotImplementedError, match="UnitRBF"):
        _ARD(Z=Z, kern=hb.gp.kernels.UnitMatern52(np.ones(1)), dtype="float64").gp.psi_bound_and_grad(X, 0.1, Y, 0.4)
    dt = torch.float64
    a = [dev(v, dt) for v in (X, np.full_like(X, 0.1), Y, Z, np.ones(1))]
    Q, Rw = dev(np.eye(32), dt), dev(np.ones((32, 1)), dt)
    with pytest.raises(TypeError):
        H.sgp_psi_grad(*a, Q.float(), Rw)
    with pytest.raises(ValueError):
        H.sgp_psi_grad(*a, Q[:-1].contiguous(), Rw)
    with pytest.raises(ValueError):
        H.sgp_psi_grad(*a, Q, Rw, ws=torch.empty(8, dtype=dt, device="cuda"))


# ------------------------------------------------------------------------------------------------ 3. models
def _raw_of(m):
    return {n: m._session.read_raw(v).copy() for n, v in m._hyper_variables().items()}


def _directional(m, names, g, f_dev, f_ref, g_ref, raw0, h, seed=3):
    """per parameter group: the analytic directional derivative on the device against a central difference of f_dev, within
    4 x the error the same difference makes on the CPU restatement"""
    rng = np.random.RandomState(seed)
    rows = []
    for name in names:
        u = np.asarray(rng.standard_normal(raw0[name].shape))
        u = u / np.sqrt((u * u).sum())
        fd_dev = CG.directional_fd(lambda x: f_dev(name, x), raw0[name], u, h)
        fd_ref = CG.directional_fd(lambda x: f_ref(name, x), raw0[name], u, h)
        an_dev, an_ref = float((g[name] * u).sum()), float((np.reshape(g_ref[name], u.shape) * u).sum())
        rows.append((name, abs(an_dev - fd_dev), 4.0 * abs(an_ref - fd_ref)))
        print("%-12s analytic (device) %.9e, central difference (device) %.9e (h = %g): |gap| %.3e; on the CPU restatement: "
              "analytic %.9e difference %.9e; bound %.3e" % (name, an_dev, fd_dev, h, rows[-1][1], an_ref, fd_ref, rows[-1][2]))
    for name, err, bound in rows:
        assert err <= bound, name


def test_svgp_gradient_with_input_noise_against_central_differences():
    """SVGP.collapsed_bound_and_grad(X_var=s) against central differences of collapsed_bound(X_var=s) along a random raw
    direction per parameter group, float64 model, N = 1024, M = 24.
    Observed on MI355X (h = 0.01; |analytic - difference| on the device / bound): z 2.77e-5 / 1.11e-4 (directional derivative
    -0.381); lengthscales 6.54e-4 / 2.62e-3 (-12.8); k_var 2.99e-5 / 1.20e-4 (4.43); var 6.36e-3 / 2.54e-2 (-103.7): the device
    makes the CPU restatement's truncation error to four digits."""
    N, M, h = 1024, 24, 1e-2
    X, Y, Z = svgp_data(N, M, 0)
    s = _variances(N, ell=1.2)
    T = hb.transforms.positive
    with _settings():
        m = SVGP(X=X, Y=Y, Z=Z, q_shape="fullrank", dtype="float64")
        m.gp.kern.lengthscales = np.ones(1) * 1.2
        m.k_var = np.ones(1) * 0.8
        m.var = np.ones(1) * 0.2
        m.initialize()
        val, g = m.collapsed_bound_and_grad(X_var=s)
        raw0 = _raw_of(m)
        assert set(g) == {"z", "lengthscales", "k_var", "var"} and all(g[n].shape == raw0[n].shape for n in g)
        assert abs(val - m.collapsed_bound(X_var=s)) <= 1e-8 * abs(val)
        hv = m._hyper_variables()

        def f_dev(name, x):
            m._session.write_raw(hv[name], x)
            try:
                return m.collapsed_bound(X_var=s)
            finally:
                m._session.write_raw(hv[name], raw0[name])

        def cons(p):
            return tuple(T.forward(p[n]).reshape(-1) for n in ("lengthscales", "k_var", "var"))

        def f_ref(name, x):
            p = dict(raw0)
            p[name] = x
            ell, kv, s2 = cons(p)
            return PG.bound_value(X, s, Y, p["z"], ell, JITTER, float(s2[0]), float(kv[0]))

        ell0, kv0, s20 = cons(raw0)
        r = PG.bound_and_grad(X, s, Y, raw0["z"], ell0, JITTER, float(s20[0]), float(kv0[0]))
        g_ref = dict(z=r["z"], lengthscales=r["lengthscales"] * T.dforward(raw0["lengthscales"]),
                     k_var=r["k_var"] * T.dforward(raw0["k_var"]), var=r["noise_var"] * T.dforward(raw0["var"]))
        _directional(m, ("z", "lengthscales", "k_var", "var"), g, f_dev, f_ref, g_ref, raw0, h)


def test_fit_hyper_with_input_noise_climbs_its_bound():
    """fit_hyper(5, X_var=s): the trace's ends are collapsed_bound(X_var=s) before and after (1e-8), the last above the first,
    and q(u) is left at fit_q(X_var=s).  Observed on MI355X: -1025.343 -> -953.687."""
    N, M = 1024, 24
    X, Y, Z = svgp_data(N, M, 0)
    s = _variances(N)
    with _settings():
        m = SVGP(X=X, Y=Y, Z=Z, q_shape="fullrank", dtype="float64")
        m.gp.kern.lengthscales = np.ones(1) * 2.0
        m.var = np.ones(1) * 1.0
        m.initialize()
        before = m.collapsed_bound(X_var=s)
        trace = m.fit_hyper(5, lr=0.05, X_var=s)
        after = m.collapsed_bound(X_var=s)
        print("fit_hyper(5, X_var=s): %.6f -> %.6f" % (trace[0], trace[-1]))
        assert trace.shape == (6,) and abs(trace[0] - before) <= 1e-8 * abs(before) and abs(trace[-1] - after) <= 1e-8 * abs(after)
        assert trace[-1] > trace[0]
        qm = m.u.q_mu.value.copy()
        want, _ = m.fit_q(X_var=s)
        assert np.allclose(np.reshape(qm, -1), np.reshape(want, -1), rtol=1e-10, atol=1e-12)


def _gplvm_data(N=200, P=6, seed=0):
    rng = np.random.RandomState(seed)
    t = np.sort(rng.uniform(-2.0, 2.0, N))
    Y = np.stack([np.sin(1.5 * t + p) + 0.1 * p * t for p in range(P)], 1) + 0.05 * rng.randn(N, P)
    return t, Y


def test_bayesian_gplvm_gradient_against_central_differences():
    """BayesianGPLVM.bound_and_grad() (raw parameters; the KL of q(X) included) against central differences of bound() in
    X_mean, X_var (raw), z and the lengthscales: N = 200, P = 6, latent_dim = 2, M = 16.
    Observed on MI355X (h = 0.01; |analytic - difference| on the device / bound): X_mean 8.40e-7 / 3.38e-6; X_var 1.15e-7 /
    4.85e-7; z 1.10e-2 / 4.40e-2 (directional derivative 28.7); lengthscales 8.49e-3 / 3.40e-2 (163.5)."""
    _, Y = _gplvm_data()
    T = hb.transforms.positive
    h = 1e-2
    with _settings():
        m = BayesianGPLVM(Y=Y, latent_dim=2, M=16, dtype="float64")
        m.var = np.ones(1) * 0.1
        m.initialize()
        val, g = m.bound_and_grad()
        raw0 = _raw_of(m)
        assert set(g) == {"X_mean", "X_var", "z", "lengthscales", "k_var", "var"}
        assert all(g[n].shape == raw0[n].shape for n in g)
        assert abs(val - m.bound()) <= 1e-8 * abs(val)
        hv = m._hyper_variables()

        def f_dev(name, x):
            m._session.write_raw(hv[name], x)
            try:
                return m.bound()
            finally:
                m._session.write_raw(hv[name], raw0[name])

        def cons(p):
            return (p["X_mean"], T.forward(p["X_var"]), p["z"]) + tuple(T.forward(p[n]).reshape(-1)
                                                                        for n in ("lengthscales", "k_var", "var"))

        def f_ref(name, x):
            p = dict(raw0)
            p[name] = x
            mu, s, z, ell, kv, s2 = cons(p)
            return PG.bound_value(mu, s, Y, z, ell, JITTER, float(s2[0]), float(kv[0]), with_kl=True)

        mu, s, z, ell, kv, s2 = cons(raw0)
        r = PG.bound_and_grad(mu, s, Y, z, ell, JITTER, float(s2[0]), float(kv[0]), with_kl=True)
        g_ref = dict(X_mean=r["X_mean"], X_var=r["X_var"] * T.dforward(raw0["X_var"]), z=r["z"],
                     lengthscales=r["lengthscales"] * T.dforward(raw0["lengthscales"]))
        _directional(m, ("X_mean", "X_var", "z", "lengthscales"), g, f_dev, f_ref, g_ref, raw0, h)


def test_bayesian_gplvm_fit_climbs_and_its_shapes():
    """fit(30): the trace starts at bound(), ends at bound() and ends higher; latent(), fit_q() and predict_y() have the
    documented shapes.  The two fitted lengthscales are printed (one true latent dimension), nothing is asserted about them.
    Observed on MI355X: -665.227 -> 9.603 in 30 steps at lr 0.05; lengthscales 1.72, 1.54 (30 steps do not separate them yet)."""
    N, P, Q, M = 200, 6, 2, 16
    _, Y = _gplvm_data(N, P)
    with _settings():
        m = BayesianGPLVM(Y=Y, latent_dim=Q, M=M, dtype="float64")
        m.var = np.ones(1) * 0.1
        m.initialize()
        before = m.bound()
        trace = m.fit(30, lr=0.05)
        after = m.bound()
        print("BayesianGPLVM.fit(30): %.6f -> %.6f; lengthscales %s" % (trace[0], trace[-1], m.gp.kern.lengthscales.value))
        assert trace.shape == (31,) and abs(trace[0] - before) <= 1e-8 * abs(before) and abs(trace[-1] - after) <= 1e-8 * abs(after)
        assert trace[-1] > trace[0]
        mean, var = m.latent()
        assert mean.shape == (N, Q) and var.shape == (N, Q) and np.all(var > 0)
        qm, S = m.fit_q()
        assert qm.shape == (P, M) and S.shape == (M, M)
        pm, pv = m.predict_y(mean[:7])
        assert pm.shape == (7, P) and pv.shape == (7,) and np.all(pv > 0) and np.all(np.isfinite(pm))
    with pytest.raises(ValueError):
        BayesianGPLVM(Y=Y, latent_dim=2, M=16, X_var=-0.1, Z=np.zeros((16, 2)), dtype="float64")
    with pytest.raises(ValueError):
        BayesianGPLVM(Y=Y, latent_dim=2, M=16, Z=np.zeros((15, 2)), dtype="float64")
