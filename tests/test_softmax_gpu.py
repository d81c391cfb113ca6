"""Multi-class classification on the GPU against the numpy restatement tests/softmax_ref.py (itself pinned on the host by
tests/test_softmax_cpu.py): hb_sgp_mwstats (the bits of hb_sgp_wstats, class by class), hb_lik_softmax_sites / _predict,
SparseGP.natgrad_q with likelihoods.Softmax in float64 and float32 sessions, and models.SVGPMulticlass end to end.

Bounds.  The float64 sites: lam (a mean of positive terms) 1e-11 relative -- |f - lse| <= 750 inside an exp is 750 * 2^-53
~ 1e-13 relative, the mean over 128 terms adds a few ulp; g and beta, which can cancel, 1e-12 (1 + |mu|) absolute; the sum
of l 1e-12 of sum |l_j| (the bound of tests/test_sites_gpu.py).  The float32 entries compute in double and round once: one
float32 ulp against the restatement evaluated in double on the same float32 inputs.  End to end in float64: 1e-8, the bound
of test_natgrad_q_fp64_follows_the_restatement; in float32: 4 x the error of the float32 restatement, the factor
test_natgrad_q_fp32_session_predicts_within_the_float32_restatements_error grants.  Every figure is printed first."""
import numpy as np
import pytest
import torch

import henbun_amd as hb
from henbun_amd import _lib
from henbun_amd import graph as G
from henbun_amd import hip_ops as H
from henbun_amd.models import SVGPMulticlass

import optimal_q_ref as R
import sites_ref as SR
import softmax_ref as F

pytestmark = pytest.mark.gpu

KSPLIT = 432          # columns per float32 block of the restatement (tests/test_sites_gpu.py)


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


# ------------------------------------------------------------------------------------------------ 1. hb_sgp_mwstats
def _weights(C, N, seed):
    """w, r [C, N]: set 0 all ones, set 1 mixed sign with exact zeros, set 2 random positive, then the same two kinds again."""
    rng = np.random.RandomState(seed)
    w = np.ones((C, N))
    for c in range(1, C):
        if c % 2:
            w[c] = rng.randn(N)
            w[c, rng.uniform(size=N) < 0.1] = 0.0
            w[c, :2] = (-1.5, 0.0)
        else:
            w[c] = np.exp(rng.randn(N))
    return w, rng.randn(C, N)


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("N", [1000, 32768 + 40])
@pytest.mark.parametrize("dtype, M, wfrag", [("float32", 32, False), ("float32", 32, True), ("float32", 160, False),
                                             ("float32", 160, True), ("float64", 32, False), ("float32", 20, False)])
def test_sgp_mwstats_returns_the_bits_of_sgp_wstats_class_by_class(dtype, M, wfrag, N, d):
    """C in {1, 3, 5} weight sets from ONE A: np.array_equal with hb_sgp_wstats(w[c], r[c]) on Phi, b, tr for every class;
    Phi[c] bitwise symmetric; a second call returns the same bits; C = 1 with w = 1 equals hb_sgp_stats.  float32 M = 32 (one
    tile) and 160 (an off-diagonal tile) take the MFMA form, with and without Wfrag (which exists for that form only);
    float64 and float32 M = 20 the plain form.  N = 32808 crosses a chunk and leaves a ragged tail.  Without Wfrag W is the
    host's factor; with it, W and its fragment images come from the device's own factor + inverse at jitter 1e-3 (equal bits
    do not ask for an accurate W, only for one W)."""
    dt = torch.float64 if dtype == "float64" else torch.float32
    X, _, _, _, z, ell, W = SR.stats_case(N, M, d, seed=N + M + d)
    Xd, zd, elld, Wd = (dev(a, dt) for a in (X, z, ell, W))
    frag = None
    if wfrag:
        frag = torch.empty(2 * M * M, dtype=dt, device="cuda")
        _, Wd, info = H.cholesky_inverse(H.gram_fwd(zd, zd, elld, diag_add=1e-3), frag=frag)
        assert int(info.cpu()[0]) == 0
    for C in (1, 3, 5):
        w, r = _weights(C, N, seed=C + N)
        wd, rd = dev(w, dt), dev(r, dt)
        Phi, b, tr = H.sgp_mwstats(Xd, wd, rd, zd, elld, Wd, wfrag=frag)
        again = H.sgp_mwstats(Xd, wd, rd, zd, elld, Wd, wfrag=frag)
        torch.cuda.synchronize()
        assert Phi.shape == (C, M, M) and b.shape == (C, M) and tr.shape == (C,) and Phi.dtype == torch.float64
        for a, c in zip((Phi, b, tr), again):
            assert torch.equal(a, c)
        Phi, b, tr = (t.cpu().numpy() for t in (Phi, b, tr))
        for c in range(C):
            one = H.sgp_wstats(Xd, wd[c].contiguous(), rd[c].contiguous(), zd, elld, Wd, wfrag=frag)
            oP, ob, ot = (t.cpu().numpy() for t in one)
            assert np.array_equal(Phi[c], oP) and np.array_equal(b[c], ob[0]) and np.array_equal(tr[c], ot[0]), (C, c)
            assert np.array_equal(Phi[c], Phi[c].T)
        if C == 1:
            plain = H.sgp_stats(Xd, rd.reshape(N, 1), zd, elld, Wd, wfrag=frag)
            assert np.array_equal(Phi[0], plain[0].cpu().numpy()) and np.array_equal(b, plain[1].cpu().numpy())
            assert np.array_equal(tr, plain[3].cpu().numpy())


def test_sgp_mwstats_pads_rows_that_would_start_misaligned():
    """N = 1001 in float32: rows of a contiguous [C, N] start 4 bytes off a 16-byte boundary; the wrapper pads them, the
    library refuses them.  The result is still the bits of hb_sgp_wstats."""
    N, M, d, C = 1001, 32, 1, 3
    X, _, _, _, z, ell, W = SR.stats_case(N, M, d, seed=5)
    Xd, zd, elld, Wd = (dev(a, torch.float32) for a in (X, z, ell, W))
    w, r = _weights(C, N, seed=1)
    wd, rd = dev(w, torch.float32), dev(r, torch.float32)
    Phi, b, tr = H.sgp_mwstats(Xd, wd, rd, zd, elld, Wd)
    for c in range(C):
        one = H.sgp_wstats(Xd, wd[c].clone(), rd[c].clone(), zd, elld, Wd)
        assert torch.equal(Phi[c], one[0]) and torch.equal(b[c], one[1][0]) and torch.equal(tr[c], one[2][0])
    out = [torch.empty(s, dtype=torch.float64, device="cuda") for s in ((C, M, M), (C, M), (C,))]
    ws = H.workspace(torch.float32, Xd.device, H.sgp_mwstats_ws_elems(torch.float32, N, M, d, C))
    with pytest.raises(_lib.HipBackendError, match="16-byte"):
        _lib.lib().call("hb_sgp_mwstats_f32", H.KERN_RBF, H._p(Xd), H._p(wd), H._p(rd), N, H._p(zd), H._p(elld), 1, H._p(Wd),
                        None, H._p(out[0]), H._p(out[1]), H._p(out[2]), N, M, d, C, H._p(ws), H.stream())
    assert H.sgp_mwstats_ws_elems(torch.float32, 10 ** 6, 512, 2, 10) == H.sgp_wstats_ws_elems(torch.float32, 10 ** 6, 512, 2)


# ------------------------------------------------------------------------------------------------ 2. the sites
def _site_inputs(C, N, seed):
    """(y, mean, var) before the scales 1.25 / 0.8: mu = 1.25 mean reaches +-40 exactly, v = 0.8 var runs from exact 0 (every
    fifth point, all classes) to exactly 50; the labels cover class 0 and class C - 1."""
    rng = np.random.RandomState(seed)
    mean = rng.randn(C, N) * rng.choice([0.5, 4.0, 16.0], size=(1, N))
    mean = np.clip(mean, -32.0, 32.0)
    mean[0, 0], mean[C - 1, 0] = 32.0, -32.0
    var = np.exp(rng.uniform(-6, np.log(62.5), (C, N)))
    var[:, ::5] = 0.0
    var[1, N // 2] = 62.5
    y = rng.randint(0, C, N)
    y[0], y[-1] = 0, C - 1
    return y.astype(np.float64), mean, var


def _ulps32(got, ref):
    """|got - ref| in units of the float32 spacing at ref."""
    a32 = np.maximum(np.abs(ref.astype(np.float32)), np.finfo(np.float32).tiny)
    ulp = (np.nextafter(a32, np.float32(np.inf)) - a32).astype(np.float64)
    return np.abs(got.astype(np.float64) - ref.astype(np.float32).astype(np.float64)) / ulp


MS, VS = 1.25, 0.8


_SITE_CASES = [(C, N, S) for C in (2, 3, 5, 10, 33, 64) for N in (1, 77, 1000) for S in (1, 128)]
# the grid is at most 1024 workgroups of 256 / CP points: beyond 1024 * 256 / CP points a workgroup walks its loop over
# point tiles more than once -- with C = 64, S = 128 re-staging both node tiles on every trip, with C = 3 keeping the one
_SITE_CASES += [(64, 5000, 128), (3, 70001, 16)]


@pytest.mark.parametrize("C, N, S", _SITE_CASES)
def test_softmax_sites_and_predict_against_the_restatement(C, N, S):
    """hb_lik_softmax_sites and hb_lik_softmax_predict, float64 and float32 storage, in groups of 2 .. 64 lanes per point
    (C = 3, 5, 10, 33 pad their group), with a last wave whose groups are partly idle, and two sizes at which a workgroup
    takes more than one trip through its point loop.  Bounds: the module docstring.  Also:
    lam >= 0; with var = 0 the closed forms g = onehot - softmax(mu), lam = p (1 - p), prob = softmax(mu); the columns of
    prob sum to 1 within 1e-12; two calls return the same bits."""
    y, mean, var = _site_inputs(C, N, seed=100 * C + N + S)
    nodes = np.random.RandomState(S + C).randn(S, C)
    nd = dev(nodes, torch.float64)
    for dtype in ("float64", "float32"):
        dt, npdt = (torch.float64, np.float64) if dtype == "float64" else (torch.float32, np.float32)
        yq, mq, vq = (a.astype(npdt) for a in (y, mean, var))
        yd, md, vd = dev(yq, dt), dev(mq, dt), dev(vq, dt)
        lam, beta, lsum = H.lik_softmax_sites(yd, md, vd, nd, mscale=MS, vscale=VS)
        lam2, beta2, lsum2 = H.lik_softmax_sites(yd, md, vd, nd, mscale=MS, vscale=VS)
        prob, ld, total = H.lik_softmax_predict(md, vd, nd, y=yd, mscale=MS, vscale=VS)
        prob2, ld2, total2 = H.lik_softmax_predict(md, vd, nd, y=yd, mscale=MS, vscale=VS)
        only, none_ld, none_total = H.lik_softmax_predict(md, vd, nd, mscale=MS, vscale=VS)
        torch.cuda.synchronize()
        for a, c in ((lam, lam2), (beta, beta2), (lsum, lsum2), (prob, prob2), (ld, ld2), (total, total2), (prob, only)):
            assert torch.equal(a, c)
        assert none_ld is None and none_total is None and lsum.dtype == torch.float64 and total.dtype == torch.float64
        lam, beta, prob, ld = (t.cpu().numpy() for t in (lam, beta, prob, ld))
        lsum, total = float(lsum.cpu()[0]), float(total.cpu()[0])
        mu, v = MS * mq.astype(np.float64), VS * vq.astype(np.float64)
        rl, rlam, rbeta, rg = F.sites(yq, mu, v, nodes)
        rprob, rld = F.predict(mu, v, nodes, yq)
        assert all(np.all(np.isfinite(a)) for a in (lam, beta, prob, ld)) and np.all(lam >= 0.0)
        e_sum = abs(lsum - rl.sum()) / np.abs(rl).sum()
        e_tot = abs(total - rld.sum()) / max(np.abs(rld).sum(), 1e-300)
        zero = (v.sum(0) == 0.0)
        hot = (np.arange(C)[:, None] == yq[None, :].astype(np.int64)).astype(np.float64)
        p0 = np.exp(F.log_softmax(mu))
        if dtype == "float64":
            e_lam = (np.abs(lam - rlam) / np.maximum(rlam, 1e-300)).max()
            e_beta = (np.abs(beta - rbeta) / (1.0 + np.abs(mu))).max()
            e_g = (np.abs((beta - lam * mu) - rg) / (1.0 + np.abs(mu))).max()
            e_prob = (np.abs(prob - rprob) / np.maximum(rprob, 1e-300)).max()
            e_ld = (np.abs(ld - rld) / (1.0 + np.abs(rld))).max()
            e_col = np.abs(prob.sum(0) - 1.0).max()
            print("softmax C=%d N=%d S=%d float64: lam %.2e beta %.2e g %.2e sum %.2e; prob %.2e cols %.2e logdens %.2e total %.2e"
                  % (C, N, S, e_lam, e_beta, e_g, e_sum, e_prob, e_col, e_ld, e_tot))
            assert e_lam <= 1e-11 and e_prob <= 1e-11
            assert e_beta <= 1e-12 and e_g <= 1e-12 and e_ld <= 1e-12 and e_col <= 1e-12
            assert e_sum <= 1e-12 and e_tot <= 1e-12
            if zero.any():
                g0 = (beta - lam * mu)[:, zero]
                assert (np.abs(g0 - (hot - p0)[:, zero]) / (1.0 + np.abs(mu[:, zero]))).max() <= 1e-12
                assert np.abs(lam[:, zero] - (p0 * (1 - p0))[:, zero]).max() <= 1e-11 * 0.25 + 1e-16
                assert np.abs(prob[:, zero] - p0[:, zero]).max() <= 1e-11
        else:
            u = [float(_ulps32(a, b).max()) for a, b in ((lam, rlam), (beta, rbeta), (prob, rprob), (ld, rld))]
            print("softmax C=%d N=%d S=%d float32: ulps lam %.2f beta %.2f prob %.2f logdens %.2f; sum %.2e total %.2e"
                  % ((C, N, S) + tuple(u) + (e_sum, e_tot)))
            assert max(u) <= 1.0
            assert e_sum <= 1e-12 and e_tot <= 1e-12


def test_softmax_entries_refuse_bad_arguments_before_any_launch():
    """y = NULL with logdens or total asked for, C outside 2 .. 64, S outside 1 .. 1024, a negative vscale; N = 0 writes
    lsum = 0 and total = 0."""
    C, N, S = 3, 8, 4
    f64 = dict(dtype=torch.float64, device="cuda")
    y, mean, var = (torch.zeros(s, **f64) for s in ((N,), (C, N), (C, N)))
    nodes, out, ld, one = torch.zeros((S, C), **f64), torch.empty((C, N), **f64), torch.empty((N,), **f64), torch.full((1,), 7.0, **f64)
    ws = H.workspace(torch.float64, y.device, 1024)
    call, p = _lib.lib().call, H._p

    def predict(yy, ldd, tot, n=N, c=C, s=S, vs=1.0):
        call("hb_lik_softmax_predict_f64", p(yy), p(mean), p(var), 1.0, vs, p(nodes), s, p(out), p(ldd), p(tot), n, c, p(ws), H.stream())

    def sites(n=N, c=C, s=S, vs=1.0):
        call("hb_lik_softmax_sites_f64", p(y), p(mean), p(var), 1.0, vs, p(nodes), s, p(out), p(out), p(one), n, c, p(ws), H.stream())

    for kw in (dict(yy=None, ldd=ld, tot=None), dict(yy=None, ldd=None, tot=one)):
        with pytest.raises(_lib.HipBackendError, match="need the labels"):
            predict(**kw)
    for kw in (dict(c=1), dict(c=65), dict(s=0), dict(s=1025), dict(vs=-1.0), dict(n=-1)):
        with pytest.raises(_lib.HipBackendError):
            sites(**kw)
        with pytest.raises(_lib.HipBackendError):
            predict(y, ld, one, **kw)
    sites(n=0)
    assert float(one.cpu()[0]) == 0.0
    one.fill_(7.0)
    predict(y, ld, one, n=0)
    assert float(one.cpu()[0]) == 0.0
    assert _lib.lib().raw("hb_lik_softmax_ws_elems")(10 ** 6, 3) == 1024 and _lib.lib().raw("hb_lik_softmax_ws_elems")(1, 64) == 1


def test_softmax_draws_its_default_nodes_on_the_device():
    """Without injected nodes Softmax.nodes() draws [S, C] float64 standard normals from hip_ops.Rng(seed): finite, the same
    array on a second call, equal for equal seeds and different for another seed, and of plausible moments (|mean| within
    5 / sqrt(S C), variance within 20 % at S C = 3072).  SVGPMulticlass(num_nodes=, seed=) hands both to its likelihood and
    its fit runs on those nodes."""
    a, b, c = (hb.likelihoods.Softmax(3, num_nodes=1024, seed=s) for s in (4, 4, 5))
    na = a.nodes()
    assert na.shape == (1024, 3) and na.dtype == np.float64 and np.all(np.isfinite(na))
    assert a.nodes() is na and np.array_equal(b.nodes(), na) and not np.array_equal(c.nodes(), na)
    assert abs(na.mean()) <= 5.0 / np.sqrt(na.size) and abs(na.var() - 1.0) <= 0.2
    X, y, Z, _ = _ring(300, 16)
    m = SVGPMulticlass(X=X, y=y, Z=Z, num_classes=3, num_nodes=64, seed=7, dtype="float64")
    m.gp.kern.lengthscales = np.ones(1)
    m.k_var = np.ones(1) * K_VAR
    lik = object.__getattribute__(m, "likelihood")
    assert (lik.num_nodes, lik.seed) == (64, 7)
    m.reset_q()
    _, _, info = m.fit_q(steps=5)
    assert np.array_equal(lik.nodes(), hb.likelihoods.Softmax(3, num_nodes=64, seed=7).nodes())
    assert np.all(np.isfinite(info["elbo"])) and info["elbo"][-1] > info["elbo"][0]


# ------------------------------------------------------------------------------------------------ 3. natgrad_q
K_VAR, RHO = 4.0, 0.5
_DATA, _REF = {}, {}


def _ring(N, M):
    if (N, M) not in _DATA:
        _DATA[(N, M)] = F.ring(3, N, M, 128, 0)
    return _DATA[(N, M)]


def _model(N, M, dtype, nodes=None):
    X, y, Z, eps = _ring(N, M)
    eps = eps if nodes is None else nodes
    m = SVGPMulticlass(X=X, y=y, Z=Z, num_classes=3, nodes=eps, dtype=dtype)
    m.gp.kern.lengthscales = np.ones(1)
    m.k_var = np.ones(1) * K_VAR
    m.initialize()
    return m, X, y, Z, eps


def _device_W(Z, dt):
    z = dev(Z, dt)
    _, W, info = H.cholesky_inverse(H.gram_fwd(z, z, dev(np.ones(1), dt), diag_add=float(hb.settings.numerics.jitter_level)))
    assert int(info.cpu()[0]) == 0
    return W.cpu().numpy()


def _ref64(steps, residual="diagonal"):
    """The float64 restatement on the N = 300, M = 16 ring with W read back from the device, once per setting."""
    if (steps, residual) not in _REF:
        X, y, Z, eps = _ring(300, 16)
        W = _device_W(Z, torch.float64)
        _REF[(steps, residual)] = F.natgrad(X, y, Z, np.ones(1), hb.settings.numerics.jitter_level, 3, eps, k_var=K_VAR,
                                            residual=residual, steps=steps, rho=RHO, tol=0.0, W=W) + (W,)
    return _REF[(steps, residual)]


def test_natgrad_q_softmax_fp64_follows_the_restatement():
    """12 half steps from the prior in a float64 session (C = 3, N = 300, M = 16, k_var = 4, injected nodes): the ELBO trace,
    the residual trace, m and every S_c S_c^T to 1e-8.  Then 40 steps: the residual ends <= 1e-3 (the restatement: 7e-6), the
    ELBO ends above its value after the first step, and the arg-max of predict's prob is right on >= 99 % of the training
    points (the restatement: all).  Monotonicity is not asserted: the ELBO wiggles by about 1e-4 near the fixed point."""
    m, X, y, Z, eps = _model(300, 16, "float64")
    lik = object.__getattribute__(m, "likelihood")
    qm, S, info = m.gp.natgrad_q(X, y[:, None].astype(np.float64), lik, k_var=K_VAR, steps=12, rho=RHO, tol=0.0)
    rm, rS, rinfo, W = _ref64(12)
    assert info["steps"] == 12 and len(info["elbo"]) == 13 and len(info["residual"]) == 13
    assert qm.shape == (3, 16) and S.shape == (3, 16, 16) and np.array_equal(S, np.tril(S))
    assert all(np.all(np.diag(S[c]) > 0) for c in range(3))
    e_elbo = np.abs(info["elbo"] / rinfo["elbo"] - 1).max()
    e_res = np.abs(info["residual"] - rinfo["residual"]).max()
    e_m = np.abs(qm - rm).max() / np.abs(rm).max()
    SS, rSS = S @ S.transpose(0, 2, 1), rS @ rS.transpose(0, 2, 1)
    e_S = max(np.abs(SS[c] - rSS[c]).max() / np.abs(rSS[c]).max() for c in range(3))
    print("natgrad_q softmax fp64: elbo %.4f -> %.4f (rel err %.2e), residual -> %.2e (err %.2e), m %.2e S S^T %.2e"
          % (info["elbo"][0], info["elbo"][-1], e_elbo, info["residual"][-1], e_res, e_m, e_S))
    assert e_elbo <= 1e-8 and e_res <= 1e-8 and e_m <= 1e-8 and e_S <= 1e-8
    # 40 steps from the prior, on a Data of the model
    Xd, Yd = object.__getattribute__(m, "X"), object.__getattribute__(m, "Y")
    qm, S, info = m.gp.natgrad_q(Xd, Yd, lik, k_var=K_VAR, steps=40, rho=RHO, tol=0.0)
    r40 = _ref64(40)[2]
    print("   40 steps: residual %.2e, elbo[1] %.4f elbo[-1] %.4f (restatement %.4f)"
          % (info["residual"][-1], info["elbo"][1], info["elbo"][-1], r40["elbo"][-1]))
    assert info["steps"] == 40 and np.abs(info["elbo"] / r40["elbo"] - 1).max() <= 1e-8
    assert info["residual"][-1] <= 1e-3
    assert info["elbo"][-1] >= info["elbo"][1]
    # a start from a given q: the restatement's 12th iterate, continued for 28 steps, follows the same trace
    _, _, cont = m.gp.natgrad_q(Xd, Yd, lik, k_var=K_VAR, q0=(rm, rS), steps=28, rho=RHO, tol=0.0)
    assert np.abs(cont["elbo"] / r40["elbo"][12:] - 1).max() <= 1e-8
    A = R.A_of(W, Z, X, np.ones(1))
    mu, v = F.marginals(qm, S, A, 1.0)                                   # unit-variance moments: the scales go to the kernel
    prob, _, _ = H.lik_softmax_predict(dev(mu, torch.float64), dev(v, torch.float64), dev(eps, torch.float64),
                                       mscale=np.sqrt(K_VAR), vscale=K_VAR)
    acc = float(np.mean(np.argmax(prob.cpu().numpy(), 0) == y))
    print("   training accuracy %.4f" % acc)
    assert acc >= 0.99


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_natgrad_q_softmax_with_rows_that_need_padding(dtype):
    """N = 301: the rows of lam, beta [C, N] would not start 16-byte aligned in float32, so natgrad_q keeps them in rows
    padded to a multiple of 4 (and copies the sites into them).  3 half steps against the restatement: the ELBO trace to
    1e-8 relative in float64; in float32 its largest error within 4 x that of the float32 restatement on the device's W."""
    m, X, y, Z, eps = _model(301, 16, dtype)
    lik = object.__getattribute__(m, "likelihood")
    jitter = hb.settings.numerics.jitter_level
    _, _, info = m.gp.natgrad_q(X, y[:, None].astype(np.float64), lik, k_var=K_VAR, steps=3, rho=RHO, tol=0.0)
    ref = F.natgrad(X, y, Z, np.ones(1), jitter, 3, eps, k_var=K_VAR, steps=3, rho=RHO, tol=0.0, W=_device_W(Z, torch.float64))[2]["elbo"]
    err = np.abs(info["elbo"] - ref).max()
    if dtype == "float64":
        bound = 1e-8 * np.abs(ref).min()
    else:
        X32, Z32, ell32 = X.astype(np.float32), Z.astype(np.float32), np.ones(1, np.float32)
        q = F.natgrad(X32, y, Z32, ell32, jitter, 3, eps, k_var=K_VAR, steps=3, rho=RHO, tol=0.0, dtype=np.float32,
                      W=_device_W(Z, torch.float32), ksplit=KSPLIT)[2]["elbo"]
        bound = 4.0 * np.abs(q - ref).max()
    print("natgrad_q softmax N=301 %s: elbo %s, largest error %.2e (bound %.2e)" % (dtype, np.round(info["elbo"], 4), err, bound))
    assert err <= bound


def test_natgrad_q_softmax_fp32_session_predicts_within_the_float32_restatements_error():
    """fit_q in a float32 session (12 half steps from the prior), then predict_proba at X against the float64 restatement;
    bound: 4 x the error of the float32 restatement (float32 A, marginals and weighted products, lam and beta rounded to
    float32, float64 tails) on the model's own float32 W.  Accuracy >= 99 %.  The model fits and predicts class probabilities
    with the moments without the residual (models.SVGPMulticlass), so both restatements run with residual 'neglected'."""
    m, X, y, Z, eps = _model(300, 16, "float32")
    m.reset_q()
    _, _, info = m.fit_q(steps=12, tol=0.0)
    prob32 = m.predict_proba(X)
    rm, rS, rinfo, W64 = _ref64(12, "neglected")
    rprob, _ = F.predict(*F.marginals(rm, rS, R.A_of(W64, Z, X, np.ones(1)), K_VAR, "neglected"), eps)
    X32, Z32, ell32 = X.astype(np.float32), Z.astype(np.float32), np.ones(1, np.float32)
    W32 = _device_W(Z, torch.float32)
    fm, fS, _ = F.natgrad(X32, y, Z32, ell32, hb.settings.numerics.jitter_level, 3, eps, k_var=K_VAR, residual="neglected",
                          steps=12, rho=RHO, tol=0.0, dtype=np.float32, W=W32, ksplit=KSPLIT)
    qprob, _ = F.predict(*F.marginals(fm, fS, R.A_of(W32, Z32, X32, ell32), K_VAR, "neglected"), eps)
    b, g = np.abs(qprob - rprob).max(), np.abs(prob32 - rprob).max()
    acc = float(np.mean(np.argmax(prob32, 0) == y))
    print("natgrad_q softmax fp32: prob error %.3e (float32 restatement %.3e, %.2f x); elbo %.4f (fp64 %.4f); accuracy %.4f"
          % (g, b, g / b, info["elbo"][-1], rinfo["elbo"][-1], acc))
    assert prob32.dtype == np.float32 and prob32.shape == (3, 300)
    assert g <= 4.0 * b
    assert acc >= 0.99


# ------------------------------------------------------------------------------------------------ 4. the model
def _grad_plan(m):
    """(plan, objective, d objective / d q_mu) of the model's own ELBO on ALL rows (tests/test_sites_gpu.py)."""
    opt = m.ELBO()
    opt._ensure_compiled()
    m.initialize()
    obj = opt._trace(None)
    q = object.__getattribute__(m, "u")
    grads = G.gradients(obj, [object.__getattribute__(q, "q_mu")._leaf])
    return m._session.make_plan([obj] + grads, minibatch=None), obj, grads


def test_svgp_multiclass_end_to_end():
    """C = 3, N = 600, M = 32, float64.  reset_q(); fit_q() writes blocks the model reads back unchanged (1e-14);
    predict_proba is right on >= 99 % of the training points; predict_log_density is the log of the label's predict_proba
    entry (1e-12); after fit_q the Monte-Carlo gradient of the sampled ELBO (all rows, analytic KL, 128 draws) with respect
    to q_mu is zero within 4 standard errors for >= 99 % of the entries and the Monte-Carlo ELBO equals the fit's within 4
    standard errors, the criteria of test_svgplik_fit_q_zeroes_the_gradient_of_the_sampled_elbo; three Adam steps run, stay finite and move the lengthscale.

    The nodes are 1024 Halton points (softmax_ref.halton_normal), not the 128 pseudo-random ones of the other tests.  fit_q
    zeroes the gradient of the FIXED-NODE sum; the criterion measures the gradient of the exact expectation, so the two must
    agree to a fraction of the criterion's standard error.  With respect to m that difference is sqrt(k) A (E g - mean_s g),
    pure quadrature error, and the restatement puts a number on it: 128 pseudo-random nodes leave up to 12 standard errors,
    1024 Halton nodes 0.27.  The model fits with the moments WITHOUT the residual, because its sampled ELBO draws one
    residual per point for all classes and softmax does not see a common shift (models.SVGPMulticlass).  Observed on MI355X
    before either was in place: 128 pseudo-random nodes and per-class residuals, 69 % of the entries within 4 s.e., the worst
    at 12.6; 1024 Halton nodes and per-class residuals, 89 %, the worst at 8.5, the Monte-Carlo ELBO -31.39 +- 0.29 against the
    fit's -33.58 (the restatement without the residual: -31.85).  With both: 100 %, the worst at 3.81, -31.25 +- 0.31 against
    -31.85."""
    K = 128
    cfg = hb.settings.get_settings()
    cfg.numerics.kl_form = "analytic"
    with hb.settings.temp_settings(cfg):
        m, X, y, Z, eps = _model(600, 32, "float64", nodes=F.halton_normal(1024, 3))
        plan, obj, grads = _grad_plan(m)

        def draws():
            g, o = [], []
            for _ in range(K):
                plan.run()
                plan.check()
                g.append(plan.value(grads[0]).astype(np.float64).reshape(-1))
                o.append(float(np.ravel(plan.value(obj))[0]))
            g, o = np.stack(g), np.asarray(o)
            return g.mean(0), g.std(0, ddof=1) / np.sqrt(K), o.mean(), o.std(ddof=1) / np.sqrt(K)

        g0, se0, _, _ = draws()
        m.reset_q()
        qm, S, info = m.fit_q()
        bm, bS = m._current_blocks()
        assert qm.shape == (3, 32) and S.shape == (3, 32, 32)
        assert np.allclose(bm, qm, rtol=0, atol=1e-14) and np.allclose(bS, S, rtol=0, atol=1e-14)
        g1, se1, e1, see1 = draws()
        frac0, frac1 = np.mean(np.abs(g0) <= 4 * se0), np.mean(np.abs(g1) <= 4 * se1)
        print("SVGPMulticlass: fit_q %d steps, elbo %.4f, residual %.2e; d ELBO / d q_mu within 4 s.e.: initial q %.0f %% (max "
              "%.1f s.e.), after fit_q %.0f %% (max %.2f); Monte-Carlo ELBO %.3f +- %.3f"
              % (info["steps"], info["elbo"][-1], info["residual"][-1], 100 * frac0, np.max(np.abs(g0) / se0), 100 * frac1,
                 np.max(np.abs(g1) / se1), e1, see1))
        prob = m.predict_proba(X)
        acc = float(np.mean(m.predict(X) == y))
        ld, total = m.predict_log_density(X, y)
        e_ld = np.abs(ld - np.log(prob[y, np.arange(600)])).max()
        mean, var = m.predict_f(X[:50])
        print("   accuracy %.4f, predict_log_density vs log prob %.2e, total %.4f" % (acc, e_ld, total))
        assert prob.shape == (3, 600) and np.abs(prob.sum(0) - 1).max() <= 1e-12 and mean.shape == (3, 50) and np.all(var > 0)
        assert acc >= 0.99
        assert e_ld <= 1e-12 and abs(total - ld.sum()) <= 1e-12 * np.abs(ld).sum()
        assert np.all(se1 > 0) and see1 > 0
        assert frac1 >= 0.99
        assert abs(e1 - info["elbo"][-1]) <= 4.0 * see1
        ell0 = m.gp.kern.lengthscales.value.copy()
        opt = m.ELBO()
        v0 = opt.run(minibatch_size=128)
        opt.optimize(maxiter=3, minibatch_size=128)
        v1 = opt.run(minibatch_size=128)
        assert np.isfinite(v0) and np.isfinite(v1)
        assert np.all(np.isfinite(m.gp.kern.lengthscales.value)) and not np.array_equal(m.gp.kern.lengthscales.value, ell0)
        with pytest.raises(ValueError, match="label"):
            m.predict_log_density(X[:4], np.array([0, 1, 2, 3]))
