"""hb_gram_predict and the exact GP's cached predictive variance on the GPU (hip_ops.gram_predict, ExactPosterior.build_cache
/ predict_f(var='cache') / acquisition / argmax, ExactGPR.suggest) against hb_gram_matvec's own bits, the float64
restatements tests/variance_cache_ref.py and tests/acq_ref.py (pinned on the host by tests/test_variance_cache_cpu.py)
and the dense posterior of tests/exact_gp_ref.py.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from henbun_amd import _lib, hip_ops as H
from henbun_amd.models import ExactGPR

import exact_gp_ref as E
import variance_cache_ref as VC

pytestmark = pytest.mark.gpu

TORCH = {"float64": torch.float64, "float32": torch.float32}
NP = {"float64": np.float64, "float32": np.float32}
CHUNK = 2048


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def host(t):
    return t.cpu().numpy().astype(np.float64)


def ordered_sum_of_squares(o):
    """q [n] = sum_s o[s]^2 in float64, s ascending, each square and each sum rounded once: the order of the kernel."""
    q = np.zeros(o.shape[1])
    for s in range(o.shape[0]):
        q = q + o[s] * o[s]
    return q


# ------------------------------------------------------------------------------------------------ 1. the kernel
# (n, N, P, S, d, dl): n in {1, 127, 129, 300}; N one chunk, two chunks, 17 chunks in two groups; (P, S) with no cache rows
# and across the 64-row tile; d in {1, 2, 5} with dl in {1, d}; the largest N with small n and S
SWEEP = [
    (1, 1, 1, 1, 1, 1),
    (127, 33, 1, 16, 2, 2),
    (129, CHUNK, 3, 66, 5, 5),
    (300, CHUNK + 1, 1, 64, 2, 1),
    (129, 33, 1, 65, 5, 1),
    (300, CHUNK, 1, 131, 1, 1),
    (1, CHUNK + 1, 1, 1, 5, 5),
    (127, 16 * CHUNK + 5, 1, 16, 2, 2),
]
_SWEEP = {}


def _sweep_case(case, dtype):
    if (case, dtype) not in _SWEEP:
        n, N, P, S, d, dl = case
        rng = np.random.default_rng(n + 3 * N + 5 * S + 7 * d + dl)
        x = rng.uniform(0.0, 4.0, (n, d)).astype(NP[dtype])
        x2 = rng.uniform(0.0, 4.0, (N, d)).astype(NP[dtype])
        ell = (np.array([0.8]) if dl == 1 else 0.7 + 0.2 * np.arange(d)).astype(NP[dtype])
        V = rng.standard_normal((S, N)).astype(NP[dtype])
        _SWEEP[(case, dtype)] = tuple(dev(a, TORCH[dtype]) for a in (x, x2, ell, V))
    return _SWEEP[(case, dtype)]


def test_the_chunk_is_the_one_the_shapes_straddle():
    assert H.gram_matvec_chunk() == CHUNK


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "n%d-N%d-P%d-S%d-d%d-dl%d" % c)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_mean_and_variance_against_the_product(dtype, case):
    """mean: the bits of hb_gram_matvec on V[:P].  var against o = hb_gram_matvec(V[P:]) read back in float64, q = sum o^2
    in the kernel's order: float64 (o is t itself) within 4 x 2^-52 (prior + q); float32 (o is t rounded once, so o^2 is
    t^2 to 2^-23) within 2^-23 q + 2^-24 |var| plus the same slack; exactly 0 wherever prior - q is negative beyond that;
    exactly (T) prior without cache rows.  prior is the median of q: both sides of the clamp occur."""
    n, N, P, S, d, dl = case
    x, x2, ell, V = _sweep_case(case, dtype)
    scale = 1.7
    mean_ref = H.gram_matvec(x, x2, ell, V[:P].contiguous(), scale=scale)
    if S == P:
        prior, q = 0.3, np.zeros(n)
    else:
        q = ordered_sum_of_squares(host(H.gram_matvec(x, x2, ell, V[P:].contiguous(), scale=scale)))
        prior = float(np.median(q)) if n > 1 else 2.0 * float(q[0]) + 0.1
    mean, var, val, bv, bi = H.gram_predict(x, x2, ell, V, P=P, scale=scale, prior=prior)
    torch.cuda.synchronize()
    assert val is None and bv is None and bi is None
    assert mean.shape == (P, n) and var.shape == (n,) and mean.dtype == var.dtype == TORCH[dtype]
    assert torch.equal(mean, mean_ref)
    got = host(var)
    if S == P:
        assert np.all(got == float(NP[dtype](prior)))
        return
    slack = 4.0 * 2.0 ** -52 * (prior + q)
    tol = slack if dtype == "float64" else 2.0 ** -23 * q + 2.0 ** -24 * np.abs(got) + slack
    raw = prior - q
    err = np.abs(got - np.maximum(raw, 0.0))
    print("gram_predict %s %s: prior %.4g, %d of %d columns clamped, largest error / bound %.3e"
          % (dtype, case, prior, int((raw < 0).sum()), n, float((err / tol).max())))
    assert np.all(np.isfinite(got)) and np.all(got >= 0.0)
    assert np.all(err <= tol)
    assert np.all(got[raw < -tol] == 0.0)
    if n > 1:
        assert (raw < -tol).any() and (raw > tol).any()


def _acq_case(dtype, n=300, N=257, r=20, seed=3):
    """One latent function with r cache rows, N within one chunk, q < prior everywhere: (x, x2, ell, V, scale, prior)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, 4.5, (n, 2)).astype(NP[dtype])
    x2 = rng.uniform(0.0, 4.0, (N, 2)).astype(NP[dtype])
    V = np.concatenate([0.1 * rng.standard_normal((1, N)), 0.01 * rng.standard_normal((r, N))]).astype(NP[dtype])
    return tuple(dev(a, TORCH[dtype]) for a in (x, x2, np.array([0.9, 1.2]), V)) + (1.3, 1.3)


def _own_moments(x, x2, ell, V, scale, prior):
    """The kernel's own double (t[0], prior - q) for one chunk, restated exactly: with scale 1 hb_gram_matvec returns the
    chunk's accumulator itself, t is that times scale in double, q the ordered sum."""
    t = scale * host(H.gram_matvec(x, x2, ell, V, scale=1.0))
    return t[0], prior - ordered_sum_of_squares(t[1:])


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("kind", ["ei", "pi", "ucb"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_tails_against_the_restatement(dtype, kind, largest):
    """val against acq_ref's tail in float64 at the kernel's own (mean, var) -- the doubles the tail is evaluated at,
    restated exactly from the one chunk's accumulators; the stored mean and var are their roundings.  Bound: that of
    test_acq_gpu.py for hb_sgp_acq's values given its moments, relative 1e-12, + 2^-24 in float32 storage."""
    x, x2, ell, V, scale, prior = _acq_case(dtype)
    m_d, v_d = _own_moments(x, x2, ell, V, scale, prior)
    best = float(np.quantile(m_d, 0.7 if largest else 0.3))
    a = dict(best=best, param=1.5 if kind == "ucb" else 0.01, var_floor=1e-6)
    mean, var, val, _, _ = H.gram_predict(x, x2, ell, V, P=1, scale=scale, prior=prior, acq=kind, largest=largest, **a)
    torch.cuda.synchronize()
    assert np.array_equal(host(mean)[0], m_d.astype(NP[dtype]).astype(np.float64))
    assert np.array_equal(host(var), v_d.astype(NP[dtype]).astype(np.float64))
    rv = VC.acquisition(kind, m_d, v_d, a["best"], a["param"], largest, a["var_floor"])
    u = (m_d - best) / np.sqrt(v_d)
    bound = 1e-12 + (0.0 if dtype == "float64" else 2.0 ** -24)
    ev = np.abs(host(val) - rv) / np.abs(rv)
    print("gram_predict tail %s %s largest=%s: val relative %.3e (bound %.3e); var in [%.3g, %.3g], u in [%.2f, %.2f], |val| in "
          "[%.3e, %.3e]" % (dtype, kind, largest, ev.max(), bound, v_d.min(), v_d.max(), u.min(), u.max(), np.abs(rv).min(),
                            np.abs(rv).max()))
    assert v_d.min() > a["var_floor"] and np.abs(rv).min() > 1e-30
    assert ev.max() <= bound


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_results_are_a_function_of_the_column(dtype, monkeypatch):
    """x in ragged pieces (cuts that are no multiple of 128) carries the bits of the whole call for mean, var and val, with
    one chunk and with 17; the wrapper forced to cut x into pieces of 128 columns returns the same outputs and the same
    (best_idx, best_val)."""
    for case, cuts in (((300, 257, 1, 21, 2, 2), (0, 100, 131, 300)), ((127, 16 * CHUNK + 5, 1, 16, 2, 2), (0, 3, 126, 127))):
        n, N, P, S, d, dl = case
        x, x2, ell, V = _acq_case(dtype)[:4] if N == 257 else _sweep_case(case, dtype)
        q = ordered_sum_of_squares(host(H.gram_matvec(x, x2, ell, V[1:].contiguous(), scale=1.3)))
        kw = dict(P=1, scale=1.3, prior=float(1.1 * q.max()), acq="ei", best=0.1, param=0.01, var_floor=1e-6, value=True)
        whole = H.gram_predict(x, x2, ell, V, argmax=True, **kw)
        again = H.gram_predict(x, x2, ell, V, argmax=True, **kw)
        pieces = [H.gram_predict(x[a:b].contiguous(), x2, ell, V, **kw) for a, b in zip(cuts[:-1], cuts[1:])]
        monkeypatch.setattr(H, "GRAM_PREDICT_WS_BYTES", 1)
        assert H._gram_predict_piece(n, N, S, TORCH[dtype]) == 128
        forced = H.gram_predict(x, x2, ell, V, argmax=True, **kw)
        monkeypatch.undo()
        torch.cuda.synchronize()
        for k in range(5):
            assert torch.equal(whole[k], again[k]) and torch.equal(whole[k], forced[k]), k
        assert torch.equal(whole[0], torch.cat([p[0] for p in pieces], dim=1))
        assert torch.equal(whole[1], torch.cat([p[1] for p in pieces])) and torch.equal(whole[2], torch.cat([p[2] for p in pieces]))
        val = host(whole[2])
        assert int(whole[4][0]) == int(np.argmax(val)) and float(whole[3][0]) == val.max()


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_argmax_is_numpys_first_maximum(dtype, largest):
    """Every candidate appears twice (rows j and j + 150 of x are equal), so the maximum is tied: the first row wins.
    Rows with a NaN coordinate -- rows 0 and 77 with their twins, and the last row -- give NaN values and are never chosen; the arg-max alone writes no
    values and returns the same pair; all rows NaN: (-1, -inf)."""
    x, x2, ell, V, scale, prior = _acq_case(dtype)
    x = x.clone()
    x[0, 1] = x[77, 0] = float("nan")
    x[150:] = x[:150]
    x[299, 0] = float("nan")
    kw = dict(P=1, scale=scale, prior=prior, acq="ei", best=0.2, param=0.0, largest=largest, var_floor=1e-6)
    _, _, val, bv, bi = H.gram_predict(x, x2, ell, V, mean=False, var=False, value=True, argmax=True, **kw)
    m0, v0, val0, bv0, bi0 = H.gram_predict(x, x2, ell, V, mean=False, var=False, argmax=True, **kw)
    bad = torch.full_like(x, float("nan"))
    _, _, _, bvn, bin_ = H.gram_predict(bad, x2, ell, V, mean=False, var=False, argmax=True, **kw)
    torch.cuda.synchronize()
    val = host(val)
    nan = np.isnan(val)
    want = int(np.nanargmax(val))
    print("gram_predict arg-max %s largest=%s: %d NaN columns, best %.6e at %d (numpy: %d), its twin at %d"
          % (dtype, largest, nan.sum(), float(bv[0]), int(bi[0]), want, want + 150))
    assert sorted(np.nonzero(nan)[0]) == [0, 77, 150, 227, 299] and want < 150 and val[want] == val[want + 150]
    assert int(bi[0]) == want and float(bv[0]) == val[want] and bv.dtype == torch.float64 and bi.dtype == torch.int64
    assert m0 is None and v0 is None and val0 is None and int(bi0[0]) == want and float(bv0[0]) == val[want]
    assert int(bin_[0]) == -1 and float(bvn[0]) == -np.inf


def test_bad_arguments_never_reach_a_launch():
    """The library's own checks (raw calls with real device buffers) and the wrapper's: each raises, and the NaN-filled
    outputs keep their NaNs."""
    dt = torch.float32
    x, x2, V, ell = dev(np.ones((5, 3)), dt), dev(np.ones((4, 3)), dt), dev(np.ones((2, 4)), dt), dev(np.ones(1), dt)
    mean = torch.full((2, 5), float("nan"), dtype=dt, device="cuda")
    var, val = (torch.full((5,), float("nan"), dtype=dt, device="cuda") for _ in range(2))
    bv = torch.full((1,), float("nan"), dtype=torch.float64, device="cuda")
    ws = torch.empty(1024, dtype=dt, device="cuda")
    p = lambda t: None if t is None else H._p(t)

    def raw(kind=H.KERN_RBF, dl=1, P=2, acq=-1, ws_=ws, val_=None, bv_=None, prior=1.0):
        _lib.lib().call("hb_gram_predict_f32", kind, p(x), p(x2), p(ell), dl, p(V), P, 1.0, prior, acq, 0.0, 0.0, 1, 0.0, p(mean),
                        p(var), p(val_), p(bv_), None, 5, 4, 3, 2, p(ws_), H.stream())

    for kw, word in ((dict(kind=H.KERN_SQDIST), "UnitRBF"), (dict(dl=2), "lengthscales"), (dict(P=0), "mean rows"),
                     (dict(P=3), "mean rows"), (dict(acq=H.ACQ["ei"], P=2, val_=val), "one latent function"),
                     (dict(acq=5, P=1, val_=val), "unknown acquisition"), (dict(val_=val), "need an acquisition"),
                     (dict(bv_=bv), "need an acquisition"), (dict(ws_=None), "workspace"), (dict(prior=float("nan")), "prior")):
        with pytest.raises(_lib.HipBackendError, match=word):
            raw(**kw)
    with pytest.raises(_lib.HipBackendError, match="UnitRBF"):
        H.gram_predict(x, x2, ell, V, kind=H.KERN_SQDIST)
    with pytest.raises(ValueError, match="mean rows"):
        H.gram_predict(x, x2, ell, V, P=3)
    with pytest.raises(ValueError, match="one latent function"):
        H.gram_predict(x, x2, ell, V, P=2, acq="ei")
    with pytest.raises(ValueError, match="acq must be one of"):
        H.gram_predict(x, x2, ell, V, P=1, acq="thompson")
    with pytest.raises(ValueError, match="need an acquisition"):
        H.gram_predict(x, x2, ell, V, argmax=True)
    with pytest.raises(ValueError, match="entries"):
        H.gram_predict(x, x2, dev(np.ones(2), dt), V)
    with pytest.raises(ValueError, match="columns"):
        H.gram_predict(x, x2, ell, dev(np.ones((2, 5)), dt))
    with pytest.raises(TypeError, match="dtype"):
        H.gram_predict(x, x2.double(), ell, V)
    with pytest.raises(TypeError, match="dtype"):
        H.gram_predict(x, x2, ell, V.double())
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (mean, var, val, bv))


# ------------------------------------------------------------------------------------------------ 2. the model
RANKS = (16, 64, 128, 256)
_FIT, _TRUTH = {}, {}


def _case(dtype="float64"):
    """The 600-point case of the restatement (ell = 1, noise_var = 0.09) with X and Xnew as a session of `dtype` holds them
    (rounded to it, carried in float64): the references see the inputs the device sees."""
    X, ell, k_var, noise_var, Xnew = VC.square_case(600, 5.0)
    Y = np.sin(X.sum(1, keepdims=True)) + 0.1 * np.random.default_rng(1).standard_normal((600, 1))
    return X.astype(NP[dtype]).astype(np.float64), Y, ell, k_var, noise_var, Xnew.astype(NP[dtype]).astype(np.float64)


def _fit(dtype):
    """ExactGPR on the case, fitted once per dtype."""
    if dtype not in _FIT:
        X, Y, ell, k_var, noise_var, _ = _case(dtype)
        m = ExactGPR(X=X, Y=Y, dtype=dtype)
        m.gp.kern.lengthscales = ell.copy()
        m.k_var = np.ones(1) * k_var
        m.var = np.ones(1) * noise_var
        m.fit()
        _FIT[dtype] = m
    return _FIT[dtype]


def _truth(dtype):
    """(mean [1, n], v_exact [n]) at the 256 test points from the dense Cholesky in float64, once per dtype."""
    if dtype not in _TRUTH:
        X, Y, ell, k_var, noise_var, Xnew = _case(dtype)
        _, mean, var = E.posterior(X, Y, ell, k_var, noise_var, Xnew)
        _TRUTH[dtype] = (mean, var)
    return _TRUTH[dtype]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_cached_variance_end_to_end(dtype):
    """build_cache at ranks 16, 64, 128, 256 (default threshold).  The device's basis C, read back, goes through the
    restatement (its own T, factor and R_c in float64, R_c rounded to the session's dtype): var_upper agrees with it
    within the product's bound propagated through the square, slack_j = sum_s 2 |t_sj| dt_sj + dt_sj^2, with dt the bound of
    tests/test_gram_matvec_gpu.py on t = R_c k*: (11 + d + min(N, 2048) + 1) 2^-24 k_var sum_i |R_c[s, i]| K_ij in float32,
    1e-11 k_var sum_i |R_c[s, i]| in float64 -- plus the rounding of the stored result.  Then the properties: an upper
    bound of the dense variance up to that slack, at most k_var (1 + 2^-23), falling with the rank up to the two slacks,
    the selection exhausted below 256 rows, and there within 4 x the restatement's own distance from the exact variance."""
    X, Y, ell, k_var, noise_var, Xnew = _case(dtype)
    mean_true, v_true = _truth(dtype)
    post = object.__getattribute__(_fit(dtype), "posterior")
    N, d = X.shape
    Kx = E.rbf(X, Xnew, ell)
    eps_out = 2.0 ** -24 if dtype == "float32" else 2.0 ** -53
    got, slack = {}, {}
    for rank in RANKS:
        assert post.build_cache(rank=rank) is post
        info = post.cache_info
        C = post.cache_basis
        assert set(info) == {"rank", "asked", "jitter", "trace"} and info["asked"] == rank and C.shape == (info["rank"], N)
        mean, v = post.predict_f(Xnew, var="cache")
        ref = VC.build(X, ell, k_var, noise_var, C=C.astype(np.float64), rc_dtype=NP[dtype])
        t = VC.products(ref, X, ell, k_var, Xnew)
        if dtype == "float32":
            dt_ = (11 + d + min(N, CHUNK) + 1) * 2.0 ** -24 * k_var * (np.abs(ref["Rc"]) @ Kx)
        else:
            dt_ = 1e-11 * k_var * np.abs(ref["Rc"]).sum(1, keepdims=True) * np.ones_like(t)
        v_ref = k_var - (t * t).sum(0)
        slack[rank] = (2.0 * np.abs(t) * dt_ + dt_ * dt_).sum(0) + eps_out * np.abs(v_ref)
        got[rank] = v.astype(np.float64)
        err = np.abs(got[rank] - np.maximum(v_ref, 0.0))
        print("%s rank %d -> %d (jitter %.1e, restatement %.1e): |var_upper - restatement| %.3e (%.3e of its bound); "
              "var_upper - v_exact in [%.3e, %.3e]; restatement - v_exact at most %.3e"
              % (dtype, rank, info["rank"], info["jitter"], ref["jitter"], err.max(), (err / slack[rank]).max(),
                 (got[rank] - v_true).min(), (got[rank] - v_true).max(), (v_ref - v_true).max()))
        assert mean.shape == (1, 256) and v.shape == (256,) and v.dtype == NP[dtype]
        assert info["rank"] == min(rank, info["rank"]) and info["jitter"] == ref["jitter"] == 1e-13
        assert abs(info["trace"] - ref["trace"]) <= 1e-6 * ref["trace"]
        assert np.all(err <= slack[rank])
        assert np.all(got[rank] >= v_true - slack[rank])
        assert np.all(got[rank] <= k_var * (1.0 + 2.0 ** -23))
        last = (info, ref, v_ref)
    for a, b in zip(RANKS[:-1], RANKS[1:]):
        assert np.all(got[a] >= got[b] - (slack[a] + slack[b])), (a, b)
    info, ref, v_ref = last
    e_dev, e_ref = (got[256] - v_true).max(), (v_ref - v_true).max()
    print("%s exhausted at rank %d: max(var_upper - v_exact) %.3e, the restatement's %.3e" % (dtype, info["rank"], e_dev, e_ref))
    assert info["rank"] < 256
    assert e_dev <= 4.0 * e_ref + slack[256].max()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_cached_route_keeps_the_mean_and_the_solve_route_stays(dtype):
    """predict_f(var='cache') returns the mean bits of predict_f(var=False); predict_y adds the noise variance; var=True is
    still the solve: on 8 points (those where the rank-16 cache is loosest) within the bound of tests/test_exact_gp_gpu.py (1e-5 in float64, tol |k*| |K^^-1| in
    float32) of the dense variance, which the cached bound at rank 16 is nowhere near."""
    X, Y, ell, k_var, noise_var, Xnew = _case(dtype)
    _, v_true = _truth(dtype)
    post = object.__getattribute__(_fit(dtype), "posterior")
    post.build_cache(rank=16)
    m_c, v_c = post.predict_f(Xnew, var="cache")
    m_0, none = post.predict_f(Xnew, var=False)
    m_y, v_y = post.predict_y(Xnew, var="cache")
    assert none is None and np.array_equal(m_c, m_0) and np.array_equal(m_y, m_0)
    assert np.array_equal(v_y, v_c + np.asarray(post.noise_var, dtype=v_c.dtype)) and abs(post.noise_var - noise_var) <= 1e-6
    sel = np.argsort(v_c - v_true)[-8:]          # the 8 points where the rank-16 cache is loosest
    m_s, v_s = post.predict_f(Xnew[sel], var=True)
    if dtype == "float64":
        bound = np.full(8, 1e-5)
    else:
        inv_norm = 1.0 / np.linalg.eigvalsh(E.dense(X, ell, k_var, noise_var))[0]
        bound = post.tol * np.linalg.norm(k_var * E.rbf(X, Xnew[sel], ell), axis=0) * inv_norm
    err = np.abs(v_s - v_true[sel])
    print("%s var=True on 8 points: error %.3e (%.3e of its bound); the rank-16 cache is off by up to %.3e there"
          % (dtype, err.max(), (err / bound).max(), np.abs(v_c[sel] - v_true[sel]).max()))
    assert np.array_equal(m_s, m_0[:, sel]) and np.all(err <= bound)
    assert np.abs(v_c[sel] - v_true[sel]).max() > bound.max()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_acquisition_argmax_and_suggest_agree(dtype):
    """acquisition is the restatement's tail at predict_f(var='cache')'s own moments (to the rounding of those moments:
    here only finiteness and the arg-max are asserted -- the tail itself is pinned above); argmax returns numpy's first
    maximum of it and its value; ExactGPR.suggest returns that candidate, the incumbent it used and the cache's info."""
    X, Y, ell, k_var, noise_var, Xnew = _case(dtype)
    m = _fit(dtype)
    post = object.__getattribute__(m, "posterior")
    post.build_cache(rank=64)
    mean_X, _ = post.predict_f(X, var=False)
    for kind, largest, kw in (("ei", True, dict(param=0.01)), ("pi", False, dict(param=0.0)), ("ucb", True, dict(param=2.0))):
        best = float(mean_X.max() if largest else mean_X.min())
        val = post.acquisition(Xnew, kind, best=best, largest=largest, **kw)
        idx, top = post.argmax(Xnew, kind, best=best, largest=largest, **kw)
        x_next, value, info = m.suggest(Xnew, kind=kind, largest=largest, **kw)
        print("%s %s largest=%s: best candidate %d, value %.6e, incumbent %.4f" % (dtype, kind, largest, idx, top, best))
        assert val.shape == (256,) and val.dtype == NP[dtype] and np.all(np.isfinite(val))
        assert idx == int(np.argmax(val)) and top == val[idx]
        assert info["index"] == idx and value == val[idx] and info["best"] == best and info["cache"]["rank"] == 64
        assert np.array_equal(x_next, Xnew[idx].astype(NP[dtype]))
    with pytest.raises(ValueError, match="incumbent"):
        post.acquisition(Xnew, "ei")
    two = object.__getattribute__(m, "gp").condition(X, np.concatenate([Y, -Y], axis=1), noise_var, k_var=k_var).build_cache(rank=16)
    m2, v2 = two.predict_f(Xnew[:5], var="cache")
    assert m2.shape == (2, 5) and v2.shape == (5,)
    with pytest.raises(NotImplementedError, match="one latent function only"):
        two.argmax(Xnew, "ucb", param=2.0)


def test_suggest_builds_the_cache_it_needs():
    X, Y, ell, k_var, noise_var, Xnew = _case()
    m = ExactGPR(X=X[:200], Y=Y[:200], dtype="float32")
    m.gp.kern.lengthscales = ell.copy()
    m.var = np.ones(1) * noise_var
    with pytest.raises(ValueError, match="fit"):
        m.suggest(Xnew)
    m.fit(cache_rank=None)
    assert object.__getattribute__(m, "posterior").cache_info is None
    x_next, value, info = m.suggest(Xnew, cache_rank=32)
    assert info["cache"]["rank"] == 32 and info["cache"]["asked"] == 32 and x_next.shape == (2,) and value >= 0.0
    m.fit(cache_rank=48)
    assert object.__getattribute__(m, "posterior").cache_info["asked"] == 48
