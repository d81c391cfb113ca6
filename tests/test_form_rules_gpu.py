"""The form queries of the sparse-GP contractions and the launchers agree (csrc/sgp.hip, sgp_form): where a query says
yes, the call that relies on it succeeds and gives what the plain call gives; where it says 0, the library's own argument
check refuses the call before any launch.  The smallest shapes that reach each form: M = 32 and 64, n = 64, d = 1 and 2,
P = 1, one expert."""
import numpy as np
import pytest
import torch

from henbun_amd._lib import HipBackendError
from parity import observe, tile_err

pytestmark = pytest.mark.gpu
F32 = torch.float32
N = 64
SHAPES = [(32, 1), (64, 2)]


@pytest.fixture(scope="module")
def H():
    from henbun_amd import hip_ops

    assert torch.cuda.is_available()
    return hip_ops


def dev(a):
    return torch.as_tensor(np.asarray(a), dtype=F32).cuda().contiguous()


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=F32, device="cuda")


_cache = {}


def problem(H, M, d, P=1):
    """(x, z, ell, u, eps, y, var, K, L, W, frag): inducing points on a jittered line, W = chol(K)^-1 and its images."""
    if (M, d, P) not in _cache:
        rng = np.random.RandomState(100 * M + 10 * d + P)
        z = np.cumsum(1.5 * (0.75 + 0.5 * rng.rand(M, 1)), axis=0) * np.ones((1, d)) + (0.3 * rng.randn(M, d) if d > 1 else 0.0)
        x = z[rng.randint(0, M, N)] + 0.7 * rng.randn(N, d)
        t = dict(x=dev(x), z=dev(z), ell=dev(np.exp(0.1 * rng.randn(d))), u=dev(rng.randn(P, M)), eps=dev(rng.randn(N)),
                 y=dev(rng.randn(1, N)), var=dev([0.4]), fbar=dev(rng.randn(P, N)))
        t["K"] = H.gram_fwd(t["z"], t["z"], t["ell"], diag_add=0.1)
        t["frag"] = torch.zeros(H.cholesky_frag_elems(1, M), dtype=F32, device="cuda")
        t["L"], t["W"], info = H.cholesky_inverse(t["K"], frag=t["frag"])
        assert int(info.item()) == 0
        _cache[(M, d, P)] = t
    return _cache[(M, d, P)]


def fwd(H, t, **kw):
    return H.sgp_fwd(t["x"], t["z"], t["ell"], t["W"], t["u"], eps_in=t["eps"], wfrag=t["frag"], **kw)


def head_for(t, units, post=0.5):
    return dict(y=t["y"], scale=None, var=t["var"], post=post, dmu=nan(1, N), fbar=nan(1, N), part=nan(3 * units), units=units)


@pytest.mark.parametrize("M,d", SHAPES)
def test_head_rides_where_the_query_gives_units(H, M, d):
    t = problem(H, M, d)
    units = H.sgp_head_units(t["x"], t["z"], t["u"], H.PREC_NATIVE, True, False, None)
    assert units == N // 32
    f0, _, v0, _ = fwd(H, t)
    fb0 = nan(1, N)
    ll0, dmu0, ds0, dv0 = H.gauss_ll(t["y"], f0, None, t["var"], post=0.5, fbar=fb0)
    head = head_for(t, units)
    f1, _, v1, _ = fwd(H, t, head=head)
    ll1, ds1, dv1 = (torch.empty(1, dtype=F32, device="cuda") for _ in range(3))
    H.gauss_ll_fold(head["part"], units, ll1, ds1, dv1)
    for a, b in ((f0, f1), (v0, v1), (dmu0, head["dmu"]), (fb0, head["fbar"])):
        assert torch.equal(a.reshape(-1), b.reshape(-1))
    # (the sums are taken in another fixed order: the bound of test_likelihood_head_inside_the_forward_contraction)
    for a, b in ((ll0, ll1), (dv0, dv1)):
        print("head sum", float(a), float(b))
        assert abs(float(a) - float(b)) <= 2e-6 * max(abs(float(a)), float(N) ** 0.5)


@pytest.mark.parametrize("d", [1, 2])
def test_recorded_forward_rides_where_the_query_says_so(H, d):
    M = 64   # (the persistent factorisation starts at M = 64)
    t = problem(H, M, d)
    assert H.sgp_rider_supported(t["x"], t["z"], t["u"], H.PREC_NATIVE, True, False, None)

    def run(early):
        L, W, frag = torch.empty_like(t["K"]), torch.empty_like(t["K"]), torch.empty_like(t["frag"])
        info = torch.zeros(1, dtype=torch.int32, device="cuda")
        afrag = nan(H.sgp_frag_elems(1, N, M))
        out = (nan(1, N), nan(M, N), nan(N), nan(N))
        call = lambda: H.sgp_fwd(t["x"], t["z"], t["ell"], W, t["u"], eps_in=t["eps"], out=out, wfrag=frag, a_frag=afrag, skip_a=True)
        if early:
            H.sgp_rider_begin()
            call()
            assert H.sgp_rider_pending() == 1
            H.cholesky_inverse(t["K"], out=L, inv=W, info=info, frag=frag)
            assert H.sgp_rider_pending() == 0
        else:
            H.cholesky_inverse(t["K"], out=L, inv=W, info=info, frag=frag)
            call()
        torch.cuda.synchronize()
        assert int(info.item()) == 0
        return dict(L=L, W=W, frag=frag, f=out[0], v=out[2], afrag=afrag)

    ref, got = run(False), run(True)
    for k in ("L", "W", "frag"):
        assert torch.equal(ref[k], got[k]), k
    for k in ("f", "v", "afrag"):
        err = float((ref[k].double() - got[k].double()).abs().max() / ref[k].double().abs().max())
        print("rider", k, err)
        assert err <= 3e-4, (k, err)   # the bound of test_forward_contraction_inside_the_persistent_cholesky_launch


@pytest.mark.parametrize("M,d", SHAPES)
def test_fragment_major_a_where_the_strip_path_is_taken(H, M, d):
    t = problem(H, M, d)
    assert H.sgp_strip_path(1, N, M, d, 1, H.PREC_NATIVE)
    f0, A0, v0, _ = fwd(H, t)
    afrag = nan(H.sgp_frag_elems(1, N, M))
    f1, A1, v1, _ = fwd(H, t, a_frag=afrag)
    for a, b in ((f0, f1), (A0, A1), (v0, v1)):
        assert torch.equal(a, b)
    # A_frag [M/32 t][n/32 s][4 v][64 lanes = li + 32 h][4 s'] = A[32 t + li][32 s + 16 h + 4 v + s']  (include/henbun_hip.h)
    want = A0.reshape(M // 32, 32, N // 32, 2, 4, 4).permute(0, 2, 4, 3, 1, 5).reshape(-1)   # (t, li, s, h, v, s') -> (t, s, v, h, li, s')
    assert torch.equal(afrag, want)


@pytest.mark.parametrize("M,d", SHAPES)
def test_phi_direct_backward_where_the_query_says_so(H, M, d):
    t = problem(H, M, d)
    assert H.sgp_bwd_phi_supported(1, N, M, d, 1)
    afrag = torch.zeros(H.sgp_frag_elems(1, N, M), dtype=F32, device="cuda")
    f, A, v, _ = fwd(H, t, a_frag=afrag)
    args = (t["x"], t["z"], t["ell"], t["W"], t["u"])
    Lb, ub, zb, lb, _ = H.sgp_bwd(*args, t["eps"], None, v, t["fbar"], wfrag=t["frag"], a_frag=afrag)
    Phi, ub2, zb2, lb2 = H.sgp_bwd_phi(*args, t["eps"], v, t["fbar"], t["frag"], afrag)
    torch.cuda.synchronize()
    assert torch.equal(ub2, ub) and torch.equal(zb2, zb) and torch.equal(lb2, lb)
    # Phisym(-Abar A^T) in float64 from the device's own A and v, as tests/test_phi_direct_gpu.py forms it
    Ad, vd = A.double().cpu().numpy(), v.double().cpu().numpy()
    ud, fd, ed = (t[k].double().cpu().numpy() for k in ("u", "fbar", "eps"))
    c = np.where(np.abs(vd) > 0, -ed * np.sign(vd) / np.sqrt(np.maximum(np.abs(vd), 1e-300)) * fd.sum(0), 0.0)
    Q = -(ud.T @ fd + Ad * c[None, :]) @ Ad.T
    i, j = np.indices((M, M))
    got = Phi.double().cpu().numpy().reshape(M, M)
    assert np.isfinite(got).all() and np.array_equal(got, got.T)
    observe("form_rules/Phi[M%d,d%d]" % (M, d), tile_err(got, 0.5 * Q[np.maximum(i, j), np.minimum(i, j)]), 1e-5)


def test_calls_the_queries_answer_zero_for_are_refused_before_any_launch(H):
    # P = 2 with a head
    t = problem(H, 64, 1, P=2)
    assert H.sgp_head_units(t["x"], t["z"], t["u"], H.PREC_NATIVE, True, False, None) == 0
    with pytest.raises(HipBackendError):
        fwd(H, t, head=head_for(t, N // 32))
    # d = 5 with a fragment-major A
    t = problem(H, 64, 5)
    assert not H.sgp_strip_path(1, N, 64, 5, 1, H.PREC_NATIVE)
    with pytest.raises(HipBackendError):
        fwd(H, t, a_frag=nan(H.sgp_frag_elems(1, N, 64)))
    # d = 3 after sgp_rider_begin
    t = problem(H, 64, 3)
    assert not H.sgp_rider_supported(t["x"], t["z"], t["u"], H.PREC_NATIVE, True, False, None)
    H.sgp_rider_begin()
    try:
        with pytest.raises(HipBackendError):
            fwd(H, t)
        assert H.sgp_rider_pending() == 0
    finally:
        H.sgp_rider_flush()   # (disarms the recorder: nothing was recorded, nothing is launched)
    torch.cuda.synchronize()
