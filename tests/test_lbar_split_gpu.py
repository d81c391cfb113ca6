"""The K-split of sgp_lbar_frag_kernel in quarter-strips.

sgp_lbar_frag_kernel deals the 4 nS quarter-strips (8 data columns each) of the data axis to S slabs and to the four
waves of a workgroup in units of `lbar_gran` quarter-strips: 1 by default, 4 = whole strips (the split before).  A wave
walks its range in groups of four; groups are not aligned to strips, and a range that is no multiple of four starts
with a short group of 1-3.

Lbar (hb_sgp_bwd) and Phi (hb_sgp_bwd_phi) are held to the float64 product formed from the device's own W, A, v, u and
fbar, worst 32 x 32 tile, at the Lbar bound of tests/test_fp32_parity_gpu.py: one quarter-strip left out or taken twice
is an error of order 1/Q, orders above it.  The shapes are the smallest at which each edge of the split exists.  The
two granularities must agree to the same bound, and ubar / zbar / ellbar, which do not pass through the contraction, bit
for bit.  The bf16x3 contraction takes 16 columns per MFMA: its finest unit is the half-strip (`lbar_gran` 1 gives 2)."""
import numpy as np
import pytest
import torch

from parity import observe, tile_err

pytestmark = pytest.mark.gpu
F32 = torch.float32
BOUND = 1e-5      # test_fp32_parity_gpu.py: Lbar, native and bf16x3 alike


@pytest.fixture(scope="module")
def H():
    from henbun_amd import hip_ops

    assert torch.cuda.is_available()
    return hip_ops


def dev(a):
    return torch.as_tensor(np.asarray(a), dtype=F32).cuda().contiguous()


def host(t):
    return t.detach().double().cpu().numpy()


_CASES = {}


def case(H, M, n, d, P, bf3=False):
    """The problem of tests/test_phi_direct_gpu.py at one shape: inputs, the forward's outputs on the device and the
    float64 references, built once and shared."""
    key = (M, n, d, P, bf3)
    if key in _CASES:
        return _CASES[key]
    pr = H.PREC_BF16X3 if bf3 else H.PREC_NATIVE
    rng = np.random.RandomState(11 + M + n)
    z = np.cumsum(1.5 * (0.75 + 0.5 * rng.rand(M, 1)), axis=0) * np.ones((1, d))
    if d > 1:
        z = z + 0.3 * rng.randn(M, d)
    ell = np.exp(0.1 * rng.randn(d))
    x = z[rng.randint(0, M, n)] + 0.7 * rng.randn(n, d)
    u, eps, fbar = rng.randn(P, M), rng.randn(n), rng.randn(P, n)
    K = H.gram_fwd(dev(z), dev(z), dev(ell), diag_add=0.1).reshape(M, M)
    frag = torch.zeros((5 if bf3 else 2) * M * M, dtype=F32, device="cuda")
    L, W, info = H.cholesky_inverse(K, frag=frag, frag_bf16x3=bf3)
    assert info.item() == 0
    assert H.sgp_strip_path(1, n, M, d, P, pr)
    args = (dev(x), dev(z), dev(ell), W.reshape(M, M), dev(u))
    a_frag = torch.zeros(H.sgp_frag_elems(1, n, M, pr), dtype=F32, device="cuda")
    f, A, v, _ = H.sgp_fwd(*args, eps_in=dev(eps), wfrag=frag, a_frag=a_frag, prec=pr)   # row-major A too: the reference's operand
    torch.cuda.synchronize()
    # float64, from the device's own W, A and v:  Abar = u^T fbar + A diag(c),  c = -eps sign(v) / sqrt|v| * sum_p fbar_p
    Ad, vd, Wd = host(A).reshape(M, n), host(v).reshape(n), host(W).reshape(M, M)
    ud, fd, ed = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (u, fbar, eps))
    c = np.where(np.abs(vd) > 0, -ed * np.sign(vd) / np.sqrt(np.maximum(np.abs(vd), 1e-300)) * fd.sum(0), 0.0)
    Abar = ud.T @ fd + Ad * c[None, :]
    Q = -Abar @ Ad.T
    i, j = np.indices((M, M))
    ref_phi = 0.5 * Q[np.maximum(i, j), np.minimum(i, j)]
    ref_lbar = np.tril(Wd.T @ Q)
    res = dict(pr=pr, args=args, bargs=(dev(eps), None, v, dev(fbar)), frag=frag, a_frag=a_frag, f=f, A=A, v=v,
               ref_lbar=ref_lbar, ref_phi=ref_phi)
    _CASES[key] = res
    return res


def backward(H, c, phi):
    a, b = c["args"], c["bargs"]
    if phi:
        out = H.sgp_bwd_phi(a[0], a[1], a[2], a[3], a[4], b[0], b[2], b[3], c["frag"], c["a_frag"])
    else:
        out = H.sgp_bwd(*(a + b), wfrag=c["frag"], a_frag=c["a_frag"], prec=c["pr"])[:4]
    torch.cuda.synchronize()
    return out


SHAPES = [(96, 70, 2, 1, 0),       # nS = 3, Q = 12, S = 1: three quarter-strips per wave (tail-only groups), columns past n,
                                   # an odd tile count with a single-tile block
          (128, 257, 1, 3, 0),     # Q = 36, 9 per wave: two groups and a tail of 1
          (128, 1184, 1, 1, 3),    # Q = 148, slabs 50 / 49 / 49: waves of 13 and 12, tails of 1 ...
          (128, 1184, 1, 1, 5),    # ... slabs 30 / 30 / 30 / 29 / 29: waves of 8 and 7, tails of 3
          (64, 40, 1, 1, 0),       # Q = 8 over four waves: two quarter-strips each, no full group anywhere
          (512, 2048, 1, 1, 0)]    # the block structure of cfg 2: 36 blocks, S = 7, slabs 37 / 37 / 37 / 37 / 36 / 36 / 36


def _both_granularities(H, c, phi, force_s):
    res = {}
    try:
        H.debug_set("lbar_force_s", force_s)
        for gran in (1, 4):
            H.debug_set("lbar_gran", gran)
            res[gran] = backward(H, c, phi)
    finally:
        H.debug_set("lbar_gran", 1)
        H.debug_set("lbar_force_s", 0)
    return res


@pytest.mark.parametrize("phi", [False, True], ids=["lbar", "phi"])
@pytest.mark.parametrize("M,n,d,P,force_s", SHAPES)
def test_quarter_strip_split_against_fp64(H, M, n, d, P, force_s, phi):
    if phi:
        assert H.sgp_bwd_phi_supported(1, n, M, d, P)
    c = case(H, M, n, d, P)
    res = _both_granularities(H, c, phi, force_s)
    ref = c["ref_phi"] if phi else c["ref_lbar"]
    tag = "lbar_split/%s[M%d,n%d,d%d,P%d,S%d]/" % ("Phi" if phi else "Lbar", M, n, d, P, force_s)
    got = {g: host(res[g][0]).reshape(M, M) for g in (1, 4)}
    errs = {g: tile_err(got[g], ref) for g in (1, 4)}
    between = tile_err(got[1], got[4])
    print("%s gran 1: %.3e   gran 4: %.3e   between: %.3e   (bound %.0e)" % (tag, errs[1], errs[4], between, BOUND))
    for g in (1, 4):
        assert np.isfinite(got[g]).all()
        if phi:
            assert np.array_equal(got[g], got[g].T)
        else:
            assert np.all(np.triu(got[g], 1) == 0)
        observe(tag + "gran%d" % g, errs[g], BOUND)
    observe(tag + "gran1_vs_gran4", between, BOUND)
    # ubar, zbar, ellbar never pass through the contraction
    for k in (1, 2, 3):
        assert torch.equal(res[1][k], res[4][k]), k


@pytest.mark.parametrize("M,n,d,P,force_s", [SHAPES[0], SHAPES[2]])
def test_half_strip_split_bf16x3_against_fp64(H, M, n, d, P, force_s):
    c = case(H, M, n, d, P, bf3=True)
    res = _both_granularities(H, c, False, force_s)
    tag = "lbar_split/bf16x3/Lbar[M%d,n%d,d%d,P%d,S%d]/" % (M, n, d, P, force_s)
    got = {g: host(res[g][0]).reshape(M, M) for g in (1, 4)}
    errs = {g: tile_err(got[g], c["ref_lbar"]) for g in (1, 4)}
    between = tile_err(got[1], got[4])
    print("%s gran 1: %.3e   gran 4: %.3e   between: %.3e   (bound %.0e)" % (tag, errs[1], errs[4], between, BOUND))
    for g in (1, 4):
        assert np.all(np.triu(got[g], 1) == 0)
        observe(tag + "gran%d" % g, errs[g], BOUND)
    observe(tag + "gran1_vs_gran4", between, BOUND)
    for k in (1, 2, 3):
        assert torch.equal(res[1][k], res[4][k]), k
