"""hb_gram_bilinear_grad on the GPU against the numpy restatement tests/exact_mll_ref.py (bilinear_grad, pinned on the
host by tests/test_exact_mll_cpu.py).

Bounds, per component theta of g, with M_theta = sum_s |w_s| sum_ij |A_si| |B_sj| K_ij D^theta_ij (D = 1 for g[0],
(x_ik - x_jk)^2 / ell_k^3 for g[1 + k], summed over k for one lengthscale):
  float64:  1e-11 M_theta, the convention of the product's test.
  float32:  k 2^-24 M_theta, k counted from the operation sequence on inputs that are exact in float32, as
            test_gram_matvec_gpu.py counts it.  K_ij: 11 + d (the difference 1, the scale s / ell 2, their product 1 -- 4 on
            t, 9 on t^2; the d - 1 additions of r^2: 9 + d; v_exp_f32 2).  W_ij = sum_s (w_s B_sj) A_si: 1 for the rounding of
            w_s B_sj (the product itself is formed in double) and min(S, 64) for the fp32 fma chain of one block of pairs on
            the MFMA (the blocks are added in double).  W_ij K_ij, its product with t_k^2 or r^2 and every sum after them are
            double, exact or at the 2^-53 level: 1 covers them.  So k_0 = (11 + d) + min(S, 64) + 2 for g[0]; the lengthscale
            components carry the error of their own factor as well, t_k^2: 9 (ARD), r^2: 9 + d (one lengthscale).
            (As in the product's test the exponential's amplification of the error of r^2 is not in the count: the chain's
            count is a worst case the rounding errors come nowhere near.)
Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from henbun_amd import _lib, hip_ops as H

import exact_mll_ref as R

pytestmark = pytest.mark.gpu

TORCH = {"float64": torch.float64, "float32": torch.float32}
CHUNK, GROUP = 2048, 16       # hb_gram_matvec_chunk() and the chunks per launch: the shapes straddle both

# (N, S, d, dl)
CASES = [
    (1, 1, 1, 1),
    (33, 1, 1, 1),
    (127, 15, 3, 3),
    (128, 16, 4, 1),
    (129, 64, 4, 4),
    (129, 65, 2, 2),                  # two blocks of pairs
    (130, 17, 5, 5),                  # d > 4, ARD: two groups of dimensions, the memory path
    (130, 17, 5, 1),
    (CHUNK - 1, 17, 2, 2),
    (CHUNK, 17, 2, 2),
    (CHUNK + 1, 17, 2, 2),
    (2 * CHUNK + 5, 3, 2, 1),         # three chunks
    (GROUP * CHUNK + 5, 1, 1, 1),     # 17 chunks: two groups of launches, the fold carries its sum across
]
_CASE = {}


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


def _inputs(case):
    """x ~ U(0, 4)^d, the lengthscales of test_gram_matvec_gpu.py, A, B standard normal, w of mixed signs; all but w
    rounded to float32, so that ONE float64 reference serves both dtypes."""
    N, S, d, dl = case
    rng = np.random.default_rng(N + 3 * S + 7 * d + dl)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    x = f32(rng.uniform(0.0, 4.0, (N, d)))
    ell = f32(np.array([0.8]) if dl == 1 else 0.7 + 0.2 * np.arange(d))
    A, B = f32(rng.standard_normal((S, N))), f32(rng.standard_normal((S, N)))
    w = rng.uniform(0.5, 1.5, S) * np.where(np.arange(S) % 3 == 1, -1.0, 1.0)
    return x, ell, A, B, w


def _case(case):
    if case not in _CASE:
        x, ell, A, B, w = _inputs(case)
        g, M = R.bilinear_grad(x, ell, A, B, w, magnitude=True)
        _CASE[case] = (x, ell, A, B, w, g, M)
    return _CASE[case]


def _bound(dtype, case, M):
    N, S, d, dl = case
    if dtype == "float64":
        return 1e-11 * M
    k0 = (11 + d) + min(S, 64) + 2
    k = np.array([k0] + [k0 + 9 + (d if dl == 1 else 0)] * dl, dtype=np.float64)
    return k * 2.0 ** -24 * M


def _run(x, ell, A, B, w, dt):
    return H.gram_bilinear_grad(dev(x, dt), dev(ell, dt), dev(A, dt), dev(B, dt), w)


def test_the_constants_are_the_ones_the_shapes_straddle():
    assert H.gram_matvec_chunk() == CHUNK
    assert H.gram_bilinear_grad_ws_elems(GROUP * CHUNK + 5, 1) == GROUP * 257 * 2


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d-S%d-d%d-dl%d" % c)
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_contraction_against_the_restatement(dtype, case):
    x, ell, A, B, w, ref, M = _case(case)
    out = _run(x, ell, A, B, w, TORCH[dtype])
    again = _run(x, ell, A, B, w, TORCH[dtype])
    torch.cuda.synchronize()
    assert out.dtype == torch.float64 and tuple(out.shape) == (1 + case[3],)
    got = out.cpu().numpy()
    assert np.all(np.isfinite(got))
    err, bound = np.abs(got - ref), _bound(dtype, case, M)
    ratio = err / np.where(bound > 0.0, bound, 1.0)          # (N = 1: the lengthscale component and its bound are zero)
    print("gram_bilinear_grad %s %s: error / bound per component %s" % (dtype, case, np.array2string(ratio, precision=3)))
    assert torch.equal(out, again)
    assert np.all(err <= bound)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_a_weighted_quadratic_form_of_k_is_positive(dtype):
    """A = B, w > 0: g[0] = sum_s w_s a_s^T K a_s > 0, K being positive definite."""
    x, ell, A, _, w, _, _ = _case(CASES[4])
    out = _run(x, ell, A, A, np.abs(w), TORCH[dtype]).cpu().numpy()
    print("quadratic form %s: %r" % (dtype, out))
    assert out[0] > 0.0


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_blocks_of_pairs_add_up(dtype):
    """S = 65: the call equals the sum of the calls on pairs 0..63 and on pair 64 to 1e-12 M (the blocks are added in
    double in that order)."""
    x, ell, A, B, w, _, M = _case(CASES[5])
    dt = TORCH[dtype]
    whole = _run(x, ell, A, B, w, dt).cpu().numpy()
    parts = _run(x, ell, A[:64], B[:64], w[:64], dt).cpu().numpy() + _run(x, ell, A[64:], B[64:], w[64:], dt).cpu().numpy()
    print("blocks of pairs %s: difference / (1e-12 M) %s" % (dtype, np.array2string(np.abs(whole - parts) / (1e-12 * M), precision=3)))
    assert np.all(np.abs(whole - parts) <= 1e-12 * M)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_unit_weights_agree_with_the_matrix_free_product(dtype):
    """w = 1: g[0] = sum_s sum_j A_sj (B_s K)_j with B K from hb_gram_matvec (K is symmetric), within the two bounds added:
    the product's bound per element (tests/test_gram_matvec_gpu.py) weighted by |A_sj| and summed."""
    case = CASES[4]
    N, S, d, dl = case
    x, ell, A, B, _, _, _ = _case(case)
    dt = TORCH[dtype]
    one = np.ones(S)
    g0 = float(_run(x, ell, A, B, one, dt).cpu().numpy()[0])
    BK = H.gram_matvec(dev(x, dt), None, dev(ell, dt), dev(B, dt)).cpu().numpy().astype(np.float64)
    _, M = R.bilinear_grad(x, ell, A, B, one, magnitude=True)
    if dtype == "float64":
        bound = 1e-11 * M[0] + 1e-11 * float((np.abs(A) * np.abs(B).sum(1, keepdims=True)).sum())
    else:
        bound = _bound(dtype, case, M)[0] + ((11 + d) + min(N, CHUNK) + 1) * 2.0 ** -24 * M[0]
    diff = abs(g0 - float((A * BK).sum()))
    print("against gram_matvec %s: difference %.3e, %.3e of the bounds' sum" % (dtype, diff, diff / bound))
    assert diff <= bound


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_no_rows_gives_zeros(dtype):
    dt = TORCH[dtype]
    out = torch.full((3,), float("nan"), dtype=torch.float64, device="cuda")
    e = torch.empty((2, 0), dtype=dt, device="cuda")
    H.gram_bilinear_grad(torch.empty((0, 2), dtype=dt, device="cuda"), dev(np.ones(2), dt), e, e, np.ones(2), out=out)
    torch.cuda.synchronize()
    assert not out.any()


def test_bad_arguments_never_reach_a_launch():
    dt = torch.float32
    x, A, ell = dev(np.ones((5, 3)), dt), dev(np.ones((2, 5)), dt), dev(np.ones(1), dt)
    out = torch.full((2,), float("nan"), dtype=torch.float64, device="cuda")
    with pytest.raises(_lib.HipBackendError, match="UnitRBF"):
        H.gram_bilinear_grad(x, ell, A, A, np.ones(2), out=out, kind=H.KERN_SQDIST)
    with pytest.raises(_lib.HipBackendError, match="lengthscales"):
        H.gram_bilinear_grad(x, dev(np.ones(2), dt), A, A, np.ones(2))
    with pytest.raises(TypeError, match="dtype"):
        H.gram_bilinear_grad(x, ell, A, A.double(), np.ones(2), out=out)
    with pytest.raises(ValueError):
        H.gram_bilinear_grad(x, ell, A, dev(np.ones((2, 4)), dt), np.ones(2), out=out)
    with pytest.raises(ValueError, match="w must"):
        H.gram_bilinear_grad(x, ell, A, A, np.ones(3), out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
