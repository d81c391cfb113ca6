"""hb_gram_cholesky_inverse_f32, the persistent Cholesky that synthesises K(z, z) + jitter I from the points, held to the
promise of header and source: "the same function, the same bits" as hb_gram_fwd (diag_add = jitter) followed by
hb_cholesky_inverse -- L, W, info and both fragment images, across kinds, d, ARD, batched points and batched
lengthscales over shared points, with power-of-two and with general lengthscales -- and both to numpy float64 on
well-conditioned points (tests/parity.py; the bounds are those of test_fp32_cholesky_inverse_chain_against_fp64: the
same factorisation on the same kind of matrix)."""
import numpy as np
import pytest
import torch

from henbun_amd import _lib
from henbun_amd import hip_ops as H

import gram_ref
from parity import observe, tile_err

pytestmark = pytest.mark.gpu
F32 = torch.float32
JITTER = float(np.float32(0.1))
KINDS = {"rbf": (H.KERN_RBF, gram_ref.RBF), "csym": (H.KERN_CSYM_RBF, gram_ref.CSYM)}
# (B, M, d, dl, points batched, lengthscales): (3, 64, 2, 2) shares its points among three lengthscale vectors (sX = 0,
# sEll = dl).
# These lengthscales are powers of two, for the float64 bounds: x / ell is then exact in fp32, and so is the difference of
# two scaled coordinates that lie within a factor of two of each other (any neighbours here).  With a general lengthscale
# the kernels round x / ell before they subtract (tests/gram_ref.py), an absolute error of 2^-24 (|a| + |b|) in a - b: at
# |a| ~ 200 that alone is 3e-5 relative in K -- the Gram matrix's own forward error for such inputs, fifteen times the
# bound on L, and nothing the factorisation can be held to.  Powers of two also hide what the "same bits" promise is
# most exposed to -- a reciprocal or a contracted multiply-subtract at one of the two sites where gram_value is inlined
# rounds only when x / ell does -- so the bit-for-bit comparison runs a second time, on general lengthscales (below).
CASES = [(1, 64, 1, 1, False, [1.0]),
         (1, 128, 3, 3, False, [1.0, 2.0, 0.5]),
         (2, 192, 2, 1, True, [1.0]),
         (3, 64, 2, 2, False, [[1.0, 2.0], [1.0, 0.5], [0.5, 1.0]]),
         (1, 64, 5, 5, False, [1.0, 2.0, 0.5, 1.0, 2.0]),
         (1, 512, 1, 1, False, [1.0])]
CASE_IDS = ["B%d-M%d-d%d-dl%d" % c[:4] for c in CASES]


def points(B, M, d, batched, ell, spacing=1.5):
    """Sorted points ~`spacing` lengthscales apart along the first axis, as well_conditioned_gram of
    test_fp32_parity_gpu builds them, shifted so that the first sits at 0.25: the mirror term of the centrally symmetric
    kernel is then of order one for the first point (0.88 on the diagonal, ~0.2 against its neighbour) instead of
    vanishing everywhere; further axes uniform in [0, 1.5); `ell` as [1 or B, dl]; everything rounded to fp32.
    cond(K + 0.1 I) on these points with the lengthscales of CASES: RBF 3.1 .. 8.2, CSYM-RBF 3.1 .. 8.9 (computed on
    the host; the test asserts < 1e2)."""
    rng = np.random.RandomState(1000 * M + 10 * d + B)
    nb = B if batched else 1
    z = np.cumsum(spacing * (0.75 + 0.5 * rng.rand(nb, M, 1)), axis=1)
    z = z - z[:, :1] + 0.25
    if d > 1:
        z = np.concatenate([z, 1.5 * rng.rand(nb, M, d - 1)], axis=-1)
    ell = np.atleast_2d(np.asarray(ell, dtype=np.float64))
    return z.astype(np.float32), ell.astype(np.float32)


def general_lengthscales(case):
    """Lengthscales of the case's own shape (one vector, or one per batch item), uniform in [0.7, 1.4] and rounded to
    fp32: none a power of two, so 1 / ell, x / ell and x * (1 / ell) all round, each differently."""
    B, M, d, dl = case[:4]
    shape = np.atleast_2d(np.asarray(case[5])).shape
    ell = np.random.RandomState(7000 + 1000 * M + 10 * d + B).uniform(0.7, 1.4, size=shape).astype(np.float32)
    mant = np.frexp(ell)[0]
    assert shape[1] == dl and np.all(mant != 0.5)
    return ell


def reference(kind, z, ell, B, M):
    """K + jitter I, its Cholesky factor and the factor's inverse in float64, [B, M, M]"""
    K, _ = gram_ref.gram(kind, z.astype(np.float64), z.astype(np.float64), ell.astype(np.float64))
    K = np.broadcast_to(K, (B, M, M)) + JITTER * np.eye(M)
    L = np.linalg.cholesky(K)
    return K, L, np.linalg.inv(L)


def both_paths(hk, z, ell, B, M, batched):
    """hb_gram_cholesky_inverse_f32 and gram_fwd + cholesky_inverse on the same points: asserts equal bits of L, W, info
    and both fragment images (plain and bf16x3); returns the two pairs (L, W) as float64 [B, M, M]."""
    X = torch.from_numpy(z if batched else z[0]).cuda()
    el = torch.from_numpy(ell if ell.shape[0] > 1 else ell[0]).cuda()
    for bf3 in (False, True):
        ne = H.cholesky_frag_elems(B, M, bf3)
        frag1 = torch.full((ne,), -7.0, dtype=F32, device="cuda")
        frag2 = torch.full((ne,), -7.0, dtype=F32, device="cuda")
        L1, W1, info1 = H.gram_cholesky_inverse(X, el, JITTER, kind=hk, frag=frag1, frag_bf16x3=bf3)
        K2 = H.gram_fwd(X, X, el, kind=hk, diag_add=JITTER)
        L2, W2, info2 = H.cholesky_inverse(K2, frag=frag2, frag_bf16x3=bf3)
        torch.cuda.synchronize()
        assert not info1.cpu().numpy().any() and torch.equal(info1, info2)
        assert torch.equal(L1.reshape(B, M, M), L2.reshape(B, M, M)), "L differs from gram_fwd + cholesky_inverse"
        assert torch.equal(W1.reshape(B, M, M), W2.reshape(B, M, M)), "W differs from gram_fwd + cholesky_inverse"
        assert torch.equal(frag1, frag2), "fragment images differ (bf16x3 = %s)" % bf3
        assert not torch.isnan(frag1).any()
    h = lambda t: t.double().cpu().numpy().reshape(B, M, M)
    return (h(L1), h(W1)), (h(L2), h(W2))


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gram_fed_cholesky_equals_the_two_step_path_bit_for_bit(kind, case):
    B, M, d, dl, batched, ell = case
    hk, rk = KINDS[kind]
    z, ell = points(B, M, d, batched, ell)
    Kr, Lr, Wr = reference(rk, z, ell, B, M)
    assert max(np.linalg.cond(Kr[b]) for b in range(B)) < 1e2
    assert H.cholesky_persistent_shape(B, M, F32)
    (Lh, Wh), (L2, W2) = both_paths(hk, z, ell, B, M, batched)
    assert np.all(np.triu(Lh, 1) == 0) and np.all(np.triu(Wh, 1) == 0)
    eL, eW = tile_err(Lh, Lr), tile_err(Wh, Wr)
    print("gram_cholesky[%s,B%d,M%d,d%d,dl%d]: L %.2e  W %.2e" % (kind, B, M, d, dl, eL, eW))
    observe("gram_cholesky/%s/L[%d,%d,%d]" % (kind, B, M, d), eL, 2e-6)
    observe("gram_cholesky/%s/W[%d,%d,%d]" % (kind, B, M, d), eW, 3e-6)
    # the two-step path against the same reference (equal bits make this the same number; stated for a failure's sake)
    observe("gram_fwd+cholesky/%s/L[%d,%d,%d]" % (kind, B, M, d), tile_err(L2, Lr), 2e-6)
    observe("gram_fwd+cholesky/%s/W[%d,%d,%d]" % (kind, B, M, d), tile_err(W2, Wr), 3e-6)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gram_fed_cholesky_keeps_the_same_bits_with_general_lengthscales(kind, case):
    """The same cases and the same assertions of equal bits (L, W, info, both fragment images) with lengthscales that
    are no powers of two -- single, ARD, and one vector per batch item over shared points: every scaled coordinate is
    then a rounded value, and a reciprocal in place of a division, or a multiply contracted into the subtraction, at
    only one of the two places that inline gram_value would change bits.  No float64 bound here (see CASES)."""
    B, M, d, dl, batched, _ = case
    z, ell = points(B, M, d, batched, general_lengthscales(case))
    assert H.cholesky_persistent_shape(B, M, F32)
    (L1, W1), _ = both_paths(KINDS[kind][0], z, ell, B, M, batched)
    assert np.all(np.triu(L1, 1) == 0) and np.all(np.triu(W1, 1) == 0)


def test_a_shape_outside_the_persistent_form_is_rejected():
    """M = 96 has no persistent form (hb_cholesky_persistent_shape == 0): an error, not another path."""
    assert not H.cholesky_persistent_shape(1, 96, F32)
    z, ell = points(1, 96, 1, False, [1.0])
    with pytest.raises(_lib.HipBackendError, match="hb_gram_cholesky_inverse"):
        H.gram_cholesky_inverse(torch.from_numpy(z[0]).cuda(), torch.from_numpy(ell[0]).cuda(), JITTER)
    torch.cuda.synchronize()
