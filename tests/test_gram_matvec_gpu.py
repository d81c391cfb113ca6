"""hb_gram_matvec on the GPU against the numpy restatement tests/exact_gp_ref.py (pinned on the host by
tests/test_exact_gp_cpu.py).

Bounds, per output element (s, j), with A_s = sum_i |V_si| and W_sj = sum_i |V_si| K_ij:
  float64:  1e-11 (|scale| A_s + |shift V_sj|).
  float32:  (k + min(N, CHUNK) + 1) 2^-24 (|scale| W_sj + |shift V_sj|), k = 11 + d, counted from the operation sequence on
            inputs that are exact in float32: the difference z - x 1, the scale s / ell 2 (the constant, the division), their
            product 1 -- 4 on t, 9 on t^2; the d - 1 additions of r^2 bring it to at most 9 + d; v_exp_f32 2.  min(N, CHUNK) is
            the fp32 fma chain of one chunk on the MFMA (the chunks are added in double) and 1 the rounding of the result.
            (The exponential turns a relative error of r^2 into r^2 / 2 times as much of K, which tests/gram_ref.py carries
            as a weight 1 + r^2 / 2 on K_ij; the bound here has K_ij alone -- the tighter form -- and holds: the chain's
            count is a worst case the rounding errors come nowhere near.)
Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from henbun_amd import _lib, hip_ops as H

import exact_gp_ref as E

pytestmark = pytest.mark.gpu

TORCH = {"float64": torch.float64, "float32": torch.float32}
NP = {"float64": np.float64, "float32": np.float32}
CHUNK = 2048          # hb_gram_matvec_chunk(), asserted below: the shapes straddle it


def dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()


# (n, N, S, d, dl, symmetric, scale, shift): every (n, N) pair, S, d and dl the kernel treats differently appears; the
# chunk-straddling shapes come with S = 17 and d = 5 (the memory path); the symmetric form takes N = n
CASES = [
    (1, 1, 1, 1, 1, False, 1.0, 0.0),
    (127, 33, 15, 3, 3, False, 1.7, 0.0),
    (128, 32, 16, 4, 1, False, 1.0, 0.0),
    (129, 31, 64, 3, 1, False, -0.6, 0.0),
    (129, 31, 65, 4, 4, False, 1.7, 0.0),
    (300, 300, 17, 1, 1, True, 1.7, 0.3),
    (33, 33, 16, 5, 5, True, 0.5, 0.01),
    (300, CHUNK - 1, 17, 5, 5, False, 1.7, 0.0),
    (300, CHUNK, 17, 5, 1, False, 1.7, 0.0),
    (130, CHUNK + 1, 17, 5, 5, False, 1.7, 0.0),
    (257, 2 * CHUNK + 5, 17, 5, 5, False, 1.7, 0.0),
    (CHUNK + 1, CHUNK + 1, 17, 5, 5, True, 1.7, 0.3),
    (257, 2 * CHUNK + 5, 1, 2, 2, False, 1.0, 0.0),
    (130, 16 * CHUNK + 5, 17, 2, 2, False, 1.7, 0.0),          # 17 chunks: two groups, the fold carries its sum across
]
_CASE = {}


def _case(case, dtype):
    """Inputs rounded to the dtype, the float64 restatement on them and the magnitudes of the bounds: computed once."""
    key = (case, dtype)
    if key not in _CASE:
        n, N, S, d, dl, sym, scale, shift = case
        rng = np.random.default_rng(n + 3 * N + 5 * S + 7 * d + dl)
        x = rng.uniform(0.0, 4.0, (n, d)).astype(NP[dtype])
        x2 = None if sym else rng.uniform(0.0, 4.0, (N, d)).astype(NP[dtype])
        ell = (np.array([0.8]) if dl == 1 else 0.7 + 0.2 * np.arange(d)).astype(NP[dtype])
        V = rng.standard_normal((S, N)).astype(NP[dtype])
        ref = E.matvec(x, x2, ell, V, scale, shift, CHUNK)
        A, W = E.matvec_magnitude(x, x2, ell, V)
        sv = np.abs(shift * V.astype(np.float64)) if sym else 0.0
        _CASE[key] = (x, x2, ell, V, ref, A, W, sv)
    return _CASE[key]


def _run(x, x2, ell, V, scale, shift, dt):
    return H.gram_matvec(dev(x, dt), None if x2 is None else dev(x2, dt), dev(ell, dt), dev(V, dt), scale=scale, shift=shift)


def test_the_chunk_is_the_one_the_shapes_straddle():
    assert H.gram_matvec_chunk() == CHUNK


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-N%d-S%d-d%d-dl%d-%s" % (c[0], c[1], c[2], c[3], c[4], "sym" if c[5] else "x2"))
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_product_against_the_restatement(dtype, case):
    n, N, S, d, dl, sym, scale, shift = case
    x, x2, ell, V, ref, A, W, sv = _case(case, dtype)
    out = _run(x, x2, ell, V, scale, shift, TORCH[dtype])
    torch.cuda.synchronize()
    assert out.shape == ref.shape and out.dtype == TORCH[dtype]
    got = out.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got))
    err = np.abs(got - ref)
    if dtype == "float64":
        bound = 1e-11 * (abs(scale) * A + sv)
    else:
        count = (11 + d) + min(N, CHUNK) + 1
        bound = count * 2.0 ** -24 * (abs(scale) * W + sv)
    bound = np.broadcast_to(bound, err.shape)
    worst = float((err / bound).max())
    print("gram_matvec %s %s: max error %.3e, largest error / bound %.3e" % (dtype, case, err.max(), worst))
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_the_product_is_a_function_of_its_column_and_its_row(dtype):
    """(257, 2 CHUNK + 5, S = 17, d = 5): two calls are bitwise equal; x in three ragged pieces carries the bits of the whole
    call; each of three rows of V computed alone (S = 1) carries the bits it has among the 17.  The same with one chunk
    (129 x 31, S = 65: two tiles of right-hand sides), with 17 chunks (two groups of launches) and for the symmetric form
    with a shift, row by row."""
    dt = TORCH[dtype]
    for case, cuts in ((CASES[10], (0, 100, 131, 257)), (CASES[4], (0, 1, 128, 129)), (CASES[13], (0, 3, 129, 130))):
        n, N, S, d, dl, sym, scale, shift = case
        x, x2, ell, V, _, _, _, _ = _case(case, dtype)
        xd, x2d, ed, Vd = dev(x, dt), dev(x2, dt), dev(ell, dt), dev(V, dt)
        whole = H.gram_matvec(xd, x2d, ed, Vd, scale=scale)
        again = H.gram_matvec(xd, x2d, ed, Vd, scale=scale)
        pieces = [H.gram_matvec(xd[a:b].contiguous(), x2d, ed, Vd, scale=scale) for a, b in zip(cuts[:-1], cuts[1:])]
        rows = [H.gram_matvec(xd, x2d, ed, Vd[s:s + 1].contiguous(), scale=scale) for s in (0, 7, S - 1)]
        buf = torch.full_like(whole, float("nan"))
        H.gram_matvec(xd, x2d, ed, Vd, scale=scale, out=buf)
        torch.cuda.synchronize()
        assert torch.equal(whole, again) and torch.equal(whole, buf)
        assert torch.equal(whole, torch.cat(pieces, dim=1))
        assert torch.equal(whole[[0, 7, S - 1]], torch.cat(rows, dim=0))
    for case in (CASES[5], CASES[11]):
        n, N, S, d, dl, sym, scale, shift = case
        x, _, ell, V, _, _, _, _ = _case(case, dtype)
        xd, ed, Vd = dev(x, dt), dev(ell, dt), dev(V, dt)
        whole = H.gram_matvec(xd, None, ed, Vd, scale=scale, shift=shift)
        rows = [H.gram_matvec(xd, None, ed, Vd[s:s + 1].contiguous(), scale=scale, shift=shift) for s in (0, S - 1)]
        torch.cuda.synchronize()
        assert torch.equal(whole[[0, S - 1]], torch.cat(rows, dim=0))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_no_rows_gives_zeros_and_no_columns_nothing(dtype):
    dt = TORCH[dtype]
    x, ell = dev(np.ones((5, 2)), dt), dev(np.ones(1), dt)
    out = torch.full((3, 5), float("nan"), dtype=dt, device="cuda")
    H.gram_matvec(x, torch.empty((0, 2), dtype=dt, device="cuda"), ell, torch.empty((3, 0), dtype=dt, device="cuda"), out=out)
    torch.cuda.synchronize()
    assert not out.any()
    none = H.gram_matvec(torch.empty((0, 2), dtype=dt, device="cuda"), x, ell, torch.ones((3, 5), dtype=dt, device="cuda"))
    assert tuple(none.shape) == (3, 0)


def test_bad_arguments_never_reach_a_launch():
    """Bad kind, a shift with x2 given, dl outside {1, d}, mismatched dtypes: each raises, and `out` keeps its NaNs."""
    dt = torch.float32
    x, x2, V = dev(np.ones((5, 3)), dt), dev(np.ones((4, 3)), dt), dev(np.ones((2, 4)), dt)
    ell = dev(np.ones(1), dt)
    out = torch.full((2, 5), float("nan"), dtype=dt, device="cuda")
    with pytest.raises(_lib.HipBackendError, match="UnitRBF"):
        H.gram_matvec(x, x2, ell, V, out=out, kind=H.KERN_SQDIST)
    with pytest.raises(_lib.HipBackendError, match="shift"):
        H.gram_matvec(x, x2, ell, V, shift=0.1, out=out)
    with pytest.raises(_lib.HipBackendError, match="lengthscales"):
        H.gram_matvec(x, x2, dev(np.ones(2), dt), V, out=out)
    with pytest.raises(TypeError, match="dtype"):
        H.gram_matvec(x, x2.double(), ell, V, out=out)
    with pytest.raises(TypeError, match="dtype"):
        H.gram_matvec(x, x2, ell, V.double(), out=out)
    with pytest.raises(ValueError):
        H.gram_matvec(x, x2, ell, dev(np.ones((2, 5)), dt), out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
