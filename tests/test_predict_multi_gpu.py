"""hb_sgp_predict_multi on the MI355X: the marginals of C full-rank latent functions that share x, z, ell and W from one
call.  The library's rule is that every entry that reports a mean or a variance stores the same bits, so the results are
compared with np.array_equal against C calls of hb_sgp_predict(HB_SGP_S_TRIL): the fused strip kernel (float32, Wfrag,
M % 32 == 0) at one tile (M = 32) and with off-diagonal tiles (M = 160), the chunked form (float32 M = 20, float64
M = 32), C below, at and across a PRED_PMAX group (1, 2, 5), d = 1 and 3, a ragged last strip (n = 1000) and a chunk
crossing (n = 32768 + 40), both residual modes.  One case of each form against the definition in numpy float64, and the
refusals."""
import numpy as np
import pytest
import torch

from henbun_amd import _lib
from henbun_amd import hip_ops as H

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
JITTER = 1e-3
CS = (1, 2, 5)
MODES = (H.SGP_DIAGONAL, H.SGP_NEGLECTED)
FORMS = {"fused32-M32": (F32, 32, True), "fused32-M160": (F32, 160, True), "chunked32-M20": (F32, 20, False),
         "chunked64-M32": (F64, 32, False)}
_CACHE = {}


def _case(form, d, n):
    """Operands of one case, built once and never written: x, z, ell, W (and Wfrag) from the library's own factorisation,
    m [5, M], S [5, M, M]; C < 5 takes the leading rows."""
    key = (form, d, n)
    if key in _CACHE:
        return _CACHE[key]
    dt, M, frag = FORMS[form]
    rs = np.random.RandomState(1000 * M + 10 * d + (n > 1000))
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda().contiguous()
    box = 0.6 * M ** (1.0 / d)
    z, ell = dev(rs.uniform(0, box, (M, d))), dev(rs.uniform(0.8, 1.3, d))
    x = dev(rs.uniform(-0.5, box + 0.5, (n, d)))
    K = H.gram_fwd(z, z, ell, diag_add=JITTER)
    wfrag = torch.empty(H.cholesky_frag_elems(1, M), dtype=dt, device="cuda") if frag else None
    _, W, info = H.cholesky_inverse(K, frag=wfrag)
    assert int(info.cpu()[0]) == 0
    m = dev(rs.randn(5, M))
    S = dev(np.tril(0.3 * rs.randn(5, M, M) / np.sqrt(M)) + np.eye(M) * rs.uniform(0.2, 0.9, (5, M, 1)))
    torch.cuda.synchronize()
    _CACHE[key] = (x, z, ell, W, wfrag, m, S)
    return _CACHE[key]


def _separate(x, z, ell, W, wfrag, m, S, mode):
    C = m.shape[0]
    mean, var = (torch.empty((C, x.shape[0]), dtype=x.dtype, device="cuda") for _ in range(2))
    for c in range(C):
        H.sgp_predict(x, z, ell, W, m[c:c + 1], S[c], s_kind=H.SGP_S_TRIL, mode=mode, jitter=0.0,
                      out=(mean[c:c + 1], var[c:c + 1]), wfrag=wfrag)
    return mean, var


@pytest.mark.parametrize("n", [1000, 32768 + 40])
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("form", list(FORMS))
def test_bits_of_the_per_latent_calls(form, d, n):
    x, z, ell, W, wfrag, m5, S5 = _case(form, d, n)
    dt, M, frag = FORMS[form]
    for C in CS:
        m, S = m5[:C].contiguous(), S5[:C].contiguous()
        assert H.sgp_predict_multi_fused(dt, n, M, d, C, wfrag is not None) is frag
        # the one-latent entry takes the same form, so the comparison is fused against fused, chunked against chunked
        assert H.sgp_predict_fused(dt, 1, n, M, d, 1, H.SGP_S_TRIL, wfrag is not None) is frag
        for mode in MODES:
            mean, var = H.sgp_predict_multi(x, z, ell, W, m, S, mode=mode, wfrag=wfrag)
            rm, rv = _separate(x, z, ell, W, wfrag, m, S, mode)
            mean, var, rm, rv = (t.cpu().numpy() for t in (mean, var, rm, rv))
            assert np.all(np.isfinite(mean)) and np.all(np.isfinite(var))
            assert np.array_equal(mean, rm), (C, mode, np.abs(mean - rm).max())
            assert np.array_equal(var, rv), (C, mode, np.abs(var - rv).max())
            again = H.sgp_predict_multi(x, z, ell, W, m, S, mode=mode, wfrag=wfrag)
            assert np.array_equal(again[0].cpu().numpy(), mean) and np.array_equal(again[1].cpu().numpy(), var)


def test_fused_answers_one_exactly_for_the_fused_shapes():
    for M in (32, 64, 160, 512):
        for d in (1, 2, 3, 4):
            for C in (1, 2, 4, 5, 64):
                assert H.sgp_predict_multi_fused(F32, 1000, M, d, C, True) is True
                assert _lib.lib().raw("hb_sgp_predict_multi_fused")(1000, M, d, C, 1, 4) == 1
                assert H.sgp_predict_multi_ws_elems(F32, 1000, M, d, C, True) == C * M * M
    for args in ((F32, 1000, 32, 1, 2, False), (F64, 1000, 32, 1, 2, True), (F32, 1000, 20, 1, 2, False),
                 (F32, 1000, 544, 1, 2, True), (F32, 1000, 32, 5, 2, True), (F32, 1000, 32, 1, 65, True),
                 (F32, 1000, 32, 1, 0, True)):
        assert H.sgp_predict_multi_fused(*args) is False
    # the chunked form needs the scratch of ONE one-latent call, whatever C
    assert H.sgp_predict_multi_ws_elems(F64, 5000, 32, 1, 7, False) == H.sgp_predict_ws_elems(F64, 1, 5000, 32, 1, 1, H.SGP_S_TRIL, False)


def _definition(x, z, ell, m, S, mode):
    """mean, var [C, n] from the definition in float64: L = chol(K(z, z) + jitter I), A = L^-1 K(z, x)."""
    k = lambda a, b: np.exp(-0.5 * (((a[:, None, :] - b[None, :, :]) / ell) ** 2).sum(-1))
    L = np.linalg.cholesky(k(z, z) + JITTER * np.eye(len(z)))
    A = np.linalg.solve(L, k(z, x))
    a2 = (A * A).sum(0)
    r = np.abs(1.0 - a2) if mode == H.SGP_DIAGONAL else 0.0 * a2
    return m @ A, np.stack([((np.tril(Sc).T @ A) ** 2).sum(0) + r for Sc in S])


@pytest.mark.parametrize("form, tol", [("fused32-M160", 5e-4), ("chunked64-M32", 1e-10)])
def test_against_the_definition(form, tol):
    """The bounds tests/test_predict_gpu.py holds hb_sgp_predict to: 5e-4 for the fused float32 form (the float32
    factorisation of K(z, z) + jitter I dominates), 1e-10 for float64.
    Observed on MI355X: fused float32 mean 4.6e-5, var 1.2e-5; float64 mean 4.1e-14, var 1.3e-14."""
    x, z, ell, W, wfrag, m, S = _case(form, 3, 1000)
    mean, var = H.sgp_predict_multi(x, z, ell, W, m, S, mode=H.SGP_DIAGONAL, wfrag=wfrag)
    f = lambda t: t.cpu().numpy().astype(np.float64)
    rm, rv = _definition(f(x), f(z), f(ell), f(m), f(S), H.SGP_DIAGONAL)
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    print("predict_multi %s: mean %.3g var %.3g" % (form, rel(f(mean), rm), rel(f(var), rv)))
    assert rel(f(mean), rm) <= tol and rel(f(var), rv) <= tol


def test_refusals_are_return_codes_before_any_launch():
    x, z, ell, W, wfrag, m5, S5 = _case("fused32-M32", 1, 1000)
    n, M, d = 1000, 32, 1
    sentinel = 7.5
    mean, var = (torch.full((5, n), sentinel, dtype=F32, device="cuda") for _ in range(2))
    ws = H.workspace(F32, x.device, 5 * M * M)
    p = H._p

    def call(C=2, kind=H.KERN_RBF, mode=H.SGP_DIAGONAL, mean_=mean, var_=var, ws_=ws, wf=wfrag, dl=1):
        _lib.lib().call("hb_sgp_predict_multi_f32", kind, p(x), p(z), p(ell), dl, p(W), p(wf), p(m5), p(S5), mode, p(mean_),
                        p(var_), n, M, d, C, p(ws_), H.stream())

    for kw, match in ((dict(C=0), "latent functions"), (dict(C=65), "latent functions"), (dict(kind=H.KERN_SQDIST), "UnitRBF"),
                      (dict(mode=H.SGP_FULLRANK), "residual mode"), (dict(mean_=None), "NULL"), (dict(var_=None), "NULL"),
                      (dict(ws_=None), "workspace"), (dict(dl=2), "lengthscales")):
        with pytest.raises(_lib.HipBackendError, match=match):
            call(**kw)
    # the wrapper refuses a short workspace by name, an S that does not match m and results of the wrong shape
    with pytest.raises(ValueError, match="sgp_predict_multi_ws_elems"):
        H.sgp_predict_multi(x, z, ell, W, m5, S5, wfrag=wfrag, ws=torch.empty(5 * M * M - 1, dtype=F32, device="cuda"))
    with pytest.raises(ValueError, match="S \\[C, M, M\\]"):
        H.sgp_predict_multi(x, z, ell, W, m5, S5[:4].contiguous(), wfrag=wfrag)
    with pytest.raises(ValueError, match="mean"):
        H.sgp_predict_multi(x, z, ell, W, m5, S5, wfrag=wfrag, out=(mean[:4], var))
    with pytest.raises(TypeError):
        H.sgp_predict_multi(x, z, ell, W, m5.double(), S5, wfrag=wfrag)
    torch.cuda.synchronize()
    assert float(mean.min().cpu()) == sentinel == float(var.max().cpu())      # nothing was launched
    call()                                                                     # and the accepted call does write
    torch.cuda.synchronize()
    assert float(mean[:2].max().cpu()) != sentinel and float(mean[2:].min().cpu()) == sentinel
