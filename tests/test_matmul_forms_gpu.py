"""Every form of hb_matmul_* against an exact integer reference, through the C ABI with explicit strides.

Operands are integers in [-4, 4] stored as fp32 / fp64, alpha in {1, -0.5, 2}, integer bias / C0 / Y: every product and
every partial sum is then exact in both precisions whatever the summation order, the slab count or the MFMA shape, so
each kernel must return the bits of the numpy float64 reference (np.array_equal; this file holds no tolerance).  Every
operand sits in a NaN-filled buffer with padding after each row and between batch items; C sits in a buffer prefilled
with a sentinel bit pattern at ldc = N + 3, sC = M ldc + 5: nothing outside the M x N blocks may change and no NaN may
reach the result.  Each case first asks hb_matmul_form which form / slab count / operand path it is about to run, so a
case written for one kernel cannot silently test another when a threshold moves."""
import contextlib
from ctypes import c_void_p

import numpy as np
import pytest
import torch

from henbun_amd import _lib
from henbun_amd import hip_ops as H

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
T64, T128, WGK, ROWS, RREG = 0, 1, 2, 3, 4
NN, NT, TN, TT = (False, False), (False, True), (True, False), (True, True)
ALL_T = (NN, NT, TN, TT)
WS_ELEMS = 1 << 22            # the workspace hip_ops.matmul passes
GUARD = 16                    # NaN elements in front of and behind every operand (16 keeps a 16-byte aligned base)
SENT = {F32: (np.uint32, 0x7FC5A5A5), F64: (np.uint64, 0x7FF8A5A5A5A5A5A5)}   # a NaN with a payload: never a result
LOWER, TRIL, PHI, SYM, SYMLOW, ACTGRAD = (H.MM_LOWER_OUT, H.MM_TRIL_OUT, H.MM_PHI_OUT, H.MM_SYM_OUT, H.MM_SYMLOW_OUT,
                                          H.MM_ACTGRAD)


def _np(dt):
    return np.float32 if dt == F32 else np.float64


@contextlib.contextmanager
def _switch(**kw):
    """mm_* diagnostic switches for the body, cleared again whatever happens."""
    try:
        for k, v in kw.items():
            H.debug_set(k, v)
        yield
    finally:
        H.debug_clear()


class _Strided:
    """A [nb, rows, cols] integer array inside a NaN buffer: row stride cols + pad, batch stride rows * ld + 8 (0 when
    nb == 1 stands for a shared operand), `off` elements past a 16-byte aligned base."""

    def __init__(self, rng, dt, nb, rows, cols, pad, off=0):
        self.ld = cols + pad
        self.stride = rows * self.ld + 8
        n = GUARD + off + (nb - 1) * self.stride + rows * self.ld + GUARD
        host = np.full(n, np.nan, dtype=_np(dt))
        it = host.itemsize
        view = np.lib.stride_tricks.as_strided(host[GUARD + off:], (nb, rows, cols), (self.stride * it, self.ld * it, it))
        self.val = rng.integers(-4, 5, (nb, rows, cols)).astype(np.float64)
        view[...] = self.val
        self.dev = torch.from_numpy(host).cuda()
        self.ptr = self.dev.data_ptr() + (GUARD + off) * it
        assert (self.dev.data_ptr() + GUARD * it) % 16 == 0

    @property
    def aligned(self):
        return self.ptr % 16 == 0


_ws = {}


def _workspace(dt):
    """One NaN-filled workspace per dtype: a slab that is read before it is written shows up in the result."""
    if dt not in _ws:
        _ws[dt] = torch.empty(WS_ELEMS, dtype=dt, device="cuda")
    _ws[dt].fill_(float("nan"))
    return _ws[dt]


def _reference(A, B, ta, tb, alpha, beta, bias, act, flags, C0, Y, K):
    """The product and its epilogue in float64.  Exact: |sum| <= 16 K <= 16 * 4224 < 2^24, and the epilogue (alpha, bias,
    beta C0, the halvings of Phi / Sym) keeps every value a multiple of 1/4 below 2^24 / 4."""
    assert 16 * K <= 16 * 4224 < 2 ** 24 and 4 * (2 * 16 * K + 4 + 2 * 4) < 2 ** 24
    opA = np.swapaxes(A, -1, -2) if ta else A
    opB = np.swapaxes(B, -1, -2) if tb else B
    R = alpha * np.matmul(opA, opB)
    if flags & ACTGRAD:
        return R * (Y > 0)
    if flags & SYM:
        return 0.5 * (R + np.swapaxes(R, -1, -2))
    if flags & SYMLOW:
        low = np.tril(R)
        return 0.5 * (low + np.swapaxes(np.tril(R, -1), -1, -2))
    if bias is not None:
        R = R + bias[:, None, :]
    if act == "relu":
        R = np.maximum(R, 0.0)
    if beta != 0.0:
        R = R + beta * C0
    if flags & (TRIL | PHI):
        R = np.tril(R)
    if flags & PHI:
        i = np.arange(min(R.shape[-2:]))
        R[..., i, i] *= 0.5
    return R


def _check_c(dt, dev, host0, batch, M, N, ldc, sC, ref, untouched=None):
    """Everything outside the M x N blocks still holds what it held; the blocks are NaN-free and equal `ref` bit for bit
    (where `untouched` is set, the block must instead still hold its initial content)."""
    itype, _ = SENT[dt]
    got = dev.cpu().numpy()
    blocks = lambda a: np.lib.stride_tricks.as_strided(a[7:], (batch, M, N), (sC * a.itemsize, ldc * a.itemsize, a.itemsize))
    outside = np.ones(got.shape, dtype=bool)
    blocks(outside)[...] = False
    assert np.array_equal(got.view(itype)[outside], host0.view(itype)[outside]), "a store outside the M x N blocks of C"
    res = blocks(got)
    want = ref.astype(_np(dt))
    assert np.array_equal(want.astype(np.float64), ref), "reference not representable"
    if untouched is not None:
        assert np.array_equal(blocks(got.view(itype))[untouched], blocks(host0.view(itype))[untouched]), \
            "a tile the flag leaves alone was written"
        assert not np.isnan(res[~untouched]).any()
        assert np.array_equal(res[~untouched], want[~untouched])
    else:
        assert not np.isnan(res).any(), "NaN in the result: padding or an unwritten slab was read"
        assert np.array_equal(res, want)
    return res


def run(dt, batch, M, N, K, trans=NN, expect=None, alpha=1.0, beta=0.0, bias=None, act="none", flags=0, pad_a=4, pad_b=4,
        off_a=0, off_b=0, share_a=False, share_b=False, seed=0):
    """One hb_matmul call.  expect: (form, S, vec, finish, bfast) the case was written for, asserted through
    hb_matmul_form before the launch.  bias: None, 'shared' ([N]) or 'batch' ([batch, N])."""
    ta, tb = trans
    rng = np.random.default_rng(seed + 1000 * M + 10 * N + K)
    A = _Strided(rng, dt, 1 if share_a else batch, K if ta else M, M if ta else K, pad_a, off_a)
    B = _Strided(rng, dt, 1 if share_b else batch, N if tb else K, K if tb else N, pad_b, off_b)
    sA = 0 if (share_a or batch == 1) else A.stride
    sB = 0 if (share_b or batch == 1) else B.stride
    ldc, sC = N + 3, M * (N + 3) + 5
    itype, sent = SENT[dt]
    host0 = np.full(7 + batch * sC + 7, sent, dtype=itype).view(_np(dt))
    it = host0.itemsize
    C0 = None
    if beta != 0.0:
        C0 = rng.integers(-4, 5, (batch, M, N)).astype(np.float64)
        np.lib.stride_tricks.as_strided(host0[7:], (batch, M, N), (sC * it, ldc * it, it))[...] = C0
    Cdev = torch.from_numpy(host0.copy()).cuda()
    biasv = Yv = bdev = None
    sBias = 0
    if flags & ACTGRAD:
        Yv = rng.integers(-4, 5, (batch, M, N)).astype(np.float64)
        bdev = torch.from_numpy(Yv.astype(_np(dt))).cuda()
        sBias = M * N if batch > 1 else 0
    elif bias is not None:
        nbias = batch if bias == "batch" else 1
        biasv = rng.integers(-4, 5, (nbias, N)).astype(np.float64)
        bdev = torch.from_numpy(biasv.astype(_np(dt))).cuda()
        sBias = N if bias == "batch" else 0
    ws = _workspace(dt)
    f = H.matmul_form(dt, batch, M, N, K, lda=A.ld, ldb=B.ld, ldc=ldc, sA=sA, sB=sB, transA=ta, transB=tb, beta=beta,
                      flags=flags, a_aligned=A.aligned, b_aligned=B.aligned, ws_elems=ws.numel())
    if expect is not None:
        assert (f.form, f.S, int(f.vec), int(f.finish), int(f.bfast)) == tuple(expect), (f, expect)
    sfx = "_f32" if dt == F32 else "_f64"
    _lib.lib().call("hb_matmul" + sfx, c_void_p(A.ptr), c_void_p(B.ptr), c_void_p(Cdev.data_ptr() + 7 * it), batch, M, N, K,
                    A.ld, B.ld, ldc, sA, sB, sC, int(ta), int(tb), float(alpha), float(beta),
                    c_void_p(bdev.data_ptr()) if bdev is not None else None, sBias, H.ACT[act], int(flags),
                    c_void_p(ws.data_ptr()), ws.numel(), H.stream())
    torch.cuda.synchronize()
    ref = _reference(A.val, B.val, ta, tb, alpha, beta, biasv, act, flags, C0, Yv, K)
    untouched = None
    if flags & LOWER:
        # LOWER_OUT promises the tiles that touch the lower triangle and leaves the others alone; the tile edge is the form's
        t = {T64: 64, T128: 128, WGK: 32}[f.form]
        r, c = np.arange(M)[:, None] // t, np.arange(N)[None, :] // t
        untouched = np.broadcast_to(c > r, (batch, M, N))
    return _check_c(dt, Cdev, host0, batch, M, N, ldc, sC, ref, untouched), f


# the epilogues a form takes, as keyword sets of run(): every one is exact under integer operands
EPI_PLAIN = [dict(), dict(alpha=-0.5), dict(alpha=2.0, bias="shared", act="relu"), dict(bias="batch", beta=2.0),
             dict(alpha=-0.5, bias="shared", act="relu", beta=2.0)]
EPI_TRI = [dict(flags=LOWER), dict(flags=LOWER, alpha=2.0, bias="shared", beta=2.0), dict(flags=TRIL, alpha=-0.5),
           dict(flags=PHI, alpha=-0.5), dict(flags=PHI, bias="shared", act="relu", beta=2.0)]
EPI_SQUARE = [dict(flags=SYM, alpha=-0.5), dict(flags=SYMLOW, alpha=-0.5), dict(flags=SYM), dict(flags=SYMLOW, alpha=2.0)]
EPI_ACTGRAD = [dict(flags=ACTGRAD, act="relu", alpha=-0.5), dict(flags=ACTGRAD, act="relu")]


def _cycle(seq, i):
    return seq[i % len(seq)]


def _every_epilogue_and_transpose(Ks):
    """(K, trans, epilogue, seed) for the tile engine's two operand paths: each of the twelve epilogues (EPI_PLAIN,
    EPI_TRI, EPI_ACTGRAD) meets each of the four transposes, at K = Ks[(e + t) % 4] for epilogue e and transpose t --
    so each epilogue also meets each of the four K, and each (K, transpose) pair three epilogues (e = K's index - t
    mod 4).  48 products of milliseconds each."""
    assert len(Ks) == len(ALL_T) == 4
    epis = EPI_PLAIN + EPI_TRI + EPI_ACTGRAD
    return [(Ks[(e + t) % 4], trans, epi, 4 * e + t) for e, epi in enumerate(epis) for t, trans in enumerate(ALL_T)]


# ---------------------------------------------------------------- tile engine, vector path
@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("mn", [(64, 64), (68, 132), (4, 4), (200, 96)], ids=str)
def test_tile_engine_vector_path(dt, mn):
    """One, two, three and five k-steps (the two-steps-per-iteration loop of run_vec and its odd tail), one tile, ragged
    multi-tile shapes whose edge groups clamp to M - VEC / N - VEC, and the smallest shape, where the clamp lands on
    index 0 (fp64: 2 x 2).  K < 128: no split, and neither the rows nor the in-workgroup form takes these shapes."""
    M, N = (2, 2) if (dt == F64 and mn == (4, 4)) else mn
    for K, trans, epi, seed in _every_epilogue_and_transpose((16, 32, 48, 80)):
        run(dt, 1, M, N, K, trans, expect=(T64, 1, 1, 0, 0), seed=seed, **epi)


# ---------------------------------------------------------------- tile engine, scalar path
@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("mn", [(65, 130), (5, 7)], ids=str)
def test_tile_engine_scalar_path(dt, mn):
    M, N = mn
    for K, trans, epi, seed in _every_epilogue_and_transpose((1, 15, 17, 33)):
        run(dt, 1, M, N, K, trans, expect=(T64, 1, 0, 0, 0), seed=seed, **epi)


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("trans", ALL_T, ids=["nn", "nt", "tn", "tt"])
def test_misaligned_base_or_odd_leading_dimension_takes_the_scalar_path(dt, trans):
    """A vector-eligible shape: a base pointer one element off, or a leading dimension padded by 1, must push it onto the
    scalar path; a padding of 4 keeps the vector path.  All must stay exact."""
    for kw, vec in ((dict(off_a=1), 0), (dict(off_b=1), 0), (dict(pad_a=1), 0), (dict(pad_b=1), 0), (dict(), 1),
                    (dict(pad_a=8, pad_b=12), 1)):
        run(dt, 1, 64, 64, 32, trans, expect=(T64, 1, vec, 0, 0), alpha=-0.5, bias="shared", **kw)
        run(dt, 1, 68, 132, 48, trans, expect=(T64, 1, vec, 0, 0), **kw)


# ---------------------------------------------------------------- 128-tile engine
@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("shape", [(132, 260, 48), (128, 128, 16)], ids=str)
def test_tile128_engine_forced_to_small_shapes(dt, shape):
    M, N, K = shape
    with _switch(mm_force_bt=128):
        for i, trans in enumerate(ALL_T):
            for j, epi in enumerate(EPI_PLAIN[1:3] + EPI_TRI[:1] + EPI_TRI[3:4] + EPI_ACTGRAD[:1]):
                run(dt, 1, M, N, K, trans, expect=(T128, 1, 1, 0, 0), seed=5 * i + j, **epi)
    if K >= 48:   # split-K on 128-tiles, with the finish launch
        with _switch(mm_force_bt=128, mm_force_s=3):
            run(dt, 1, M, N, K, NN, expect=(T128, 3, 1, 1, 0), alpha=-0.5, bias="shared", beta=2.0)
            run(dt, 1, M, N, K, TT, expect=(T128, 3, 1, 1, 0), flags=LOWER)


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("batch, bfast", [(50, 0), (56, 1)])
def test_tile128_engine_at_its_natural_threshold(dt, batch, bfast):
    """256^3 over a batch of 50: 200 active 128-tiles; 56 also takes the batch-fastest grid.  No switch set."""
    run(dt, batch, 256, 256, 256, NN, expect=(T128, 1, 1, 0, bfast), alpha=-0.5, bias="batch", act="relu")
    run(dt, batch, 256, 256, 256, TT, expect=(T128, 1, 1, 0, bfast), alpha=2.0, bias="shared", beta=2.0)


def test_tile128_engine_lower_tiles_at_its_natural_threshold():
    """With a triangular epilogue a 256 x 256 result has three active 128-tiles: 67 matrices make 201."""
    run(F32, 67, 256, 256, 256, NT, expect=(T128, 1, 1, 0, 0), flags=PHI, alpha=-0.5)
    run(F32, 67, 256, 256, 256, TN, expect=(T128, 1, 1, 0, 0), flags=LOWER)
    run(F32, 66, 256, 256, 256, NN, expect=(T64, 1, 1, 0, 0), flags=TRIL)     # 198: 64-tiles


# ---------------------------------------------------------------- batch: grid.y against the batch-fastest grid
@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("batch, bfast", [(3, 0), (8, 1), (16, 1)])
def test_batch_grids_and_broadcast_operands(dt, batch, bfast):
    for i, trans in enumerate(ALL_T):
        e = (T64, 1, 1, 0, bfast)
        run(dt, batch, 68, 60, 48, trans, expect=e, share_a=True, seed=i)
        run(dt, batch, 68, 60, 48, trans, expect=e, share_b=True, alpha=-0.5, seed=i)
        run(dt, batch, 68, 60, 48, trans, expect=e, bias="batch", act="relu", seed=i)
        run(dt, batch, 68, 60, 48, trans, expect=e, bias="shared", beta=2.0, alpha=2.0, seed=i)
    run(dt, batch, 68, 60, 48, NN, expect=(T64, 1, 1, 0, bfast), flags=ACTGRAD, act="relu")
    run(dt, batch, 68, 68, 48, NT, expect=(T64, 1, 1, 0, bfast), flags=TRIL)
    run(dt, batch, 68, 60, 17, NN, expect=(T64, 1, 0, 0, bfast), bias="batch")      # the same grids on the scalar path


# ---------------------------------------------------------------- split-K slabs and the finish launch
def _vec_ok(dt, M, N, trans):
    v = 4 if dt == F32 else 2
    return int((not trans[0] or M % v == 0) and (trans[1] or N % v == 0))


SPLIT = [  # (M, N, K), transposes, switches, S, vector path by (dtype, transposes)
    ((64, 64, 144), ALL_T, {}, 2, lambda dt, t: 1),
    ((64, 64, 704), ALL_T, {}, 8, lambda dt, t: 1),                 # 11 slabs, rounded down to 8
    ((64, 64, 4112), (TN, TT), {}, 64, lambda dt, t: 1),            # slabs of 80: the last twelve are empty
    ((7, 5, 4100), ALL_T, {}, 64, lambda dt, t: 0),
    ((130, 130, 80), ALL_T, {"mm_force_s": 3}, 3, lambda dt, t: _vec_ok(dt, 130, 130, t)),   # slabs 32 / 32 / 16
]


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", SPLIT, ids=[str(c[0]) for c in SPLIT])
def test_split_k_and_finish_every_epilogue(dt, case):
    """fp32 stays on the tile engine here because K % 128 != 0 or K > 4096."""
    (M, N, K), transes, sw, S, vec = case
    epis = EPI_PLAIN + EPI_TRI + EPI_ACTGRAD + (EPI_SQUARE if M == N else [])
    with _switch(**sw):
        for i, epi in enumerate(epis):
            trans = _cycle(transes, i)
            run(dt, 1, M, N, K, trans, expect=(T64, S, vec(dt, trans), 1, 0), seed=i, **epi)
        for i, trans in enumerate(transes):     # and every transpose at least once
            run(dt, 1, M, N, K, trans, expect=(T64, S, vec(dt, trans), 1, 0), seed=50 + i, **_cycle(EPI_PLAIN[2:], i))


def test_split_k_vector_path_forms_stated_as_literals():
    """The vector path of the (130, 130, 80) case, spelled out instead of computed: N = 130 is no multiple of four floats,
    so fp32 is vector-eligible only when both operands are k-contiguous; fp64 (two per group) always is."""
    assert [_vec_ok(F32, 130, 130, t) for t in ALL_T] == [0, 1, 0, 0]
    assert [_vec_ok(F64, 130, 130, t) for t in ALL_T] == [1, 1, 1, 1]


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("batch", [3, 8])
def test_split_k_over_a_batch(dt, batch):
    """Slabs x batch in both grid orders: (48, 64, 256) has one tile per matrix, so the launcher splits it four ways."""
    e = (T64, 4, 1, 1, 1 if batch == 8 else 0)
    run(dt, batch, 48, 64, 256, NN, expect=e, bias="batch", act="relu", alpha=-0.5, beta=2.0)
    run(dt, batch, 48, 64, 256, TT, expect=e, flags=ACTGRAD, act="relu")
    run(dt, batch, 48, 48, 256, TN, expect=e, flags=SYM, share_b=True)


def run_colsum(dt, M, N, K, expect, pad_a=4, off_a=0, seed=0):
    """hb_matmul_colsum: C = A^T B and the column sums of B (contiguous: ldb = N), both exact."""
    rng = np.random.default_rng(seed + 1000 * M + 10 * N + K)
    A = _Strided(rng, dt, 1, K, M, pad_a, off_a)
    B = _Strided(rng, dt, 1, K, N, 0)
    ldc, sC = N + 3, M * (N + 3) + 5
    itype, sent = SENT[dt]
    host0 = np.full(7 + sC + 7, sent, dtype=itype).view(_np(dt))
    it = host0.itemsize
    Cdev = torch.from_numpy(host0.copy()).cuda()
    cs0 = np.full(5 + N + 5, sent, dtype=itype).view(_np(dt))
    csdev = torch.from_numpy(cs0.copy()).cuda()
    ws = _workspace(dt)
    f = H.matmul_form(dt, 1, M, N, K, lda=A.ld, ldb=N, ldc=ldc, transA=True, a_aligned=A.aligned, b_aligned=B.aligned,
                      ws_elems=ws.numel(), colsum=True)
    assert (f.form, f.S, int(f.vec), int(f.finish), int(f.colsum_fused)) == tuple(expect), (f, expect)
    _lib.lib().call("hb_matmul_colsum" + ("_f32" if dt == F32 else "_f64"), c_void_p(A.ptr), c_void_p(B.ptr),
                    c_void_p(Cdev.data_ptr() + 7 * it), c_void_p(csdev.data_ptr() + 5 * it), M, N, K, A.ld, N, ldc,
                    c_void_p(ws.data_ptr()), ws.numel(), H.stream())
    torch.cuda.synchronize()
    assert 4 * K < 2 ** 24
    _check_c(dt, Cdev, host0, 1, M, N, ldc, sC, np.matmul(np.swapaxes(A.val, -1, -2), B.val))
    got = csdev.cpu().numpy()
    assert np.array_equal(got.view(itype)[:5], cs0.view(itype)[:5]) and np.array_equal(got.view(itype)[5 + N:], cs0.view(itype)[5 + N:])
    assert np.array_equal(got[5:5 + N], B.val[0].sum(axis=0).astype(_np(dt)))


@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_colsum_fused_and_fallback(dt):
    """(form, S, vec, finish, fused).  Fused: one slab, two slabs, eight, and 64 of which twelve are empty, plus a ragged
    multi-tile result; fallback (a reduction launch of its own): K % 16 != 0, N % 4 != 0, a misaligned A."""
    run_colsum(dt, 64, 64, 48, (T64, 1, 1, 0, 1))
    run_colsum(dt, 64, 64, 144, (T64, 2, 1, 1, 1))
    run_colsum(dt, 64, 64, 704, (T64, 8, 1, 1, 1))
    run_colsum(dt, 64, 64, 4112, (T64, 64, 1, 1, 1))
    run_colsum(dt, 68, 132, 80, (T64, 1, 1, 0, 1))
    run_colsum(dt, 68, 132, 272, (T64, 4, 1, 1, 1))
    run_colsum(dt, 7, 5, 4100, (T64, 64, 0, 1, 0))
    run_colsum(dt, 64, 64, 100, (T64, 1, 0, 0, 0))
    run_colsum(dt, 64, 64, 144, (T64, 2, 0, 1, 0), off_a=1)
    run_colsum(dt, 64, 64, 144, (T64, 2, 0, 1, 0), pad_a=1)


# ---------------------------------------------------------------- in-workgroup split-K (fp32)
WGK_SHAPES = [(1, 32, 32, 128), (3, 64, 96, 128), (1, 64, 64, 4096), (8, 128, 128, 384)]


@pytest.mark.parametrize("shape", WGK_SHAPES, ids=str)
def test_wgk_every_epilogue_and_transpose(shape):
    """No switch set: these shapes reach matmul_wgk_kernel by the launcher's own rule."""
    batch, M, N, K = shape
    e = (WGK, 1, 0, 0, 0)
    epis = EPI_PLAIN + EPI_TRI + (EPI_SQUARE if M == N else [])
    for i, epi in enumerate(epis):
        for j, trans in enumerate(ALL_T if K <= 384 else (_cycle(ALL_T, i),)):
            res, _ = run(F32, batch, M, N, K, trans, expect=e, seed=4 * i + j, pad_a=4 * (1 + j % 2), pad_b=4 * (1 + i % 3), **epi)
            if epi.get("flags", 0) & (SYM | SYMLOW):
                assert np.array_equal(res, np.swapaxes(res, -1, -2)), "SYM_OUT / SYMLOW_OUT must be exactly symmetric"
    run(F32, batch, M, N, K, NN, expect=e, share_a=True)
    run(F32, batch, M, N, K, TT, expect=e, share_b=True, bias="batch")


def test_shapes_and_operands_that_must_leave_the_wgk_form():
    run(F32, 1, 64, 64, 4224, NN, expect=(T64, 64, 1, 1, 0), alpha=-0.5)          # K > 4096
    run(F32, 1, 48, 64, 128, NN, expect=(T64, 2, 1, 1, 0), bias="shared")         # M % 32
    run(F32, 1, 64, 64, 128, NN, expect=(T64, 2, 1, 1, 0), flags=ACTGRAD, act="relu")
    run(F32, 1, 64, 64, 128, NT, expect=(T64, 2, 0, 1, 0), pad_a=1)
    run(F32, 1, 64, 64, 128, TN, expect=(T64, 2, 0, 1, 0), off_b=1)
    run(F64, 1, 64, 64, 128, NN, expect=(T64, 2, 1, 1, 0))
    with _switch(mm_no_wgk=1):
        run(F32, 8, 128, 128, 384, NN, expect=(T64, 6, 1, 1, 1), flags=SYM)    # slabs x batch-fastest grid x finish
        run(F32, 1, 64, 64, 128, TT, expect=(T64, 2, 1, 1, 0), flags=SYMLOW)


# ---------------------------------------------------------------- the two row forms (fp32)
ROW_M = (2048, 2049, 2079)
ROW_EPI = [dict(alpha=-0.5), dict(bias="shared", act="relu", alpha=2.0), dict(flags=ACTGRAD, act="relu", alpha=-0.5),
           dict(bias="shared")]


def _rows_cases(form, K, N, sw):
    with _switch(**sw):
        for M in ROW_M:
            for tb in (False, True):
                for i, epi in enumerate(ROW_EPI):
                    run(F32, 1, M, N, K, (False, tb), expect=(form, 1, 0, 0, 0), seed=i, pad_a=4 if i % 2 == 0 else 8,
                        pad_b=4 if tb else (1 if i % 2 else 4), **epi)


@pytest.mark.parametrize("kn", [(8, 7), (24, 100), (40, 128), (64, 16), (64, 256), (136, 128), (256, 32)], ids=str)
def test_row_streaming_form(kn):
    """matmul_rows_kernel.  (64, 256) is a shape the register form takes first: mm_no_rowsreg brings it here, where it
    is the widest staging the LDS limit admits at eight waves; every other shape arrives by the launcher's own rule."""
    K, N = kn
    _rows_cases(ROWS, K, N, {"mm_no_rowsreg": 1} if kn == (64, 256) else {})


@pytest.mark.parametrize("kn", [(16, 64), (32, 33), (64, 250), (128, 96)], ids=str)
def test_row_register_form(kn):
    K, N = kn
    _rows_cases(RREG, K, N, {})


def test_row_forms_leave_for_the_tile_engine():
    """A leading dimension padded by 1 (or a misaligned A) sends a rows shape to the tile engine, scalar path; M = 2047
    is below the threshold; mm_no_rows switches the forms off."""
    run(F32, 1, 2048, 100, 24, NN, expect=(T64, 1, 0, 0, 0), pad_a=1, bias="shared", act="relu")
    run(F32, 1, 2049, 64, 64, NT, expect=(T64, 1, 0, 0, 0), pad_a=1, flags=ACTGRAD, act="relu")
    run(F32, 1, 2048, 64, 64, NN, expect=(T64, 1, 0, 0, 0), off_a=1)
    run(F32, 1, 2048, 64, 64, NT, expect=(T64, 1, 0, 0, 0), pad_b=1)
    run(F32, 1, 2047, 64, 64, NN, expect=(T64, 1, 1, 0, 0), bias="shared")
    run(F32, 1, 2048, 64, 64, NN, expect=(T64, 1, 1, 0, 0), beta=2.0)
    with _switch(mm_no_rows=1):
        run(F32, 1, 2079, 250, 64, NN, expect=(T64, 1, 0, 0, 0), bias="shared", act="relu")


# ---------------------------------------------------------------- hip_ops.matmul_ld
@pytest.mark.parametrize("m, form", [(300, T64), (2100, RREG)])
@pytest.mark.parametrize("transB", [False, True], ids=["n", "t"])
def test_matmul_ld_reads_the_leading_rows_of_a_wider_buffer(m, form, transB):
    """As sgp_select uses it: A is the leading k = 64 columns of a history buffer of row stride 512, on both sides of the
    rows threshold.  The rest of the buffer is NaN."""
    k, n, lda = 64, 48, 512
    rng = np.random.default_rng(m)
    hist = np.full((m, lda), np.nan, dtype=np.float32)
    a = rng.integers(-4, 5, (m, k)).astype(np.float64)
    hist[:, :k] = a
    b = rng.integers(-4, 5, (n, k) if transB else (k, n)).astype(np.float64)
    f = H.matmul_form(F32, 1, m, n, k, lda=lda, ldb=k if transB else n, transB=transB)
    assert (f.form, f.S, f.vec) == (form, 1, form == T64)
    out = torch.full((m, n), float("nan"), dtype=F32, device="cuda")
    H.matmul_ld(torch.from_numpy(hist).cuda(), lda, torch.from_numpy(b.astype(np.float32)).cuda(), k if transB else n, out, m, n, k,
                transB=transB, alpha=-0.5)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().astype(np.float64), -0.5 * (a @ (b.T if transB else b)))
