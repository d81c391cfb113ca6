"""The operand / output / workspace contract of the `hip_ops` wrappers (hip_ops._operands, _out, _ws), one table row per
wrapper whose `ws` and / or caller-supplied results go through those helpers (the wrappers that keep their own result
handling, and why, are named in the docstring of hip_ops._out; they have no row here).  The C entries take every buffer
as a bare pointer, so the wrapper's check is the only one a buffer gets.  For each row:

  1. a workspace of EXACTLY the queried size (a view big[:need]) and explicit results return the bits of the default call;
  2. a workspace one element short raises ValueError naming the wrapper and its *_ws_elems query -- the short view lies
     inside a buffer of `need` elements, and sentinel-filled results are untouched afterwards (nothing was launched);
  3. a workspace of the other dtype raises ValueError;
  4. a result with one extent off by one, and a result of the other dtype, each raise ValueError (the rows marked
     exact=False take any shape of the right element count: the plan hands them results in its own nodes' shapes);
  5. one operand of the other dtype raises TypeError;
  6. a non-contiguous operand (a transposed view) raises ValueError.

The scratch images that are not `ws` (`frag`, `abar_frag`, `bws`) have a test of their own at the end.
Every refused buffer is at least as large in bytes as the right one.  Shapes: n = 33, M = 32, d = 2, P = 1, N = 40,
S = 2, L = 4, C = 2 (the fused encoder takes n = 32, Din = 32, H = 128; the Gram-fed factorisation M = 64)."""
import numpy as np
import pytest
import torch

from henbun_amd import hip_ops as H

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
n, M, d, N, S, L, C = 33, 32, 2, 40, 2, 4, 2
SENTINEL = 7.0


def _other(dt):
    return F64 if dt == F32 else F32


class Ops(dict):
    __getattr__, __setattr__ = dict.__getitem__, dict.__setitem__


_OPS = {}


def operands(dt):
    """The operands every row draws from, built once per dtype and never written."""
    if dt in _OPS:
        return _OPS[dt]
    rs = np.random.RandomState(11)
    dev = lambda a, t=dt: torch.as_tensor(np.ascontiguousarray(a), dtype=t).cuda().contiguous()
    o = Ops()
    o.x, o.z, o.X = dev(rs.uniform(0, 3, (n, d))), dev(rs.uniform(0, 3, (M, d))), dev(rs.uniform(0, 3, (N, d)))
    o.ell = dev([0.9, 1.3])
    o.W = dev(0.1 * np.tril(rs.randn(M, M)))
    o.m, o.s = dev(rs.randn(M)), dev(0.1 + rs.rand(M))
    o.m1, o.s1 = o.m.reshape(1, M), o.s.reshape(1, M)
    o.Y, o.w, o.r = dev(rs.randn(N, 1)), dev(rs.rand(N)), dev(rs.randn(N))
    o.w2, o.r2 = dev(rs.rand(C, N)), dev(rs.randn(C, N))
    o.omega, o.coef, o.inc = dev(rs.randn(L, d)), dev(rs.randn(S, 2 * L + M)), dev(rs.randn(S))
    o.V, o.A, o.B, o.wv = dev(rs.randn(S, N)), dev(rs.randn(S, N)), dev(rs.randn(S, N)), dev(rs.rand(S), F64)
    o.z64, o.ell64 = dev(o.z.cpu().numpy(), F64), dev([0.9, 1.3], F64)
    o.Q, o.R = dev(rs.randn(M, M), F64), dev(rs.randn(M, 1), F64)
    o.w64, o.r64 = dev(rs.rand(N), F64), dev(rs.randn(N), F64)
    a = rs.randn(M, M)
    o.spd = dev(a @ a.T + M * np.eye(M))
    o.pts = dev(rs.uniform(0, 3, (64, d)))
    o.labels, o.mean, o.var = dev(rs.randint(0, C, N)), dev(rs.randn(C, N)), dev(0.1 + rs.rand(C, N))
    o.nodes = dev(rs.randn(S, C), F64)
    o.var1, o.idx = dev([0.7]), dev(rs.randint(0, N, 5), torch.int64)
    o.fmu, o.fS, o.fu = dev(rs.randn(S, 8)), dev(np.tril(rs.randn(S, 8, 8))), dev(rs.randn(S, 8))
    o.fxbar, o.fklbar = dev(rs.randn(S, 8)), dev([1.0])
    o.fx = H.fullrank_sample_kl_fwd(o.fmu, o.fS, u_in=o.fu)[0]
    o.tv, o.tt = dev(rs.randn(S, 10)), dev(rs.randn(4, 4))
    if dt == F32:   # the fused encoder and what its backward reads
        o.y, o.w0, o.b0 = dev(rs.randn(32, 32)), dev(0.2 * rs.randn(32, 128)), dev(0.1 * rs.randn(128))
        o.w1, o.b1, o.u = dev(0.2 * rs.randn(128, 32)), dev(0.1 * rs.randn(32)), dev(rs.randn(32, 16))
        o.xbar, o.klbar = dev(rs.randn(32, 16)), dev([1.0])
        o.ex, _, o.eu, o.eo = H.mlp2_sample_fwd(o.y, o.w0, o.b0, o.w1, o.b1, "tanh", u_in=o.u)
    torch.cuda.synchronize()
    _OPS[dt] = o
    return o


DIAG = H.SGP_S_DIAG


class Row:
    """who; call(o, **buffers) -> results; ws = (dtype or None for the operands', need(dt), query); outs = {keyword: shape,
    (shape, dtype) or a tuple of them}; mixed / strided: the operand handed over in the other dtype / as a transposed view."""

    def __init__(self, who, call, ws=None, outs=None, mixed=None, strided=None, dtypes=(F32, F64)):
        self.who, self.call, self.ws, self.outs, self.mixed, self.strided, self.dtypes = who, call, ws, outs or {}, mixed, strided, dtypes


ROWS = [
    Row("sgp_predict", lambda o, **k: H.sgp_predict(o.x, o.z, o.ell, o.W, o.m1, o.s1, **k),
        ws=(None, lambda dt: H.sgp_predict_ws_elems(dt, 1, n, M, d, 1, DIAG, False), "sgp_predict_ws_elems"),
        outs={"out": ((1, n), (1, n))}, mixed="z", strided="x"),
    Row("sgp_predict_grad", lambda o, **k: H.sgp_predict_grad(o.x, o.z, o.ell, o.W, o.m, o.s, **k),
        ws=(None, lambda dt: H.sgp_predict_grad_ws_elems(dt, n, M, d, DIAG, False), "sgp_predict_grad_ws_elems"),
        outs={"out": ((n,), (n,), (n, d), (n, d))}, mixed="W", strided="z"),
    Row("sgp_acq", lambda o, **k: H.sgp_acq(o.x, o.z, o.ell, o.W, o.m, o.s, "ei", best=0.1, grad=True, argmax=True, **k),
        ws=(None, lambda dt: H.sgp_acq_ws_elems(dt, n, M, d, DIAG, False), "sgp_acq_ws_elems"), mixed="m", strided="x"),
    Row("sgp_predict_cov", lambda o, **k: H.sgp_predict_cov(o.x, o.z, o.ell, o.W, o.s1, 1, **k),
        ws=(None, lambda dt: H.sgp_predict_cov_ws_elems(dt, 1, n, M, 1, DIAG), "sgp_predict_cov_ws_elems"),
        outs={"out": (1, n, n)}, mixed="W", strided="x"),
    Row("sgp_stats", lambda o, **k: H.sgp_stats(o.X, o.Y, o.z, o.ell, o.W, **k),
        ws=(None, lambda dt: H.sgp_stats_ws_elems(dt, N, M, d, 1), "sgp_stats_ws_elems"), mixed="Y", strided="X"),
    Row("sgp_wstats", lambda o, **k: H.sgp_wstats(o.X, o.w, o.r, o.z, o.ell, o.W, **k),
        ws=(None, lambda dt: H.sgp_wstats_ws_elems(dt, N, M, d), "sgp_wstats_ws_elems"), mixed="w", strided="z"),
    Row("sgp_mwstats", lambda o, **k: H.sgp_mwstats(o.X, o.w2, o.r2, o.z, o.ell, o.W, **k),
        ws=(None, lambda dt: H.sgp_mwstats_ws_elems(dt, N, M, d, C), "sgp_mwstats_ws_elems"), mixed="z", strided="X"),
    Row("sgp_pathwise", lambda o, **k: H.sgp_pathwise(o.x, o.omega, o.z, o.ell, o.coef, **k),
        outs={"out": (S, n)}, mixed="omega", strided="x"),
    Row("sgp_pathwise_grad", lambda o, **k: H.sgp_pathwise_grad(o.x, o.omega, o.z, o.ell, o.coef, **k),
        outs={"out": (S, n), "grad": (S, n, d)}, mixed="coef", strided="z"),
    Row("sgp_pathwise_argmax", lambda o, **k: H.sgp_pathwise_argmax(o.x, o.omega, o.z, o.ell, o.coef, **k),
        ws=(None, lambda dt: H.sgp_pathwise_argmax_ws_elems(dt, n, S), "sgp_pathwise_argmax_ws_elems"), mixed="z", strided="omega"),
    Row("sgp_pathwise_acq", lambda o, **k: H.sgp_pathwise_acq(o.x, o.omega, o.z, o.ell, o.coef, o.inc, **k),
        ws=(F64, lambda dt: H.sgp_pathwise_acq_ws_elems(n, S), "sgp_pathwise_acq_ws_elems"), outs={"out": (n,)},
        mixed="omega", strided="x"),
    Row("gram_matvec", lambda o, **k: H.gram_matvec(o.x, o.X, o.ell, o.V, **k),
        ws=(None, lambda dt: H.gram_matvec_ws_elems(dt, n, N, S), "gram_matvec_ws_elems"), outs={"out": (S, n)},
        mixed="V", strided="x"),
    Row("gram_bilinear_grad", lambda o, **k: H.gram_bilinear_grad(o.X, o.ell, o.A, o.B, o.wv, **k),
        ws=(F64, lambda dt: H.gram_bilinear_grad_ws_elems(N, d), "gram_bilinear_grad_ws_elems"), outs={"out": ((1 + d,), F64)},
        mixed="A", strided="X"),
    Row("sgp_kgrad", lambda o, **k: H.sgp_kgrad(o.X, o.Y, o.z64, o.ell64, o.Q, o.R, **k),
        ws=(F64, lambda dt: H.sgp_kgrad_ws_elems(N, M, d, 1), "sgp_kgrad_ws_elems"), mixed="Y", strided="X"),
    Row("sgp_wkgrad", lambda o, **k: H.sgp_wkgrad(o.X, o.w64, o.r64, o.z64, o.ell64, o.Q, o.R, **k),
        ws=(F64, lambda dt: H.sgp_kgrad_ws_elems(N, M, d, 1), "sgp_kgrad_ws_elems"), mixed="w64", strided="z64"),
    Row("sgp_select", lambda o, **k: H.sgp_select(o.X, o.ell, 8, **k),
        ws=(None, lambda dt: H.sgp_select_ws_elems(dt, N, 8, d), "sgp_select_ws_elems"), mixed="ell", strided="X"),
    Row("cholesky_inverse", lambda o, **k: H.cholesky_inverse(o.spd, **k),
        ws=(None, lambda dt: H.cholesky_ws_elems(1, M, dt), "cholesky_ws_elems"), outs={"out": (M, M), "inv": (M, M)},
        strided="spd"),
    Row("gram_cholesky_inverse", lambda o, **k: H.gram_cholesky_inverse(o.pts, o.ell, 1e-3, **k),
        ws=(None, lambda dt: H.cholesky_ws_elems(1, 64, dt), "cholesky_ws_elems"), outs={"out": (64, 64), "inv": (64, 64)},
        strided="pts", dtypes=(F32,)),
    Row("mlp2_sample_fwd", lambda o, **k: H.mlp2_sample_fwd(o.y, o.w0, o.b0, o.w1, o.b1, "tanh", u_in=o.u, **k),
        ws=(F32, lambda dt: H.mlp2_sample_ws_elems(32, 32, 128), "mlp2_sample_ws_elems"),
        outs={"out": ((32, 16), (1,), (32, 16), (32, 32))}, mixed="w0", strided="y", dtypes=(F32,)),
    Row("mlp2_sample_bwd", lambda o, **k: H.mlp2_sample_bwd(o.y, o.w0, o.b0, o.w1, "tanh", o.eo, o.eu, o.ex, o.xbar, o.klbar, **k),
        ws=(F32, lambda dt: H.mlp2_sample_ws_elems(32, 32, 128), "mlp2_sample_ws_elems"),
        outs={"out": ((32, 128), (128,), (128, 32), (32,))}, mixed="w1", strided="w0", dtypes=(F32,)),
    # the older wrappers a plan emits: results of any contiguous shape with the right element count (exact=False)
    Row("gauss_ll", lambda o, **k: H.gauss_ll(o.V, o.A, None, o.var1, **k), outs={"out": ((1,), (S, N), (1,), (1,))}, strided="V"),
    Row("reduce_mid", lambda o, **k: H.reduce_mid(o.V, 1, S, N, **k), outs={"out": (N,)}, strided="V"),
    Row("gather_rows", lambda o, **k: H.gather_rows(o.X, o.idx, **k), outs={"out": (5, d)}, strided="X"),
    Row("matutil", lambda o, **k: H.matutil(o.spd, H.MATUTIL_SYM, **k), outs={"out": (M, M)}, strided="spd"),
    Row("fullrank_sample_kl_fwd", lambda o, **k: H.fullrank_sample_kl_fwd(o.fmu, o.fS, u_in=o.fu, **k),
        outs={"out": ((S, 8), (1,), (S, 8))}, strided="fmu"),
    Row("fullrank_sample_kl_bwd", lambda o, **k: H.fullrank_sample_kl_bwd(o.fS, o.fu, o.fx, o.fxbar, o.fklbar, **k),
        outs={"out": ((S, 8), (S, 8, 8))}, mixed="fxbar", strided="fu"),
    Row("vec_to_tri", lambda o, **k: H.vec_to_tri(o.tv, **k), outs={"out": (S, 4, 4)}, strided="tv"),
    Row("tri_to_vec", lambda o, **k: H.tri_to_vec(o.tt, **k), outs={"out": (10,)}, strided="tt"),
    Row("gram_fwd", lambda o, **k: H.gram_fwd(o.x, o.X, o.ell, **k), outs={"out": (n, N)}, strided="x"),
    Row("cholesky", lambda o, **k: H.cholesky(o.spd, **k), outs={"out": (M, M)}, strided="spd"),
    Row("trinv", lambda o, **k: H.trinv(o.W, **k), outs={"out": (M, M)}, strided="W"),
    Row("pcg_dot", lambda o, **k: H.pcg_dot(o.A, o.B, **k), outs={"out": ((S,), F64)}, strided="A"),
    Row("lik_sites", lambda o, **k: H.lik_sites(H.LIK_GAUSSIAN, o.mean, o.mean, o.var, **k),
        outs={"out": ((C * N,), (C * N,))}, strided="mean"),
    Row("lik_softmax_sites", lambda o, **k: H.lik_softmax_sites(o.labels, o.mean, o.var, o.nodes, **k),
        outs={"out": ((C, N), (C, N))}, strided="mean"),
]
CASES = [pytest.param(r, dt, id="%s-%s" % (r.who, str(dt)[6:])) for r in ROWS for dt in r.dtypes]


def _specs(row, dt):
    """{keyword: [(shape, dtype), ...], is_tuple}"""
    out = {}
    for kw, spec in row.outs.items():
        single = not isinstance(spec[0], tuple) or (len(spec) == 2 and isinstance(spec[1], torch.dtype))
        items = [spec] if single else list(spec)
        items = [(s[0], s[1]) if (len(s) == 2 and isinstance(s[1], torch.dtype)) else (tuple(s), dt) for s in items]
        out[kw] = (items, not single)
    return out


def _buffers(row, dt, fill=None):
    kw = {}
    for name, (items, is_tuple) in _specs(row, dt).items():
        ts = [torch.full(shape, SENTINEL if fill is None else fill, dtype=t, device="cuda") for shape, t in items]
        kw[name] = tuple(ts) if is_tuple else ts[0]
    return kw


def _flat(res):
    res = res if isinstance(res, (tuple, list)) else (res,)
    return [t for t in res if t is not None]


def _same_bits(a, b):
    if a.dtype.is_floating_point:
        iv = torch.int32 if a.dtype == F32 else torch.int64
        a, b = a.contiguous().view(iv), b.contiguous().view(iv)
    return a.shape == b.shape and bool(torch.equal(a, b))


def _ws_of(row, dt):
    wdt = row.ws[0] or dt
    return wdt, int(row.ws[1](dt)), row.ws[2]


def _roomy(shape, dt, like_bytes=8):
    """A contiguous tensor of `shape` and `dt` inside an allocation of at least `like_bytes` per element."""
    numel = int(np.prod(shape))
    return torch.zeros(max(numel, 1) * like_bytes // torch.empty((), dtype=dt).element_size(), dtype=dt, device="cuda")[:numel].view(shape)


@pytest.mark.parametrize("row, dt", CASES)
def test_exactly_sized_buffers_are_accepted_and_return_the_default_bits(row, dt):
    o = operands(dt)
    ref = _flat(row.call(o))
    kw = _buffers(row, dt)
    if row.ws is not None:
        wdt, need, _ = _ws_of(row, dt)
        kw["ws"] = torch.zeros(need + 64, dtype=wdt, device="cuda")[:need]
        assert kw["ws"].numel() == need
    got = _flat(row.call(o, **kw))
    torch.cuda.synchronize()
    assert len(got) == len(ref)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert _same_bits(a, b), "%s: result %d differs between explicit and default buffers" % (row.who, k)
    for name, (items, is_tuple) in _specs(row, dt).items():   # the results are the caller's buffers themselves
        given = kw[name] if is_tuple else (kw[name],)
        assert all(any(g.data_ptr() == t.data_ptr() for t in got) for g in given), (row.who, name)


@pytest.mark.parametrize("row, dt", [c for c in CASES if c.values[0].ws is not None])
def test_short_and_mistyped_workspaces_are_refused_before_any_launch(row, dt):
    o = operands(dt)
    wdt, need, query = _ws_of(row, dt)
    kw = _buffers(row, dt)
    if need > 0:
        whole = torch.zeros(need, dtype=wdt, device="cuda")
        with pytest.raises(ValueError, match="the workspace must hold") as e:
            row.call(o, ws=whole[:need - 1], **kw)
        assert row.who in str(e.value) and query in str(e.value) and str(need) in str(e.value)
    other = torch.zeros(2 * need + 16, dtype=_other(wdt), device="cuda")
    with pytest.raises(ValueError, match="the workspace must hold"):
        row.call(o, ws=other, **kw)
    torch.cuda.synchronize()
    for v in kw.values():
        for t in (v if isinstance(v, tuple) else (v,)):
            assert bool((t == SENTINEL).all()), "%s: a result was written although the call was refused" % row.who


@pytest.mark.parametrize("row, dt", [c for c in CASES if c.values[0].outs])
def test_results_of_the_wrong_shape_or_dtype_are_refused(row, dt):
    o = operands(dt)
    for name, (items, is_tuple) in _specs(row, dt).items():
        for k, (shape, t) in enumerate(items):
            for bad in (_roomy(shape[:-1] + (shape[-1] + 1,), t), _roomy(shape, _other(t))):
                kw = _buffers(row, dt)
                kw[name] = tuple(bad if j == k else b for j, b in enumerate(kw[name])) if is_tuple else bad
                with pytest.raises(ValueError, match=row.who):
                    row.call(o, **kw)


@pytest.mark.parametrize("row, dt", [c for c in CASES if c.values[0].mixed])
def test_an_operand_of_the_other_dtype_is_a_type_error(row, dt):
    o = Ops(operands(dt))
    o[row.mixed] = o[row.mixed].to(_other(o[row.mixed].dtype))
    with pytest.raises(TypeError, match=row.who):
        row.call(o)


@pytest.mark.parametrize("row, dt", CASES)
def test_a_transposed_view_is_refused(row, dt):
    o = Ops(operands(dt))
    t = o[row.strided]
    assert t.dim() == 2 and min(t.shape) > 1
    o[row.strided] = t.t().contiguous().t()
    assert o[row.strided].shape == t.shape and not o[row.strided].is_contiguous()
    with pytest.raises(ValueError, match="contiguous"):
        row.call(o)


def test_short_scratch_images_are_refused_by_name():
    """`frag` of cholesky_inverse, `abar_frag` of sgp_bwd_phi and `bws` of sgp_fwd_gauss_kbar: one element short (a view of a
    buffer of the full size), and of the other dtype, each raise ValueError naming the argument and its size query before
    anything is launched.  Every other buffer of these calls has its full size."""
    o = operands(F32)
    z = lambda k, dt=F32: torch.zeros(k, dtype=dt, device="cuda")
    need = H.cholesky_frag_elems(1, M, False)
    for bad in (z(need)[:need - 1], z(need, F64)):
        with pytest.raises(ValueError, match="cholesky_inverse: frag must hold.*cholesky_frag_elems"):
            H.cholesky_inverse(o.spd, frag=bad)
    with pytest.raises(ValueError, match="M % 32"):
        H.cholesky_inverse(z(48 * 48).view(48, 48), frag=z(2 * 48 * 48))
    fe, wse = H.sgp_frag_elems(1, n, M), H.sgp_ws_elems(1, n, M, d, 1)
    u, eps, v, fbar = z(M).view(1, M), z(n), z(n), z(n).view(1, n)
    for bad in (z(fe)[:fe - 1], z(fe, F64)):
        with pytest.raises(ValueError, match="sgp_bwd_phi: abar_frag must hold.*sgp_frag_elems"):
            H.sgp_bwd_phi(o.x, o.z, o.ell, o.W, u, eps, v, fbar, z(2 * M * M), z(fe), abar_frag=bad)
        with pytest.raises(ValueError, match="sgp_fwd_gauss_kbar: abar_frag must hold.*sgp_frag_elems"):
            H.sgp_fwd_gauss_kbar(o.x, o.z, o.ell, o.W, u, z(2 * M * M), z(fe), bad, z(wse), {"fbar": fbar})
    for bad in (z(wse)[:wse - 1], z(wse, F64)):
        with pytest.raises(ValueError, match="sgp_fwd_gauss_kbar: bws must hold.*sgp_ws_elems"):
            H.sgp_fwd_gauss_kbar(o.x, o.z, o.ell, o.W, u, z(2 * M * M), z(fe), z(fe), bad, {"fbar": fbar})
