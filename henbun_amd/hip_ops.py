"""Device-buffer level wrappers over the C ABI (include/henbun_hip.h).

PyTorch is used here ONLY as plumbing: `torch.empty(device='cuda')` for device
memory, `tensor.data_ptr()` for the raw pointer and the current stream handle.
No torch op computes anything on this path -- every function below is one (or
a fixed few) launches of hand-written HIP kernels through ctypes.  If the
backend library is missing, `_lib.lib()` raises; there is no fallback.

The header is the only place that states an enum value or a signature: the
constants below are looked up in `_lib.constants()`, and `_lib` binds every
entry point from its prototype and rejects a call with the wrong argument count.
"""
from __future__ import annotations

import collections
import ctypes
from ctypes import c_double, c_int, c_long, c_void_p

import numpy as np
import torch

from . import _lib

# ---- enums of include/henbun_hip.h: read from the header, never restated --------
_C = _lib.constants()


def _hb(*names):
    return [_C["HB_" + n] for n in names]


EW = {k[len("HB_EW_"):]: v for k, v in _C.items() if k.startswith("HB_EW_") and k != "HB_EW_PROG_SUM"}
RED_SUM, RED_MAX = _hb("RED_SUM", "RED_MAX")
KERN_RBF, KERN_CSYM_RBF, KERN_SQDIST = _hb("KERN_RBF", "KERN_CSYM_RBF", "KERN_SQDIST")
KERN_KBAR_SYMMETRIC = _C["HB_KERN_KBAR_SYMMETRIC"]   # OR-ed into the kind of gram_bwd: Kbar is symmetric (no transposed reads)
EW_PROG_SUM = _C["HB_EW_PROG_SUM"]
COLPROG_SUM, COLPROG_MAX = _hb("COLPROG_SUM", "COLPROG_MAX")   # row reductions of a column program
MM_LOWER_OUT, MM_TRIL_OUT, MM_PHI_OUT, MM_SYM_OUT = _hb("MM_LOWER_OUT", "MM_TRIL_OUT", "MM_PHI_OUT", "MM_SYM_OUT")
MM_SYMLOW_OUT, MM_ACTGRAD = _hb("MM_SYMLOW_OUT", "MM_ACTGRAD")
MM_FORM = {k[len("HB_MM_FORM_"):].lower(): v for k, v in _C.items() if k.startswith("HB_MM_FORM_")}   # hb_matmul_form
ACT = {k[len("HB_ACT_"):].lower(): v for k, v in _C.items() if k.startswith("HB_ACT_")}
SGP_NEGLECTED, SGP_DIAGONAL, SGP_FULLRANK = _hb("SGP_NEGLECTED", "SGP_DIAGONAL", "SGP_FULLRANK")
SGP_S_DIAG, SGP_S_TRIL = _hb("SGP_S_DIAG", "SGP_S_TRIL")
ACQ = {k[len("HB_ACQ_"):].lower(): v for k, v in _C.items() if k.startswith("HB_ACQ_")}   # 'ei', 'pi', 'ucb'
PWACQ = {k[len("HB_PWACQ_"):].lower(): v for k, v in _C.items() if k.startswith("HB_PWACQ_")}   # 'ei', 'pi': over function draws
PREC_NATIVE, PREC_BF16X3 = _hb("PREC_NATIVE", "PREC_BF16X3")
LIK_GAUSSIAN, LIK_BERNOULLI, LIK_POISSON = _hb("LIK_GAUSSIAN", "LIK_BERNOULLI", "LIK_POISSON")
LIK_LAPLACE, LIK_GAMMA, LIK_NEGBINOMIAL, LIK_BINOMIAL = _hb("LIK_LAPLACE", "LIK_GAMMA", "LIK_NEGBINOMIAL", "LIK_BINOMIAL")
LIK_SOFTMAX = _C["HB_LIK_SOFTMAX"]
LIK_HETGAUSS = _C["HB_LIK_HETGAUSS"]
MATUTIL_BAND, MATUTIL_ADD_EYE, MATUTIL_PHI, MATUTIL_SYM, MATUTIL_SYMLOW = _hb("MATUTIL_BAND", "MATUTIL_ADD_EYE", "MATUTIL_PHI",
                                                                              "MATUTIL_SYM", "MATUTIL_SYMLOW")

WS_ELEMS = 1 << 16  # generic scratch (elements) for reductions / KL partials


def _suf(t: torch.Tensor) -> str:
    if t.dtype == torch.float32:
        return "_f32"
    if t.dtype == torch.float64:
        return "_f64"
    raise TypeError("henbun_amd kernels compute in float32 or float64, got %s" % t.dtype)


def _elem_bytes(dtype) -> int:
    return 4 if dtype == torch.float32 else 8


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    if t is None:
        return None
    return c_void_p(t.data_ptr())


def _chk(t: torch.Tensor, name="tensor"):
    if not t.is_cuda:
        raise ValueError("%s must live on the GPU" % name)
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return t


def _larr(vals):
    return (c_long * len(vals))(*[int(v) for v in vals])


_capturing = False


def set_capturing(flag):
    """While a hipGraph is being captured every buffer must already exist: a tensor allocated inside
    the capture would be returned to torch's caching allocator afterwards and the graph would keep
    replaying into memory that now belongs to something else."""
    global _capturing
    _capturing = bool(flag)


def _empty(*a, **k):
    if _capturing:
        raise RuntimeError("henbun_amd: device allocation during hipGraph capture (an op was emitted without "
                           "preallocated outputs/workspace)")
    return torch.empty(*a, **k)


def _empty_like(t):
    if _capturing:
        raise RuntimeError("henbun_amd: device allocation during hipGraph capture (an op was emitted without "
                           "preallocated outputs/workspace)")
    return torch.empty_like(t)


_ws_cache = {}


_ws_retired = []


def workspace(dtype, device, elems=WS_ELEMS) -> torch.Tensor:
    """Shared scratch for the stream-ordered launches of one stream.  A workspace that has to grow is
    retired, never freed: captured hipGraphs may still hold its address."""
    key = (dtype, str(device), torch.cuda.current_stream().cuda_stream)
    w = _ws_cache.get(key)
    if w is None or w.numel() < elems:
        if w is not None:
            _ws_retired.append(w)
        w = _empty(max(elems, WS_ELEMS), dtype=dtype, device=device)
        _ws_cache[key] = w
    return w


# ---- the wrapper contract: operands, outputs, workspaces -------------------------------------------------------------------
# The C entries take every buffer as a bare pointer without a length, so these checks are the only ones a caller's
# buffer gets before a kernel writes through it.  None of them allocates, synchronises or reads device memory when the
# caller passed the buffer: plans emit the wrappers during capture with everything preallocated.
def _require(cond, who, what):
    """An extent or dtype the library takes on trust (a ValueError, not an assert: python -O must not drop it)."""
    if not cond:
        raise ValueError("%s: %s" % (who, what))


def _operands(who, ref, *tensors, what="all operands must share one dtype"):
    """Each tensor given (None entries are skipped) lives on the device, is contiguous and has the dtype of `ref` (a
    tensor, checked like the others, or a torch.dtype)."""
    dtype = ref if isinstance(ref, torch.dtype) else _chk(ref).dtype
    for t in tensors:
        if t is not None and _chk(t).dtype != dtype:
            raise TypeError("%s: %s" % (who, what))


def _out(who, t, shape, dtype, device, name="out", exact=True):
    """A result buffer: the caller's `t`, which must be contiguous and exactly `shape` of `dtype`, or a fresh one.
    exact=False: any contiguous shape of that many elements -- the wrappers a plan emits with the result in the shape of
    its own graph node (leading dims split or merged, a [1] result as a scalar): gauss_ll, reduce_mid, gather_rows,
    matutil, fullrank_sample_kl_fwd / _bwd, vec_to_tri, tri_to_vec, gram_fwd, cholesky, trinv, gram_cholesky_inverse;
    gram_bilinear_grad and lik_sites take any shape of the right count as well.
    Left to their wrappers, because the planner hands them views, strided blocks, column blocks or buffers larger than
    the result on purpose: ewise, copy_nd, matmul, matmul_ld, matmul_colsum, diag_sample_kl_fwd / _bwd (rows=), sgp_fwd /
    sgp_bwd and their relatives (sgp_A, sgp_fwd_gauss_kbar, sgp_bwd_phi, sgp_bwd_phi_rest), matmul_gram_vjp[_tiles],
    gram_ell_fold, gram_tiles_fold, gauss_ll_fold, matmul_gauss's head (raw plan buffers, sized by the plan from the
    library's own queries), lik_softmax_grad and lik_hetgauss_sites (padded rows, checked there), Rng.normal / randint
    (the result IS the shape argument), and the status words `info` / `err` of every entry (int32 / int64 views of the plan's status block)."""
    if t is None:
        return _empty(tuple(shape), dtype=dtype, device=device)
    shape = tuple(int(v) for v in shape)
    if _chk(t, name).dtype != dtype or (tuple(t.shape) != shape if exact else t.numel() != int(np.prod(shape))):
        raise ValueError("%s: %s must be %s%s of the operands' dtype" % (who, name, list(shape), "" if exact else
                                                                         " (or any shape of as many elements)"))
    return t


def _outs(who, ts, shapes, dtype, device, names, exact=True):
    """_out for a tuple of results (`ts` None: all fresh)."""
    ts = (None,) * len(shapes) if ts is None else tuple(ts)
    if len(ts) != len(shapes):
        raise ValueError("%s: out must be (%s)" % (who, ", ".join(names)))
    return tuple(_out(who, t, s, dtype, device, n, exact) for t, s, n in zip(ts, shapes, names))


def _ws(who, ws, dtype, device, need, query, name="the workspace"):
    """A workspace of `need` elements of `dtype`: the caller's, checked, or the shared scratch of the stream.  `query`
    names the *_ws_elems function that answers `need`; `name`: the argument, for a scratch buffer that is not `ws`."""
    if ws is None:
        return workspace(dtype, device, max(need, 1))
    if _chk(ws, name).dtype != dtype or ws.numel() < need:
        raise ValueError("%s: %s must hold %d elements of %s (%s)" % (who, name, need, dtype, query))
    return ws


def _code(who, table, value, name="acq"):
    """The code of a name-or-code argument in one of the enum tables (ACQ, PWACQ)."""
    code = table.get(value) if isinstance(value, str) else value
    if code not in table.values():
        raise ValueError("%s: %s must be one of %s, got %r" % (who, name, sorted(table), value))
    return code


def _query(name, *ints):
    """An integer answer of the library's host-side size and form rules (nothing runs on the device)."""
    return int(_lib.lib().raw(name)(*[int(v) for v in ints]))


def _bcast_strides(shape, out_shape):
    """element strides of a contiguous tensor of `shape` viewed as `out_shape` (0 on broadcast dims)."""
    nd = len(out_shape)
    shape = (1,) * (nd - len(shape)) + tuple(shape)
    strides, acc = [0] * nd, 1
    for d in range(nd - 1, -1, -1):
        if shape[d] == 1 and out_shape[d] != 1:
            strides[d] = 0
        elif shape[d] == out_shape[d]:
            strides[d] = acc if shape[d] != 1 else 0
        else:
            raise ValueError("shape %s does not broadcast to %s" % (shape, out_shape))
        acc *= shape[d]
    return strides


def ewise(op, inputs, nout=1, params=None, out=None):
    """n-ary broadcasting elementwise op (hb_ewise_*).  Returns a tensor or a tuple."""
    opc = EW[op] if isinstance(op, str) else int(op)
    inputs = [_chk(t, "input") for t in inputs]
    out_shape = tuple(torch.broadcast_shapes(*[tuple(t.shape) for t in inputs]))
    if out is not None:
        # explicit result buffers may be larger than the operands' common shape (operands broadcast into them)
        o0 = out[0] if isinstance(out, (list, tuple)) else out
        out_shape = tuple(torch.broadcast_shapes(out_shape, tuple(o0.shape)))
    if len(out_shape) > 6:
        raise ValueError("elementwise ops support at most 6 dims")
    nin = len(inputs)
    nd = len(out_shape)
    strides = []
    for t in inputs:
        strides += _bcast_strides(tuple(t.shape), out_shape)
    if out is None:
        outs = [_empty(out_shape, dtype=inputs[0].dtype, device=inputs[0].device) for _ in range(nout)]
    else:
        outs = list(out) if isinstance(out, (list, tuple)) else [out]
        for o in outs:
            _require(tuple(o.shape) == out_shape and o.is_contiguous(), "ewise", "out must be contiguous %s" % (out_shape,))
    in_arr = (c_void_p * nin)(*[t.data_ptr() for t in inputs])
    out_arr = (c_void_p * nout)(*[o.data_ptr() for o in outs])
    pr = (c_double * 4)(*(list(params or []) + [0.0] * 4)[:4])
    _lib.lib().call("hb_ewise" + _suf(inputs[0]), opc, nin, in_arr, _larr(strides) if strides else _larr([0]),
                    nout, out_arr, nd, _larr(out_shape) if nd else _larr([1]), pr, stream())
    return outs[0] if nout == 1 else tuple(outs)


EWISE_JIT_SOURCE_BYTES = 8192


def ewise_jit_enabled():
    """Fused elementwise programs are compiled at plan-build time (hiprtc) unless `settings.runtime.ewise = interpret`
    or hiprtc cannot be loaded in this process; the interpreted form is the same program run by ew_prog_image_kernel."""
    from ._settings import settings

    if getattr(settings.runtime, "ewise", "jit") != "jit":
        return False
    return bool(_query("hb_ewise_jit_available"))


class EwiseProgram:
    """A prepared hb_ewise_prog launch (all host-side argument arrays built once)."""

    def __init__(self, code, params, inputs, istrides, outputs, out_regs, ostrides, shape):
        from ctypes import c_int

        self.suf = _suf(outputs[0])
        self.ninstr = len(code)
        self.code = (c_int * (5 * len(code)))(*[int(v) for ins in code for v in ins])
        self.params = (c_double * (2 * len(code)))(*[float(v) for pr in params for v in pr])
        self.nin = len(inputs)
        self.inputs = (c_void_p * max(self.nin, 1))(*[t.data_ptr() for t in inputs])
        self.nd = len(shape)
        flat_is = [s for st in istrides for s in st]
        self.istr = _larr(flat_is) if flat_is else _larr([0])
        self.nout = len(outputs)
        self.outputs = (c_void_p * self.nout)(*[t.data_ptr() for t in outputs])
        self.out_regs = (c_int * self.nout)(*[int(r) for r in out_regs])
        flat_os = [s for st in ostrides for s in st]
        self.ostr = _larr(flat_os) if flat_os else _larr([0])
        self.shape = _larr(shape) if shape else _larr([1])
        self._keep = (inputs, outputs)
        lib = _lib.lib()
        self.handle = None
        self.source = None
        if ewise_jit_enabled():
            # compiled form: the program becomes a gfx950 kernel of its own at plan-build time (hb_ewise_jit_*)
            n_out, red_out = c_long(0), c_int(0)
            handle = c_void_p(None)
            src = ctypes.create_string_buffer(EWISE_JIT_SOURCE_BYTES)
            lib.call("hb_ewise_jit_build" + self.suf, self.ninstr, self.code, self.params, self.nin, self.inputs, self.istr,
                     self.nout, self.outputs, self.out_regs, self.ostr, self.nd, self.shape, ctypes.byref(handle),
                     ctypes.byref(n_out), ctypes.byref(red_out), src, EWISE_JIT_SOURCE_BYTES)
            self.n, self.reduces = int(n_out.value), int(red_out.value)
            self.handle = handle
            self.source = src.value.decode()
            self.image = None
            return
        # interpreted form: the launch descriptor is built and uploaded once; a (replayed) launch carries one pointer
        # and the kernel pulls the descriptor into LDS in one parallel load
        nbytes = int(lib.raw("hb_ewise_prog_image_bytes")())
        host = ctypes.create_string_buffer(nbytes)
        n_out, red_out = c_long(0), c_int(0)
        lib.call("hb_ewise_prog_build", self.ninstr, self.code, self.params, self.nin, self.inputs, self.istr, self.nout,
                 self.outputs, self.out_regs, self.ostr, self.nd, self.shape, host, ctypes.byref(n_out),
                 ctypes.byref(red_out))
        self.n, self.reduces = int(n_out.value), int(red_out.value)
        self.image = torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(outputs[0].device)
        torch.cuda.synchronize()

    def launch(self):
        if self.image is None:
            _lib.lib().call("hb_ewise_jit_run", self.handle, stream())
        else:
            _lib.lib().call("hb_ewise_prog_run" + self.suf, _p(self.image), self.n, self.reduces, stream())

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                _lib.lib().raw("hb_ewise_jit_destroy")(h)
            except Exception:
                pass




class ColProgram:
    """A prepared column program (hb_ewise_colprog_build): a fused program over an [R, n] space, one thread per
    column, reductions over the row axis as ordinary instructions.

    `inputs` / `outputs`: lists of (tensor, element offset, row stride, column stride); code rows are
    [op, dst, a, b, c] with -1 for an unused operand slot."""

    def __init__(self, code, params, inputs, outputs, out_regs, R, n, dry=False):
        from ctypes import c_int

        ref = (outputs[0][0] if outputs else inputs[0][0])
        self.suf = _suf(ref)
        isz = ref.element_size()
        self.ninstr = len(code)
        self.code = (c_int * (5 * len(code)))(*[int(v) for ins in code for v in ins])
        self.params = (c_double * (2 * len(code)))(*[float(v) for pr in params for v in pr])
        self.nin, self.nout = len(inputs), len(outputs)
        self.inputs = (c_void_p * max(self.nin, 1))(*[t.data_ptr() + int(off) * isz for t, off, _, _ in inputs])
        self.istr = _larr([v for _, _, rs, cs in inputs for v in (rs, cs)] or [0])
        self.outputs = (c_void_p * self.nout)(*[t.data_ptr() + int(off) * isz for t, off, _, _ in outputs])
        self.ostr = _larr([v for _, _, rs, cs in outputs for v in (rs, cs)])
        self.out_regs = (c_int * self.nout)(*[int(r) for r in out_regs])
        self._keep = (inputs, outputs)
        self.R, self.n = int(R), int(n)
        src = ctypes.create_string_buffer(EWISE_JIT_SOURCE_BYTES)
        handle = c_void_p(None)
        _lib.lib().call("hb_ewise_colprog_build" + self.suf, self.ninstr, self.code, self.params, self.nin, self.inputs, self.istr,
                        self.nout, self.outputs, self.out_regs, self.ostr, self.R, self.n,
                        None if dry else ctypes.byref(handle), src, EWISE_JIT_SOURCE_BYTES)
        self.handle = None if dry else handle
        self.source = src.value.decode()

    def launch(self):
        _lib.lib().call("hb_ewise_jit_run", self.handle, stream())

    def __del__(self):
        h = getattr(self, "handle", None)
        if h is not None and h.value:
            try:
                _lib.lib().raw("hb_ewise_jit_destroy")(h)
            except Exception:
                pass


def gauss_ll(x, f, scale, var, out=None, post=None, fbar=None):
    """(ll[1], dmu[like x], dscale[1], dvar[1]) of sum_j log N(x_j | f_j*scale, var)  (hb_gauss_ll; scale may be None).
    `post`, `fbar`: also fbar = scale * (post * dmu), the gradient of post * ll w.r.t. f (hb_gauss_ll_post)."""
    _chk(x), _chk(f), _chk(var)
    _require(x.numel() == f.numel() and var.numel() == 1 and (scale is None or scale.numel() == 1), "gauss_ll",
             "x and f of one size, one variance and at most one scale expected")
    n = x.numel()
    ll, dmu, ds, dv = _outs("gauss_ll", out, ((1,), tuple(x.shape), (1,), (1,)), x.dtype, x.device, ("ll", "dmu", "dscale", "dvar"),
                            exact=False)
    ws = workspace(x.dtype, x.device, 3 * max((n + 1023) // 1024, 1))
    if fbar is not None:
        _chk(fbar)
        _require(fbar.numel() == n, "gauss_ll", "fbar must hold the elements of x")
        _lib.lib().call("hb_gauss_ll_post" + _suf(x), _p(x), _p(f), _p(scale), _p(var), n, _p(ll), _p(dmu), _p(ds), _p(dv),
                        float(post), _p(fbar), _p(ws), ws.numel(), stream())
        return ll, dmu, ds, dv
    _lib.lib().call("hb_gauss_ll" + _suf(x), _p(x), _p(f), _p(scale), _p(var), n, _p(ll), _p(dmu), _p(ds), _p(dv), _p(ws),
                    ws.numel(), stream())
    return ll, dmu, ds, dv


def reduce_mid(x, K1, R, K2, op=RED_SUM, out=None):
    """out[K1,K2] = reduce_R x[K1,R,K2] (x contiguous, any shape with K1*R*K2 elements)."""
    _chk(x)
    _require(x.numel() == K1 * R * K2, "reduce_mid", "x must hold K1 R K2 elements")
    out = _out("reduce_mid", out, (K1 * K2,), x.dtype, x.device, exact=False)
    ws = workspace(x.dtype, x.device)
    _lib.lib().call("hb_reduce" + _suf(x), op, _p(x), _p(out), K1, R, K2, _p(ws), ws.numel(), stream())
    return out


def copy_nd(src, src_strides, dst, dst_strides, shape, src_off=0, dst_off=0):
    """strided element copy; strides/offsets in elements over the flat buffers."""
    es = src.element_size()
    sp = c_void_p(src.data_ptr() + src_off * es)
    dp = c_void_p(dst.data_ptr() + dst_off * es)
    nd = len(shape)
    _lib.lib().call("hb_copy_nd" + _suf(src), sp, _larr(src_strides) if nd else _larr([0]), dp,
                    _larr(dst_strides) if nd else _larr([0]), nd, _larr(shape) if nd else _larr([1]), stream())
    return dst


def fill(t, value):
    _lib.lib().call("hb_fill" + _suf(t), _p(t), t.numel(), float(value), stream())
    return t


def gather_rows(src, idx, perm=None, out=None, err=None):
    """out[i,:] = src[perm[idx[i]],:]  (K0)."""
    _chk(src)
    nsrc = src.shape[0]
    row = src.numel() // max(nsrc, 1)
    n = idx.numel()
    out = _out("gather_rows", out, (n,) + tuple(src.shape[1:]), src.dtype, src.device, exact=False)
    _require(idx.dtype == torch.int64 and (perm is None or perm.dtype == torch.int64), "gather_rows", "int64 idx and perm expected")
    _lib.lib().call("hb_gather_rows" + _suf(src), _p(src), nsrc, row, _p(idx), _p(perm), n, _p(out), _p(err), stream())
    return out


class MultiGather:
    """out_a[i,:] = src_a[perm[idx[i]],:] for several arrays sharing idx, one launch (argument arrays built once)."""

    def __init__(self, srcs, outs, idx, perm, err):
        _require(1 <= len(srcs) <= 8 and len(srcs) == len(outs), "MultiGather", "1 to 8 arrays and as many outputs expected")
        nsrc = srcs[0].shape[0]
        for s in srcs:
            _chk(s)
            _require(s.shape[0] == nsrc and s.dtype == srcs[0].dtype, "MultiGather", "arrays of one row count and dtype expected")
        self.suf = _suf(srcs[0])
        self.narr, self.nsrc, self.n = len(srcs), nsrc, idx.numel()
        self.srcs = (c_void_p * self.narr)(*[s.data_ptr() for s in srcs])
        self.dsts = (c_void_p * self.narr)(*[o.data_ptr() for o in outs])
        self.rows = _larr([s.numel() // max(nsrc, 1) for s in srcs])
        self.idx, self.perm, self.err = idx, perm, err
        self._keep = (srcs, outs)

    def launch(self, use_perm=True):
        _lib.lib().call("hb_gather_rows_multi" + self.suf, self.narr, self.srcs, self.rows, self.dsts, self.nsrc,
                        _p(self.idx), _p(self.perm if use_perm else None), self.n, _p(self.err), stream())

    def launch_draw(self, rng, lo, hi, use_perm=True, defer=False):
        """draw idx ~ U{lo..hi-1} from `rng` (as rng.randint would) and gather, in one launch; needs n <= rng.nlanes.
        defer: recorded as a side job of the next host launch (fp32 only) instead of launched now."""
        name = "hb_side_push_gather_draw_f32" if (defer and self.suf == "_f32") else "hb_gather_rows_multi_draw" + self.suf
        _lib.lib().call(name, self.narr, self.srcs, self.rows, self.dsts, self.nsrc,
                        _p(rng.state), rng.nlanes, int(lo), int(hi), _p(self.idx), _p(self.perm if use_perm else None),
                        self.n, _p(self.err), stream())


def matutil(x, mode, lower=-1, upper=-1, alpha=0.0, out=None):
    _chk(x)
    R, C = x.shape[-2], x.shape[-1]
    B = x.numel() // max(R * C, 1)
    out = _out("matutil", out, tuple(x.shape), x.dtype, x.device, exact=False)
    _lib.lib().call("hb_matutil" + _suf(x), _p(x), _p(out), B, R, C, mode, lower, upper, float(alpha), stream())
    return out


# ---- RNG --------------------------------------------------------------------
class Rng:
    """xoroshiro128+ per-lane state on the device (hb_rng_*)."""

    def __init__(self, seed, stream_id=0, nlanes=65536, device="cuda"):
        self.nlanes = int(nlanes)
        self.state = _empty(2 * self.nlanes, dtype=torch.int64, device=device)
        self.seed, self.stream_id = int(seed), int(stream_id)
        self.reseed(seed, stream_id)

    def reseed(self, seed, stream_id=0):
        self.seed, self.stream_id = int(seed), int(stream_id)
        _lib.lib().call("hb_rng_init", _p(self.state), self.nlanes, int(seed) & (2**64 - 1),
                        int(stream_id) & (2**64 - 1), stream())

    def normal(self, shape, dtype=torch.float32, out=None):
        if out is None:
            out = _empty(shape, dtype=dtype, device=self.state.device)
        _lib.lib().call("hb_rng_normal" + _suf(out), _p(self.state), self.nlanes, _p(out), out.numel(), stream())
        return out

    def randint(self, n, lo, hi, out=None):
        if out is None:
            out = _empty(n, dtype=torch.int64, device=self.state.device)
        _lib.lib().call("hb_rng_randint", _p(self.state), self.nlanes, _p(out), out.numel(), int(lo), int(hi), stream())
        return out


def _rng_args(rng):
    if rng is None:
        return None, 0
    return _p(rng.state), rng.nlanes


# ---- K1/K2 variational sampler + MC-KL --------------------------------------
def side_flush():
    """Launch whatever side jobs are still pending on this thread (hb_side_flush); a no-op when a host launch took them."""
    _lib.lib().call("hb_side_flush", stream())


def side_pending():
    return _query("hb_side_pending")


def chain_begin():
    """Start recording a serial chain on this thread (hb_chain_begin): the small launches of the chain-aware entry points
    that follow run as one generated kernel at chain_end()."""
    _lib.lib().call("hb_chain_begin")


def chain_end():
    _lib.lib().call("hb_chain_end", stream())


def chain_discard():
    return _query("hb_chain_discard")


def chain_source():
    buf = ctypes.create_string_buffer(1 << 16)
    _lib.lib().call("hb_chain_source", buf, 1 << 16)
    return buf.value.decode()


def side_discard():
    """Drop this thread's recorded side jobs without running them (hb_side_discard); returns how many there were."""
    return _query("hb_side_discard")


def diag_sample_kl_fwd(mu, s, u_in=None, rng=None, out=None, rows=None, defer=False):
    """x = mu + exp(s)*u ; kl = -0.5*sum(2s + u^2 - x^2).  Returns (x, kl, u).
    rows=(nrows, L, ld_mu, ld_s): mu and s are column blocks of wider row-major matrices (1-D views starting at their
    first element), read in place; x and u are dense [nrows, L] (out= is then required)."""
    _chk(mu), _chk(s)
    if rows is None:
        n = mu.numel()
        L = ldm = lds = max(n, 1)
    else:
        nrows, L, ldm, lds = (int(v) for v in rows)
        n = nrows * L
        if out is None:
            raise ValueError("diag_sample_kl_fwd: strided inputs need explicit outputs")
    if out is None:
        x, kl, u = _empty_like(mu), _empty(1, dtype=mu.dtype, device=mu.device), _empty_like(mu)
    else:
        x, kl, u = out
    ws = workspace(mu.dtype, mu.device)
    rp, rl = _rng_args(rng)
    # defer: recorded as a side job of the next host launch (hb_side_push_*; fp32 only) instead of launched now
    name = "hb_side_push_diag_fwd_f32" if (defer and mu.dtype == torch.float32) else "hb_diag_sample_kl_fwd" + _suf(mu)
    _lib.lib().call(name, _p(mu), _p(s), _p(u_in), rp, rl, _p(u), _p(x), _p(kl), n, L, ldm, lds, _p(ws), stream())
    return x, kl, u


def diag_sample_kl_bwd(s, u, x, xbar, klbar, out=None, rows=None, defer=False):
    """rows=(nrows, L, ld_s, ld_out): s read, mubar/sbar written, as column blocks of wider matrices (see _fwd)."""
    if rows is None:
        n = s.numel()
        L = lds = ldo = max(n, 1)
    else:
        nrows, L, lds, ldo = (int(v) for v in rows)
        n = nrows * L
        if out is None:
            raise ValueError("diag_sample_kl_bwd: strided layout needs explicit outputs")
    if out is None:
        mubar, sbar = _empty_like(s), _empty_like(s)
    else:
        mubar, sbar = out
    name = "hb_side_push_diag_bwd_f32" if (defer and s.dtype == torch.float32) else "hb_diag_sample_kl_bwd" + _suf(s)
    _lib.lib().call(name, _p(s), _p(u), _p(x), _p(xbar), _p(klbar), _p(mubar), _p(sbar), n, L, lds, ldo, stream())
    return mubar, sbar


def fullrank_sample_kl_fwd(mu, S, u_in=None, rng=None, out=None, packed=False):
    """x_r = mu_r + tril(S_r) u_r over rows; S [..., size, size], or packed [..., size(size+1)/2] (lower triangle,
    tril_indices order)."""
    _chk(mu), _chk(S)
    size = mu.shape[-1]
    rows = mu.numel() // max(size, 1)
    _require(S.numel() == rows * (size * (size + 1) // 2 if packed else size * size), "fullrank_sample_kl_fwd",
             "S must hold one (packed) lower triangle per row of mu")
    x, kl, u = _outs("fullrank_sample_kl_fwd", out, (tuple(mu.shape), (1,), tuple(mu.shape)), mu.dtype, mu.device,
                     ("x", "kl", "u"), exact=False)
    ws = workspace(mu.dtype, mu.device)
    rp, rl = _rng_args(rng)
    # (one launch for a block of up to 1024 dimensions; the entry falls back to the three-launch form by itself)
    _lib.lib().call("hb_fullrank_sample_kl_fwd1" + _suf(mu), _p(mu), _p(S), _p(u_in), rp, rl, _p(u), _p(x), _p(kl),
                    rows, size, int(bool(packed)), _p(ws), _p(sync_word(mu.device)), stream())
    return x, kl, u


_SYNC_WORDS = {}


def sync_word(device):
    """One zero 32-bit word per (device, stream) for the kernels that meet at an arrival counter (zero at entry, left zero
    by every call; launches on one stream are ordered, so they can share it)."""
    key = (str(device), stream())
    b = _SYNC_WORDS.get(key)
    if b is None:
        b = _SYNC_WORDS[key] = torch.zeros(4, dtype=torch.int32, device=device)
    return b


def fullrank_sample_kl_bwd(S, u, x, xbar, klbar, out=None, packed=False):
    _operands("fullrank_sample_kl_bwd", S, u, x, xbar, klbar)
    size = u.shape[-1]
    rows = u.numel() // max(size, 1)
    mubar, Sbar = _outs("fullrank_sample_kl_bwd", out, (tuple(u.shape), tuple(S.shape)), S.dtype, S.device, ("mubar", "Sbar"),
                        exact=False)
    _lib.lib().call("hb_fullrank_sample_kl_bwd" + _suf(S), _p(S), _p(u), _p(x), _p(xbar), _p(klbar), _p(mubar),
                    _p(Sbar), rows, size, int(bool(packed)), stream())
    return mubar, Sbar


def tri_size(n_packed):
    """N with N(N+1)/2 == n_packed."""
    N = int((8 * n_packed + 1) ** 0.5 / 2.0 - 0.5 + 1e-9)
    if N * (N + 1) // 2 != n_packed:
        raise ValueError("%d is not a triangular number" % n_packed)
    return N


def vec_to_tri(v, out=None):
    """[..., N(N+1)/2] -> lower-triangular [..., N, N] (reference tf_wraps.py:50-71)."""
    _chk(v)
    N = tri_size(v.shape[-1])
    B = v.numel() // max(v.shape[-1], 1)
    out = _out("vec_to_tri", out, tuple(v.shape[:-1]) + (N, N), v.dtype, v.device, exact=False)
    _lib.lib().call("hb_vec_to_tri" + _suf(v), _p(v), _p(out), B, N, stream())
    return out


def tri_to_vec(tri, out=None):
    """Lower triangle of [..., N, N] -> [..., N(N+1)/2] (the gradient of vec_to_tri)."""
    _chk(tri)
    N = tri.shape[-1]
    B = tri.numel() // max(N * N, 1)
    out = _out("tri_to_vec", out, tuple(tri.shape[:-2]) + (N * (N + 1) // 2,), tri.dtype, tri.device, exact=False)
    _lib.lib().call("hb_tri_to_vec" + _suf(tri), _p(tri), _p(out), B, N, stream())
    return out


# ---- K3 Gram ------------------------------------------------------------------
def _batch_view(X, nd_tail=2):
    """(B, stride) of a [..., n, d] tensor flattened over leading dims."""
    n, d = X.shape[-2], X.shape[-1]
    B = X.numel() // max(n * d, 1)
    return B, n, d


def _ell_layout(ell, B, d):
    """(sEll, dl): a lengthscale tensor [dl] is shared by the batch, [B, dl] gives one kernel per batch entry."""
    if ell.dim() >= 2 and ell.shape[0] == B and B > 1:
        dl = ell.numel() // B
        return dl, dl
    return 0, ell.numel()


def gram_fwd(X, X2, ell, kind=KERN_RBF, out=None, diag_add=0.0):
    """K[b,i,j] = k(X[b,i], X2[b,j]); X, X2: [n,d] or [B,n,d] (a 2-D operand is shared over B);
    ell: [dl] (shared) or [B, dl] (one kernel per batch entry)."""
    _chk(X), _chk(X2), _chk(ell)
    BX, n, d = _batch_view(X)
    BX2, n2, d2 = _batch_view(X2)
    _require(d == d2, "gram_fwd", "X and X2 must share their last extent")
    B = max(BX, BX2)
    if ell.dim() >= 2 and ell.shape[0] > 1:
        B = max(B, ell.shape[0])
    _require(BX in (1, B) and BX2 in (1, B), "gram_fwd", "batch extents must match or be absent")
    sX = n * d if (BX == B and B > 1) else 0
    sX2 = n2 * d if (BX2 == B and B > 1) else 0
    sEll, dl = _ell_layout(ell, B, d)
    batched = X.dim() > 2 or X2.dim() > 2 or sEll != 0
    lead = tuple(X.shape[:-2]) if X.dim() > 2 else (tuple(X2.shape[:-2]) if X2.dim() > 2 else ((B,) if sEll else ()))
    out = _out("gram_fwd", out, (lead if batched else ()) + (n, n2), X.dtype, X.device, exact=False)
    _lib.lib().call("hb_gram_fwd" + _suf(X), kind, _p(X), sX, _p(X2), sX2, _p(ell), sEll, dl, _p(out), B, n, n2, d,
                    float(diag_add), stream())
    return out


def gram_bwd_raw(kind, X, sX, X2, sX2, ell, sEll, dl, Kbar, Xbar, X2bar, ellbar, B, n, n2, d, ws):
    """hb_gram_bwd on caller-provided buffers (no allocation: graph-capturable)."""
    _lib.lib().call("hb_gram_bwd" + _suf(X), kind, _p(X), sX, _p(X2), sX2, _p(ell), sEll, dl, _p(Kbar), _p(Xbar),
                    _p(X2bar), _p(ellbar), B, n, n2, d, _p(ws), stream())


def gram_bwd(X, X2, ell, Kbar, kind=KERN_RBF, need=(True, True, True)):
    """VJP of gram_fwd: returns (Xbar, X2bar, ellbar) (None where not needed).
    Operands shared over the batch get their gradient summed over it."""
    _chk(X), _chk(X2), _chk(ell), _chk(Kbar)
    BX, n, d = _batch_view(X)
    BX2, n2, _ = _batch_view(X2)
    B = max(BX, BX2)
    if ell.dim() >= 2 and ell.shape[0] > 1:
        B = max(B, ell.shape[0])
    sX = n * d if (BX == B and B > 1) else 0
    sX2 = n2 * d if (BX2 == B and B > 1) else 0
    sEll, dl = _ell_layout(ell, B, d)
    dev, dt = X.device, X.dtype
    Xbar = _empty((B, n, d), dtype=dt, device=dev) if need[0] else None
    X2bar = _empty((B, n2, d), dtype=dt, device=dev) if need[1] else None
    ellbar = _empty(ell.numel(), dtype=dt, device=dev) if need[2] else None
    ws = workspace(dt, dev, max(B * n * d, 1))
    gram_bwd_raw(kind, X, sX, X2, sX2, ell, sEll, dl, Kbar, Xbar, X2bar, ellbar, B, n, n2, d, ws)
    if Xbar is not None:
        Xbar = reduce_mid(Xbar, 1, B, n * d).reshape(X.shape) if (BX == 1 and B > 1) else Xbar.reshape(X.shape)
    if X2bar is not None:
        X2bar = reduce_mid(X2bar, 1, B, n2 * d).reshape(X2.shape) if (BX2 == 1 and B > 1) else X2bar.reshape(X2.shape)
    if ellbar is not None:
        ellbar = ellbar.reshape(ell.shape)
    return Xbar, X2bar, ellbar


# ---- dense linear algebra ------------------------------------------------------
def matmul(A, B, transA=False, transB=False, alpha=1.0, bias=None, act="none", lower_out=False, out=None,
           beta=0.0, tril_out=False, epilogue=0, actgrad=None):
    """C = act(alpha*op(A)@op(B) + bias) (+ beta*C).  A:[...,m,k], B:[...,k,n]; a 2-D operand broadcasts
    over the other's leading (batch) dims.  bias: [n] or [batch..., n]/[batch...,1,n].
    actgrad=Y: C = alpha*op(A)@op(B) * act'(Y), Y = the output of activation `act` ([..., m, n], contiguous)."""
    _chk(A), _chk(B)
    am, ak = (A.shape[-1], A.shape[-2]) if transA else (A.shape[-2], A.shape[-1])
    bk, bn = (B.shape[-1], B.shape[-2]) if transB else (B.shape[-2], B.shape[-1])
    if ak != bk:
        raise ValueError("matmul inner dims differ: %s vs %s" % (tuple(A.shape), tuple(B.shape)))
    la, lb = tuple(A.shape[:-2]), tuple(B.shape[:-2])
    ba, bb = int(np.prod(la)) if la else 1, int(np.prod(lb)) if lb else 1
    if ba != bb and ba != 1 and bb != 1:
        raise ValueError("matmul batch dims must match or be absent: %s vs %s" % (la, lb))
    batch = max(ba, bb)
    lead = la if ba >= bb else lb
    sA = A.shape[-2] * A.shape[-1] if (ba == batch and batch > 1) else 0
    sB = B.shape[-2] * B.shape[-1] if (bb == batch and batch > 1) else 0
    if out is None:
        out = _empty(lead + (am, bn), dtype=A.dtype, device=A.device)
    sBias = 0
    if actgrad is not None:
        _chk(actgrad)
        if bias is not None or beta != 0.0 or lower_out or tril_out or epilogue:
            raise ValueError("matmul: actgrad excludes bias, beta and the triangular epilogues")
        if tuple(actgrad.shape[-2:]) != (am, bn) or actgrad.numel() not in (am * bn, batch * am * bn):
            raise ValueError("matmul: actgrad operand %s does not match the result [%d,%d]" % (tuple(actgrad.shape), am, bn))
        if not actgrad.is_contiguous() or actgrad.dtype != A.dtype:
            raise ValueError("matmul: actgrad operand must be contiguous and of the operands' dtype")
        bias, epilogue = actgrad, MM_ACTGRAD
        sBias = am * bn if (actgrad.numel() == batch * am * bn and batch > 1) else 0
    elif bias is not None:
        _chk(bias)
        if bias.numel() == bn:
            sBias = 0
        elif bias.numel() == batch * bn:
            sBias = bn
        else:
            raise ValueError("bias shape %s does not match [%d] or [%d,%d]" % (tuple(bias.shape), bn, batch, bn))
    ws = workspace(A.dtype, A.device, 1 << 22)
    _lib.lib().call("hb_matmul" + _suf(A), _p(A), _p(B), _p(out), batch, am, bn, ak, A.shape[-1], B.shape[-1], bn,
                    sA, sB, am * bn, int(transA), int(transB), float(alpha), float(beta), _p(bias), sBias, ACT[act],
                    (MM_LOWER_OUT if lower_out else 0) | (MM_TRIL_OUT if tril_out else 0) | int(epilogue), _p(ws), ws.numel(), stream())
    return out


def matmul_ld(A, lda, B, ldb, out, m, n, k, transB=False, alpha=1.0):
    """out [m, n] (contiguous) = alpha op(A) op(B) with explicit row strides: A [m, k] at stride lda, B [k, n] (transB:
    [n, k]) at stride ldb -- operands that are the leading rows of a wider buffer, such as the history of sgp_select."""
    if A.dtype != B.dtype or out.dtype != A.dtype or out.numel() < m * n or not out.is_contiguous():
        raise ValueError("matmul_ld: one dtype and a contiguous out of m n elements expected")
    need_a = (m - 1) * lda + k
    need_b = ((n - 1) * ldb + k) if transB else ((k - 1) * ldb + n)
    if lda < k or ldb < (k if transB else n) or A.numel() < need_a or B.numel() < need_b:
        raise ValueError("matmul_ld: operands shorter than their extents and strides")
    ws = workspace(A.dtype, A.device, 1 << 22)
    _lib.lib().call("hb_matmul" + _suf(A), _p(A), _p(B), _p(out), 1, m, n, k, lda, ldb, n, 0, 0, 0, 0, int(transB),
                    float(alpha), 0.0, None, 0, ACT["none"], 0, _p(ws), ws.numel(), stream())
    return out


def matmul_colsum(A, B, out=None, colsum=None):
    """(A^T B, column sums of B) for A [K, M], B [K, N]: the weight and bias gradients of a MatBias layer from one pass over
    the incoming gradient (hb_matmul_colsum)."""
    _chk(A), _chk(B)
    K, M = A.shape[-2], A.shape[-1]
    N = B.shape[-1]
    _require(A.dim() == 2 and B.dim() == 2 and B.shape[0] == K, "matmul_colsum", "A [K, M] and B [K, N] expected")
    if out is None:
        out = _empty((M, N), dtype=A.dtype, device=A.device)
    if colsum is None:
        colsum = _empty((N,), dtype=A.dtype, device=A.device)
    _require(colsum.numel() == N and colsum.is_contiguous(), "matmul_colsum", "colsum must be contiguous [N]")
    ws = workspace(A.dtype, A.device, 1 << 22)
    _lib.lib().call("hb_matmul_colsum" + _suf(A), _p(A), _p(B), _p(out), _p(colsum), M, N, K, M, N, N, _p(ws), ws.numel(),
                    stream())
    return out, colsum




def mlp2_sample_supported(n, din, hid, nout, rng_lanes=0, has_u=True):
    return bool(_query("hb_mlp2_sample_supported", n, din, hid, nout, rng_lanes, bool(has_u)))


def mlp2_sample_ws_elems(n, din, hid):
    return _query("hb_mlp2_sample_ws_elems", n, din, hid)


def mlp2_sample_ws(n, din, hid, device):   # (for callers that keep a workspace of their own; the wrappers' default is the shared scratch)
    return _empty(mlp2_sample_ws_elems(n, din, hid), dtype=torch.float32, device=device)


def mlp2_sample_fwd(y, w0, b0, w1, b1, act, u_in=None, rng=None, out=None, ws=None):
    """(x, kl, u, o) of the fused two-layer encoder + LOCAL diagonal sample + MC-KL (hb_mlp2_sample_fwd_f32)."""
    who = "mlp2_sample_fwd"
    _operands(who, y, w0, b0, w1, b1, u_in)
    n, din = y.shape
    hid = w0.shape[1]
    x, kl, u, o = _outs(who, out, ((n, 16), (1,), (n, 16), (n, 32)), y.dtype, y.device, ("x", "kl", "u", "o"))
    ws = _ws(who, ws, torch.float32, y.device, mlp2_sample_ws_elems(n, din, hid), "mlp2_sample_ws_elems")
    _lib.lib().call("hb_mlp2_sample_fwd_f32", _p(y), _p(w0), _p(b0), _p(w1), _p(b1), ACT[act], _p(u_in),
                    _p(rng.state) if (rng is not None and u_in is None) else None, rng.nlanes if rng is not None else 0,
                    _p(x), _p(kl), _p(u), _p(o), n, din, hid, _p(ws), stream())
    return x, kl, u, o


def mlp2_sample_bwd(y, w0, b0, w1, act, o, u, x, xbar, klbar, out=None, ws=None):
    """(dw0, db0, dw1, db1) of the fused encoder + sampler (hb_mlp2_sample_bwd_f32): h recomputed from y."""
    who = "mlp2_sample_bwd"
    _operands(who, y, w0, b0, w1, o, u, x, xbar, klbar)
    n, din = y.shape
    hid = w0.shape[1]
    dw0, db0, dw1, db1 = _outs(who, out, (tuple(w0.shape), (hid,), tuple(w1.shape), (32,)), y.dtype, y.device,
                               ("dw0", "db0", "dw1", "db1"))
    ws = _ws(who, ws, torch.float32, y.device, mlp2_sample_ws_elems(n, din, hid), "mlp2_sample_ws_elems")
    _lib.lib().call("hb_mlp2_sample_bwd_f32", _p(y), _p(w0), _p(b0), _p(w1), ACT[act], _p(o), _p(u), _p(x), _p(xbar), _p(klbar),
                    _p(dw0), _p(db0), _p(dw1), _p(db1), n, din, hid, _p(ws), stream())
    return dw0, db0, dw1, db1


def cholesky(A, out=None, info=None):
    """L = chol(A) (lower), batched over leading dims.  Returns (L, info[B] int32 device tensor)."""
    _chk(A)
    M = A.shape[-1]
    _require(A.dim() >= 2 and A.shape[-2] == M, "cholesky", "square matrices [..., M, M] expected")
    B = A.numel() // max(M * M, 1)
    out = _out("cholesky", out, tuple(A.shape), A.dtype, A.device, exact=False)
    if info is None:
        info = _empty(max(B, 1), dtype=torch.int32, device=A.device)
    if out.data_ptr() == A.data_ptr() and A.numel():
        # the C entry point forbids aliasing; in-place requests go through a copy (eager use only)
        tmp = _empty_like(A)
        _lib.lib().call("hb_cholesky" + _suf(A), _p(A), _p(tmp), B, M, _p(info), stream())
        ewise("COPY", [tmp], out=out)
        return out, info
    _lib.lib().call("hb_cholesky" + _suf(A), _p(A), _p(out), B, M, _p(info), stream())
    return out, info



_chol_ws_cache = {}


def debug_set(key, value):
    """Diagnostic switch of the native library (hb_debug_set, include/henbun_hip.h): tests and tools only."""
    _lib.lib().call("hb_debug_set", key.encode(), int(value))


def debug_clear():
    _lib.lib().call("hb_debug_clear")


def cholesky_ws_elems(B, M, dtype):
    return _query("hb_cholesky_inverse_ws_elems", B, M, _elem_bytes(dtype))


def cholesky_workspace(dtype, device, B, M):
    """ZERO-FILLED workspace of hb_cholesky_inverse for (B, M) on the current stream: the persistent launch keeps its
    sync words there and leaves them zero after every call (include/henbun_hip.h, workspace contract)."""
    key = (dtype, str(device), torch.cuda.current_stream().cuda_stream, B, M)
    w = _chol_ws_cache.get(key)
    if w is None:
        w = torch.zeros(max(cholesky_ws_elems(B, M, dtype), 1), dtype=dtype, device=device)
        _chol_ws_cache[key] = w
    return w


def cholesky_inverse(A, out=None, inv=None, info=None, ws=None, frag=None, frag_bf16x3=False):
    """(L, W, info): L = chol(A) and W = L^-1 from one fused launch sequence (batched over leading dims).
    `frag` (2*B*M*M elements, M % 32 == 0): receives the fragment-major copies of W and W^T (see the header)."""
    who = "cholesky_inverse"
    _chk(A)
    M = A.shape[-1]
    _require(A.dim() >= 2 and A.shape[-2] == M, who, "square matrices [..., M, M] expected")
    B = A.numel() // max(M * M, 1)
    out, inv = _outs(who, (out, inv), (tuple(A.shape),) * 2, A.dtype, A.device, ("out", "inv"))
    if info is None:
        info = _empty(max(B, 1), dtype=torch.int32, device=A.device)
    ws, frag = _cholesky_scratch(who, ws, frag, frag_bf16x3, A.dtype, A.device, B, M)
    _lib.lib().call("hb_cholesky_inverse" + _suf(A), _p(A), _p(out), _p(inv), B, M, _p(info), _p(ws), _p(frag),
                    int(bool(frag_bf16x3 and frag is not None)), stream())
    return out, inv, info


def cholesky_frag_elems(B, M, bf16x3=False):
    """Elements of cholesky_inverse's `frag` buffer: the images of W and W^T, and the bf16x3 planes behind them if asked for."""
    return _query("hb_cholesky_frag_elems", B, M, bool(bf16x3))


def _cholesky_scratch(who, ws, frag, bf16x3, dtype, device, B, M):
    """(ws, frag) of cholesky_inverse / gram_cholesky_inverse, checked.  The default workspace is cholesky_workspace's,
    not the shared scratch: it must be zero-filled."""
    ws = _ws(who, cholesky_workspace(dtype, device, B, M) if ws is None else ws, dtype, device,
             cholesky_ws_elems(B, M, dtype), "cholesky_ws_elems")
    if frag is not None:
        _require(M % 32 == 0, who, "frag needs M %% 32 == 0, got M=%d" % M)
        _ws(who, frag, dtype, device, cholesky_frag_elems(B, M, bf16x3), "cholesky_frag_elems", "frag")
    return ws, frag


def cholesky_persistent_shape(B, M, dtype):
    """hb_cholesky_inverse takes its one-launch persistent form for this (B, M, dtype)."""
    return bool(_query("hb_cholesky_persistent_shape", B, M, _elem_bytes(dtype)))


def gram_cholesky_inverse(X, ell, diag_add, kind=KERN_RBF, out=None, inv=None, info=None, ws=None, frag=None, frag_bf16x3=False):
    """(L, W, info) of K(X, X) + diag_add I without K being written: hb_gram_cholesky_inverse_f32 (the persistent
    Cholesky synthesises its tiles from the points).  X: [M, d] or [B, M, d]; ell as in gram_fwd."""
    _chk(X), _chk(ell)
    _require(X.dtype == torch.float32, "gram_cholesky_inverse", "float32 operands expected")
    BX, M, d = _batch_view(X)
    B = BX
    if ell.dim() >= 2 and ell.shape[0] > 1:
        B = max(B, ell.shape[0])
    _require(BX in (1, B), "gram_cholesky_inverse", "batch extents must match or be absent")
    sX = M * d if (BX == B and B > 1) else 0
    sEll, dl = _ell_layout(ell, B, d)
    batched = X.dim() > 2 or sEll != 0
    shape = ((B,) if batched else ()) + (M, M)
    out, inv = _outs("gram_cholesky_inverse", (out, inv), (shape,) * 2, X.dtype, X.device, ("out", "inv"), exact=False)
    if info is None:
        info = _empty(max(B, 1), dtype=torch.int32, device=X.device)
    ws, frag = _cholesky_scratch("gram_cholesky_inverse", ws, frag, frag_bf16x3, X.dtype, X.device, B, M)
    _lib.lib().call("hb_gram_cholesky_inverse_f32", kind, _p(X), sX, _p(ell), sEll, dl, d, float(diag_add), _p(out), _p(inv), B, M,
                    _p(info), _p(ws), _p(frag), int(bool(frag_bf16x3 and frag is not None)), stream())
    return out, inv, info


def trinv(L, out=None):
    """W = L^{-1} for lower-triangular L, batched."""
    _chk(L)
    M = L.shape[-1]
    B = L.numel() // max(M * M, 1)
    out = _out("trinv", out, tuple(L.shape), L.dtype, L.device, exact=False)
    ws = workspace(L.dtype, L.device, max(B * M * M, 1))
    _lib.lib().call("hb_trinv" + _suf(L), _p(L), _p(out), B, M, _p(ws), stream())
    return out


# ---- K5/K6 fused sparse GP -----------------------------------------------------
def _sgp_dims(x, z, u):
    E = z.shape[0] if z.dim() == 3 else 1
    M, d = z.shape[-2], z.shape[-1]
    n = x.shape[-2]
    P = u.shape[-2]
    sx = n * d if (x.dim() == 3 and x.shape[0] == E and E > 1) else 0
    return E, n, M, d, P, sx


def sgp_strip_path(E, n, M, d, P, prec=PREC_NATIVE):
    """True when sgp_fwd / sgp_bwd (given wfrag) run in column-strip form and may exchange A / Kbar fragment-major."""
    return bool(_query("hb_sgp_strip_path", E, n, M, d, P, prec))


def sgp_frag_elems(E, n, M, prec=PREC_NATIVE):
    """fp32 elements of a fragment-major [E, M, n] operand buffer (columns padded to whole strips of 32); the bf16x3
    form holds three bf16 planes instead of one fp32 image: 1.5 times the bytes."""
    return _query("hb_sgp_frag_elems", E, n, M, prec)


def _sgp_fwd_query(name, x, z, u, prec, has_wfrag, draw, rng):
    """A query of the library about the sgp_fwd call with these operands (0 for anything but fp32)."""
    E, n, M, d, P, _ = _sgp_dims(x, z, u)
    if x.dtype != torch.float32:
        return 0
    return _query(name, E, n, M, d, P, prec, bool(has_wfrag), bool(draw), rng.nlanes if rng is not None else 0)


def sgp_head_units(x, z, u, prec, has_wfrag, draw, rng):
    """Number of partial-sum units hb_sgp_fwd_gauss leaves for this call (0: the likelihood head cannot ride in it)."""
    return _sgp_fwd_query("hb_sgp_head_units", x, z, u, prec, has_wfrag, draw, rng)


def matmul_gram_vjp_ok(M, K, batch, d, dtype):
    """The square product [batch, M, K] x [batch, K, M] can carry the Gram VJP of its result (hb_matmul_gram_vjp_ok)."""
    if dtype != torch.float32:
        return False
    return bool(_query("hb_matmul_gram_vjp_ok", M, K, batch, d))


def matmul_gram_vjp_ws_elems(batch, M, d):
    """Scratch elements of matmul_gram_vjp's `part` (hb_matmul_gram_vjp_ws_elems)."""
    return _query("hb_matmul_gram_vjp_ws_elems", batch, M, d)


def matmul_wgk_shape(M, N, K, batch):
    """The shape [batch, M, K] x [batch, K, N] lies inside hb_matmul_f32's in-workgroup split-K form (hb_matmul_wgk_shape:
    the shape part of the rule only -- alignment, flags and the mm_no_wgk switch are the call's own business)."""
    return bool(_query("hb_matmul_wgk_shape", M, N, K, batch))


MatmulForm = collections.namedtuple("MatmulForm", "form S vec finish bfast colsum_fused")


def matmul_form(dtype, batch, M, N, K, lda=None, ldb=None, ldc=None, sA=None, sB=None, transA=False, transB=False, beta=0.0,
                flags=0, a_aligned=True, b_aligned=True, ws_elems=1 << 22, colsum=False):
    """What hb_matmul_* (colsum: hb_matmul_colsum_*) launches for this call, asked on the host (hb_matmul_form: the
    launcher's own decision function; nothing runs): MatmulForm(form in MM_FORM, S slabs, vector operand path, finish
    launch, batch-fastest grid, fused column sums).  Strides default to contiguous operands; ws_elems to matmul()'s."""
    lda = (M if transA else K) if lda is None else lda
    ldb = (K if transB else N) if ldb is None else ldb
    ldc = N if ldc is None else ldc
    sA = (M * K if batch > 1 else 0) if sA is None else sA
    sB = (K * N if batch > 1 else 0) if sB is None else sB
    o = [ctypes.c_int(0) for _ in range(5)]
    form = _lib.lib().raw("hb_matmul_form")(_elem_bytes(dtype), int(batch), int(M), int(N), int(K), int(lda), int(ldb), int(ldc),
                                            int(sA), int(sB), int(bool(transA)), int(bool(transB)), float(beta), int(flags),
                                            int(bool(a_aligned)), int(bool(b_aligned)), int(ws_elems), int(bool(colsum)),
                                            *[ctypes.byref(v) for v in o])
    if form < 0:
        raise ValueError("matmul_form: an empty product, or arguments hb_matmul rejects")
    return MatmulForm(int(form), o[0].value, bool(o[1].value), bool(o[2].value), bool(o[3].value), bool(o[4].value))


def matmul_gram_vjp(a, b, out, transA, transB, X, sX, ell, sEll, dl, d, xbar, ell_partial, part, counters):
    """out = op(a) op(b) (batched square product) and, from the same launch, the one-pass symmetric Gram VJP of `out` as
    Kbar: xbar and the lengthscale row partials (hb_matmul_gram_vjp_f32)."""
    M = out.shape[-1]
    batch = out.numel() // (M * M)
    K = a.shape[-2] if transA else a.shape[-1]
    sA = a.stride(0) if a.dim() == 3 and a.shape[0] > 1 else 0
    sB = b.stride(0) if b.dim() == 3 and b.shape[0] > 1 else 0
    _lib.lib().call("hb_matmul_gram_vjp_f32", _p(a), _p(b), _p(out), batch, M, K, a.stride(-2), b.stride(-2), out.stride(-2),
                    sA, sB, M * M, int(bool(transA)), int(bool(transB)), _p(X), int(sX), _p(ell), int(sEll), int(dl), int(d),
                    _p(xbar), _p(ell_partial), _p(part), _p(counters), stream())


def gram_ell_fold(partial, rows, d, dl, groups, ellbar):
    """ellbar from the lengthscale row partials of a Gram VJP (hb_gram_ell_fold; chain-aware)."""
    _lib.lib().call("hb_gram_ell_fold" + _suf(partial), _p(partial), int(rows), int(d), int(dl), int(groups), _p(ellbar), stream())


def matmul_gram_vjp_tiles_ok(M, K, batch, d, dtype):
    """The square product can leave the tile partials of its result's Gram VJP for gram_tiles_fold
    (hb_matmul_gram_vjp_tiles_ok; hb_debug_set("gram_vjp_tiles", 0) answers no)."""
    if dtype != torch.float32:
        return False
    return bool(_query("hb_matmul_gram_vjp_tiles_ok", M, K, batch, d))


def matmul_gram_vjp_tiles(a, b, out, transA, transB, X, sX, ell, sEll, dl, d, part):
    """The tile partials `part` of the one-pass symmetric Gram VJP of op(a) op(b) as Kbar, from the product's own launch
    (hb_matmul_gram_vjp_tiles_f32).  out: the product itself, or None when nothing else reads it."""
    M = a.shape[-1] if transA else a.shape[-2]
    K = a.shape[-2] if transA else a.shape[-1]
    batch = a.numel() // (M * K) if a.dim() == 3 else (b.numel() // (M * K) if b.dim() == 3 else 1)
    sA = a.stride(0) if a.dim() == 3 and a.shape[0] > 1 else 0
    sB = b.stride(0) if b.dim() == 3 and b.shape[0] > 1 else 0
    _lib.lib().call("hb_matmul_gram_vjp_tiles_f32", _p(a), _p(b), _p(out) if out is not None else None, batch, M, K, a.stride(-2),
                    b.stride(-2), out.stride(-2) if out is not None else M, sA, sB, M * M, int(bool(transA)), int(bool(transB)),
                    _p(X), int(sX), _p(ell), int(sEll), int(dl), int(d), _p(part), stream())


def gram_tiles_fold(part, batch, M, d, dl, xbar, ellbar):
    """xbar and ellbar from the tile partials of matmul_gram_vjp_tiles (hb_gram_tiles_fold_f32; chain-aware)."""
    _lib.lib().call("hb_gram_tiles_fold_f32", _p(part), int(batch), int(M), int(d), int(dl), _p(xbar), _p(ellbar), stream())


def matmul_gauss_units(n, K, N, dtype):
    """Partial-sum units of hb_matmul_gauss for an [n, K] x [K, N] MatBias layer feeding a Gaussian head (0: not this shape)."""
    if dtype != torch.float32:
        return 0
    return _query("hb_matmul_gauss_units", n, K, N)


def matmul_gauss(x, w, bias, head):
    """The Gaussian likelihood head of x @ w + bias in the product's own launch (hb_matmul_gauss_f32): head = dict(y, scale,
    var, post, dmu, fbar, part, units); writes head['dmu'] (and head['fbar']) and the partial sums head['part']."""
    for t in (x, w):
        _chk(t)
    n, K = x.shape
    N = w.shape[1]
    _lib.lib().call("hb_matmul_gauss_f32", _p(x), x.stride(0), _p(w), w.stride(0), _p(bias), _p(head["y"]), _p(head.get("scale")),
                    _p(head["var"]), float(head.get("post") or 0.0), _p(head["dmu"]), _p(head.get("fbar")), _p(head["part"]),
                    int(head["units"]), int(n), int(K), int(N), stream())


def sgp_rider_supported(x, z, u, prec, has_wfrag, draw, rng):
    """1 when this forward call can be recorded (sgp_rider_begin) and start inside the launch of the persistent
    factorisation that produces its W (hb_sgp_rider_supported)."""
    return bool(_sgp_fwd_query("hb_sgp_rider_supported", x, z, u, prec, has_wfrag, draw, rng))


def sgp_rider_begin():
    """The next sgp_fwd call of this thread is recorded instead of launched; the next cholesky_inverse /
    gram_cholesky_inverse launches it inside its own grid (include/henbun_hip.h: early-start forward)."""
    _lib.lib().call("hb_sgp_rider_begin")


def sgp_rider_flush():
    """Launch a recorded forward that no factorisation picked up (a no-op otherwise)."""
    _lib.lib().call("hb_sgp_rider_flush", stream())


def sgp_rider_pending():
    return _query("hb_sgp_rider_pending")


def gauss_ll_fold(part, nb, ll, ds, dv):
    """(ll, dscale, dvar) from the partial sums part[3][nb] of a head whose per-point part ran elsewhere (hb_gauss_ll_fold)."""
    _lib.lib().call("hb_gauss_ll_fold" + _suf(part), _p(part), int(nb), _p(ll), _p(ds), _p(dv), stream())


def sgp_fwd(x, z, ell, W, u, eps_in=None, rng=None, mode=SGP_DIAGONAL, out=None, wfrag=None, prec=PREC_NATIVE,
            a_frag=None, skip_a=False, head=None):
    """Returns (f[E?,P,n], A[E?,M,n], v[E?,n], eps[E?,n]).  `wfrag`: cholesky_inverse's fragment-major copies of W.
    `head`: dict(y, scale, var, post, dmu, fbar, part, units) -- the Gaussian likelihood head's per-point part in the same
    launch (hb_sgp_fwd_gauss; units = sgp_head_units(...) > 0)."""
    for t in (x, z, ell, W, u):
        _chk(t)
    E, n, M, d, P, sx = _sgp_dims(x, z, u)
    lead = (E,) if z.dim() == 3 else ()
    dev, dt = x.device, x.dtype
    if out is None:
        f = _empty(lead + (P, n), dtype=dt, device=dev)
        A = _empty(lead + (M, n), dtype=dt, device=dev)
        v = _empty(lead + (n,), dtype=dt, device=dev)
        eps = _empty(lead + (n,), dtype=dt, device=dev)
    else:
        f, A, v, eps = out
    dl = ell.numel() // E
    rp, rl = _rng_args(rng)
    ws = workspace(dt, dev, sgp_ws_elems(E, n, M, d, P))
    # a_frag: also (skip_a: only) leave A fragment-major for sgp_bwd (column-strip form, see the header)
    if head is not None:
        _lib.lib().call("hb_sgp_fwd_gauss_f32", KERN_RBF, mode, _p(x), sx, _p(z), _p(ell), dl, _p(W), _p(wfrag), int(prec), _p(u),
                        _p(eps_in), rp, rl, _p(eps), None if (skip_a and a_frag is not None) else _p(A), _p(a_frag), _p(f), _p(v),
                        E, n, M, d, P, _p(ws), _p(head["y"]), _p(head.get("scale")), _p(head["var"]), float(head.get("post") or 0.0),
                        _p(head["dmu"]), _p(head.get("fbar")), _p(head["part"]), int(head["units"]), stream())
        return f, A, v, eps
    _lib.lib().call("hb_sgp_fwd" + _suf(x), KERN_RBF, mode, _p(x), sx, _p(z), _p(ell), dl, _p(W), _p(wfrag), int(prec), _p(u), _p(eps_in),
                    rp, rl, _p(eps), None if (skip_a and a_frag is not None) else _p(A), _p(a_frag), _p(f), _p(v), E, n,
                    M, d, P, _p(ws), stream())
    return f, A, v, eps


def sgp_ws_elems(E, n, M, d, P):
    """Workspace elements of sgp_fwd / sgp_bwd for this shape (hb_sgp_ws_elems)."""
    return _query("hb_sgp_ws_elems", E, n, M, d, P)


def sgp_fwd_kbar_supported(x, z, u, prec, has_wfrag, draw, rng):
    """True when sgp_fwd_gauss_kbar serves this forward call (hb_sgp_fwd_kbar_supported: the head rides in it, its backward is
    Phi-direct, d <= 2, at most 512 strips, and the diagnostic switch sgp_fwd_kbar is not 0).  The planner asks when it
    builds a plan."""
    return bool(_sgp_fwd_query("hb_sgp_fwd_kbar_supported", x, z, u, prec, has_wfrag, draw, rng))


def sgp_fwd_gauss_kbar(x, z, ell, W, u, wfrag, a_frag, abar_frag, bws, head, eps_in=None, rng=None, mode=SGP_DIAGONAL, out=None):
    """sgp_fwd with the Gaussian head (head['fbar'] required) and the backward's Kbar strips in ONE launch
    (hb_sgp_fwd_gauss_kbar_f32): besides sgp_fwd's results it leaves Abar fragment-major in abar_frag and the backward's
    strip partials in bws (hb_sgp_ws_elems elements, the caller's own until sgp_bwd_phi_rest has run).  A is exchanged
    fragment-major only.  Returns (f, v, eps)."""
    for t in (x, z, ell, W, u):
        _chk(t)
    E, n, M, d, P, sx = _sgp_dims(x, z, u)
    lead = (E,) if z.dim() == 3 else ()
    dev, dt = x.device, x.dtype
    who = "sgp_fwd_gauss_kbar"
    _require(dt == torch.float32 and all(t is not None for t in (wfrag, a_frag, abar_frag, bws, head.get("fbar"))), who,
             "float32 operands, wfrag, a_frag, abar_frag, bws and head['fbar'] expected")
    if out is None:
        f = _empty(lead + (P, n), dtype=dt, device=dev)
        v = _empty(lead + (n,), dtype=dt, device=dev)
        eps = _empty(lead + (n,), dtype=dt, device=dev)
    else:
        f, v, eps = out
    dl = ell.numel() // E
    rp, rl = _rng_args(rng)
    wse = sgp_ws_elems(E, n, M, d, P)
    _ws(who, bws, dt, dev, wse, "sgp_ws_elems", "bws")   # (the caller's own buffers, sized like workspaces)
    _ws(who, abar_frag, dt, dev, sgp_frag_elems(E, n, M), "sgp_frag_elems", "abar_frag")
    ws = workspace(dt, dev, wse)
    _lib.lib().call("hb_sgp_fwd_gauss_kbar_f32", KERN_RBF, mode, _p(x), sx, _p(z), _p(ell), dl, _p(W), _p(wfrag), int(PREC_NATIVE),
                    _p(u), _p(eps_in), rp, rl, _p(eps), None, _p(a_frag), _p(f), _p(v), E, n, M, d, P, _p(ws), _p(head["y"]),
                    _p(head.get("scale")), _p(head["var"]), float(head.get("post") or 0.0), _p(head["dmu"]), _p(head["fbar"]),
                    _p(head["part"]), int(head["units"]), _p(abar_frag), _p(bws), stream())
    return f, v, eps


def sgp_bwd_phi_rest(a_frag, abar_frag, bws, dims, dl, out):
    """The part of sgp_bwd_phi behind its strip kernel (hb_sgp_bwd_phi_rest_f32), on what sgp_fwd_gauss_kbar left: the
    Abar A^T contraction and the finish launch.  dims = (E, n, M, d, P); out = (Phi, ubar, zbar, ellbar), returned."""
    E, n, M, d, P = (int(t) for t in dims)
    Phi, ubar, zbar, ellbar = out
    _require(Phi.dtype == torch.float32, "sgp_bwd_phi_rest", "float32 operands expected")
    _lib.lib().call("hb_sgp_bwd_phi_rest_f32", _p(a_frag), _p(abar_frag), _p(Phi), _p(ubar), _p(zbar), _p(ellbar), int(dl), E, n, M, d,
                    P, _p(bws), stream())
    return Phi, ubar, zbar, ellbar


def sgp_A(x, z, ell, W, out=None, wfrag=None, prec=PREC_NATIVE):
    """A = W K(z,x): the M^2 n contraction alone (hb_sgp_A)."""
    E = z.shape[0] if z.dim() == 3 else 1
    M, d = z.shape[-2], z.shape[-1]
    n = x.shape[-2]
    sx = n * d if (x.dim() == 3 and x.shape[0] == E and E > 1) else 0
    if out is None:
        out = _empty(((E,) if z.dim() == 3 else ()) + (M, n), dtype=x.dtype, device=x.device)
    _lib.lib().call("hb_sgp_A" + _suf(x), KERN_RBF, _p(x), sx, _p(z), _p(ell), ell.numel() // E, _p(W), _p(wfrag), int(prec),
                    _p(out), E, n, M, d, stream())
    return out


def sgp_predict_fused(dtype, E, n, M, d, P, s_kind, has_wfrag):
    """True when hb_sgp_predict runs its fused streaming kernel for these extents (hb_sgp_predict_fused); everything else
    runs in column chunks."""
    return bool(_query("hb_sgp_predict_fused", E, n, M, d, P, s_kind, bool(has_wfrag), _elem_bytes(dtype)))


def sgp_predict_ws_elems(dtype, E, n, M, d, P, s_kind, has_wfrag):
    """Scratch elements hb_sgp_predict needs (bounded by one column chunk, not by n)."""
    return _query("hb_sgp_predict_ws_elems", E, n, M, d, P, s_kind, bool(has_wfrag), _elem_bytes(dtype))


def sgp_predict(x, z, ell, W, m, s, s_kind=SGP_S_DIAG, mode=SGP_DIAGONAL, jitter=0.0, out=None, wfrag=None, ws=None):
    """Closed-form predictive moments (mean[E?,P,n], var[E?,P,n]) of sgp_fwd's draw for u ~ N(m, S S^T) (hb_sgp_predict).
    m [E?, P, M]; s: standard deviations [E?, P, M] (SGP_S_DIAG) or ONE lower-triangular [R, R], R = E P M (SGP_S_TRIL).
    `wfrag`: cholesky_inverse's fragment-major images of W (the fused form needs them; None: chunked form)."""
    who = "sgp_predict"
    _operands(who, x, z, ell, W, m, s, wfrag)
    E, n, M, d, P, sx = _sgp_dims(x, z, m)
    lead = (E,) if z.dim() == 3 else ()
    dev, dt = x.device, x.dtype
    mean, var = _outs(who, out, (lead + (P, n),) * 2, dt, dev, ("mean", "var"))
    ws = _ws(who, ws, dt, dev, sgp_predict_ws_elems(dt, E, n, M, d, P, s_kind, wfrag is not None), "sgp_predict_ws_elems")
    _lib.lib().call("hb_sgp_predict" + _suf(x), KERN_RBF, _p(x), sx, _p(z), _p(ell), ell.numel() // E, _p(W), _p(wfrag), _p(m),
                    _p(s), int(s_kind), int(mode), float(jitter), _p(mean), _p(var), E, n, M, d, P, _p(ws), stream())
    return mean, var


def sgp_predict_multi_fused(dtype, n, M, d, C, has_wfrag):
    """True when hb_sgp_predict_multi runs its fused strip kernel for these extents (hb_sgp_predict_multi_fused);
    everything else runs the chunked form once per latent function."""
    return bool(_query("hb_sgp_predict_multi_fused", n, M, d, C, bool(has_wfrag), _elem_bytes(dtype)))


def sgp_predict_multi_ws_elems(dtype, n, M, d, C, has_wfrag):
    """Scratch elements hb_sgp_predict_multi needs: C M^2 (the S^T images of the fused form), or one chunk."""
    return _query("hb_sgp_predict_multi_ws_elems", n, M, d, C, bool(has_wfrag), _elem_bytes(dtype))


def sgp_predict_multi(x, z, ell, W, m, S, mode=SGP_DIAGONAL, out=None, wfrag=None, ws=None):
    """Closed-form predictive moments (mean [C, n], var [C, n]) of C latent functions of ONE expert with independent
    full-rank q(u_c) = N(m_c, S_c S_c^T) that share x [n, d], z [M, d], ell and W (hb_sgp_predict_multi): m [C, M], S [C, M, M]
    lower, 1 <= C <= 64; mode SGP_DIAGONAL or SGP_NEGLECTED.  The bits of C calls of sgp_predict(m[c:c+1], S[c],
    s_kind=SGP_S_TRIL) with the same `wfrag`; with it (float32, M % 32 == 0, M <= 512, d <= 4) A = W K(z, x) is formed once
    for all C in one strip kernel."""
    who = "sgp_predict_multi"
    _operands(who, x, z, ell, W, m, S, wfrag)
    if x.dim() != 2 or z.dim() != 2 or z.shape[1] != x.shape[1] or tuple(W.shape) != (z.shape[0], z.shape[0]):
        raise ValueError("%s: x [n, d], z [M, d], W [M, M] expected, got %s %s %s"
                         % (who, tuple(x.shape), tuple(z.shape), tuple(W.shape)))
    (n, d), M = x.shape, z.shape[0]
    if m.dim() != 2 or m.shape[1] != M or tuple(S.shape) != (m.shape[0], M, M) or ell.numel() not in (1, d):
        raise ValueError("%s: m [C, M], S [C, M, M] and 1 or d lengthscales expected, got %s %s %s"
                         % (who, tuple(m.shape), tuple(S.shape), tuple(ell.shape)))
    C = m.shape[0]
    if wfrag is not None and wfrag.numel() < 2 * M * M:
        raise ValueError("%s: wfrag must hold the two fragment-major images of W (2 M^2 elements)" % who)
    dev, dt = x.device, x.dtype
    mean, var = _outs(who, out, ((C, n),) * 2, dt, dev, ("mean", "var"))
    ws = _ws(who, ws, dt, dev, sgp_predict_multi_ws_elems(dt, n, M, d, C, wfrag is not None), "sgp_predict_multi_ws_elems")
    _lib.lib().call("hb_sgp_predict_multi" + _suf(x), KERN_RBF, _p(x), _p(z), _p(ell), ell.numel(), _p(W), _p(wfrag), _p(m),
                    _p(S), int(mode), _p(mean), _p(var), n, M, d, C, _p(ws), stream())
    return mean, var


def _predict_grad_shapes(who, x, z, ell, W, m, s, s_kind, wfrag):
    """(n, M, d) of the operands of sgp_predict_grad / sgp_acq, checked: on the device, contiguous, one expert and one
    latent function, shapes that fit, one dtype."""
    if x.dim() != 2 or z.dim() != 2 or z.shape[1] != x.shape[1] or tuple(W.shape) != (z.shape[0], z.shape[0]):
        raise ValueError("%s: x [n, d], z [M, d], W [M, M] expected, got %s %s %s"
                         % (who, tuple(x.shape), tuple(z.shape), tuple(W.shape)))
    (n, d), M = x.shape, z.shape[0]
    if m.numel() != M or ell.numel() not in (1, d):
        raise ValueError("%s: m [M] and 1 or d lengthscales expected, got %s %s" % (who, tuple(m.shape), tuple(ell.shape)))
    if s_kind not in (SGP_S_DIAG, SGP_S_TRIL) or s.numel() != (M if s_kind == SGP_S_DIAG else M * M):
        raise ValueError("%s: s must be [M] (SGP_S_DIAG) or [M, M] (SGP_S_TRIL), got %s" % (who, tuple(s.shape)))
    _operands(who, x, z, ell, W, m, s, wfrag)
    if wfrag is not None and wfrag.numel() < 2 * M * M:
        raise ValueError("%s: wfrag must hold the two fragment-major images of W (2 M^2 elements)" % who)
    return n, M, d


def sgp_predict_grad_ws_elems(dtype, n, M, d, s_kind, has_wfrag):
    """Scratch elements hb_sgp_predict_grad / hb_sgp_acq need (bounded by one column chunk, not by n)."""
    return _query("hb_sgp_predict_grad_ws_elems", n, M, d, s_kind, bool(has_wfrag), _elem_bytes(dtype))


def sgp_acq_ws_elems(dtype, n, M, d, s_kind, has_wfrag):
    """Scratch elements hb_sgp_acq needs (those of hb_sgp_predict_grad)."""
    return _query("hb_sgp_acq_ws_elems", n, M, d, s_kind, bool(has_wfrag), _elem_bytes(dtype))


def sgp_predict_grad(x, z, ell, W, m, s, s_kind=SGP_S_DIAG, mode=SGP_DIAGONAL, jitter=0.0, out=None, wfrag=None, ws=None,
                     values=True):
    """sgp_predict's moments and their input gradients for one expert and one latent function (hb_sgp_predict_grad):
    (mean [n], var [n], dmean [n, d], dvar [n, d]) with dmean[j, k] = d mean[j] / d x_jk.  x [n, d], z [M, d], ell [1] or
    [d], W [M, M], m [M] (any shape of M elements), s [M] standard deviations (SGP_S_DIAG) or [M, M] lower (SGP_S_TRIL).
    mean and var are the bits of sgp_predict; values=False: they are not stored, those of `out` (if given) are left
    untouched and None is returned in their place.  `out`: (mean, var, dmean, dvar) written in place.  A column's results
    do not depend on the other columns: two calls, or x in pieces, return the same bits."""
    who = "sgp_predict_grad"
    n, M, d = _predict_grad_shapes(who, x, z, ell, W, m, s, s_kind, wfrag)
    o = (None,) * 4 if out is None else tuple(out)
    dt, dev = x.dtype, x.device
    mean = _out(who, o[0], (n,), dt, dev, "mean") if values else None
    var = _out(who, o[1], (n,), dt, dev, "var") if values else None
    dmean = _out(who, o[2], (n, d), dt, dev, "dmean")
    dvar = _out(who, o[3], (n, d), dt, dev, "dvar")
    ws = _ws(who, ws, dt, dev, sgp_predict_grad_ws_elems(dt, n, M, d, s_kind, wfrag is not None), "sgp_predict_grad_ws_elems")
    _lib.lib().call("hb_sgp_predict_grad" + _suf(x), KERN_RBF, _p(x), _p(z), _p(ell), ell.numel(), _p(W), _p(wfrag), _p(m), _p(s),
                    int(s_kind), int(mode), float(jitter), _p(mean), _p(var), _p(dmean), _p(dvar), n, M, d, _p(ws), stream())
    return mean, var, dmean, dvar


def sgp_acq(x, z, ell, W, m, s, acq, best=0.0, param=0.0, scale=1.0, largest=True, var_floor=0.0, s_kind=SGP_S_DIAG,
            mode=SGP_DIAGONAL, jitter=0.0, wfrag=None, ws=None, value=True, grad=False, argmax=False):
    """A closed-form acquisition function of the model f = scale * (sgp_predict's latent) at the rows of x (hb_sgp_acq):
    acq 'ei' / 'pi' (param = xi, improvement over `best`) or 'ucb' (param = beta), for maximising (largest) or minimising
    f; the tail is evaluated per point in double.  Returns (val [n], grad [n, d], best_val [1], best_idx int64 [1]) device
    tensors, None for each output not asked for (value / grad / argmax); with argmax alone nothing of size n is written.
    best_val = max_j val[j], those bits, best_idx its first row; a NaN is never chosen, no comparable value: -1 and -inf.
    Model operands as for sgp_predict_grad."""
    who = "sgp_acq"
    n, M, d = _predict_grad_shapes(who, x, z, ell, W, m, s, s_kind, wfrag)
    code = _code(who, ACQ, acq)
    if not (value or grad or argmax):
        raise ValueError("%s: at least one of value, grad, argmax expected" % who)
    if argmax and n < 1:
        raise ValueError("%s: at least one candidate expected, got x %s" % (who, tuple(x.shape)))
    val = _empty((n,), dtype=x.dtype, device=x.device) if value else None
    g = _empty((n, d), dtype=x.dtype, device=x.device) if grad else None
    bv = _empty((1,), dtype=x.dtype, device=x.device) if argmax else None
    bi = _empty((1,), dtype=torch.int64, device=x.device) if argmax else None
    ws = _ws(who, ws, x.dtype, x.device, sgp_acq_ws_elems(x.dtype, n, M, d, s_kind, wfrag is not None), "sgp_acq_ws_elems")
    _lib.lib().call("hb_sgp_acq" + _suf(x), KERN_RBF, _p(x), _p(z), _p(ell), ell.numel(), _p(W), _p(wfrag), _p(m), _p(s),
                    int(s_kind), int(mode), float(jitter), int(code), float(best), float(param), float(scale),
                    1 if largest else 0, float(var_floor), _p(val), _p(g), _p(bv), _p(bi), n, M, d, _p(ws), stream())
    return val, g, bv, bi


def sgp_predict_cov_ws_elems(dtype, E, n, M, P, s_kind):
    """Scratch elements hb_sgp_predict_cov needs: A [E, M, n], C = S^T A [M, n] (full-rank S), a2 [E, n] -- linear in n."""
    return _query("hb_sgp_predict_cov_ws_elems", E, n, M, P, s_kind, _elem_bytes(dtype))


def sgp_predict_cov(x, z, ell, W, s, P, s_kind=SGP_S_DIAG, mode=SGP_DIAGONAL, jitter=0.0, out=None, wfrag=None, ws=None):
    """Full predictive covariance cov[E?, P, n, n] of sgp_fwd's draw for u ~ N(m, S S^T) (hb_sgp_predict_cov): bitwise
    symmetric, its diagonal the var of sgp_predict.  s: standard deviations [E?, P, M] (SGP_S_DIAG) or one lower-triangular
    [M, M] for E P == 1 (SGP_S_TRIL).  `wfrag`: cholesky_inverse's fragment-major images of W (optional)."""
    who = "sgp_predict_cov"
    _operands(who, x, z, ell, W, s, wfrag)
    E, n, M, d, _, sx = _sgp_dims(x, z, s if s_kind == SGP_S_DIAG else z)
    lead = (E,) if z.dim() == 3 else ()
    dev, dt = x.device, x.dtype
    out = _out(who, out, lead + (int(P), n, n), dt, dev)
    ws = _ws(who, ws, dt, dev, sgp_predict_cov_ws_elems(dt, E, n, M, P, s_kind), "sgp_predict_cov_ws_elems")
    _lib.lib().call("hb_sgp_predict_cov" + _suf(x), KERN_RBF, _p(x), sx, _p(z), _p(ell), ell.numel() // E, _p(W), _p(wfrag),
                    _p(s), int(s_kind), int(mode), float(jitter), _p(out), E, n, M, d, int(P), _p(ws), stream())
    return out


def sgp_stats_ws_elems(dtype, N, M, d, P):
    """Scratch elements hb_sgp_stats needs: one column chunk of A plus the K-split partial tiles -- the same for every
    N above one chunk."""
    return _query("hb_sgp_stats_ws_elems", N, M, d, P, _elem_bytes(dtype))


def sgp_stats(X, Y, z, ell, W, wfrag=None, ws=None):
    """Sufficient statistics of the whole data set for the closed-form optimal q(u) (hb_sgp_stats): with
    A = W K(z, X) [M, N], (Phi = A A^T [M, M], b = (A Y)^T [P, M], yy = sum_j Y_jp^2 [P], a2sum = tr Phi [1]) as FLOAT64
    device tensors whatever the input dtype.  X [N, d], Y [N, P], z [M, d], ell [dl], W [M, M]; one expert.  Phi is
    bitwise symmetric; two calls on the same inputs return the same bits.  `wfrag`: cholesky_inverse's fragment-major
    images of W (optional)."""
    if X.dim() != 2 or Y.dim() != 2 or z.dim() != 2 or X.shape[0] != Y.shape[0] or X.shape[1] != z.shape[1]:
        raise ValueError("sgp_stats: X [N, d], Y [N, P], z [M, d] expected, got %s %s %s"
                         % (tuple(X.shape), tuple(Y.shape), tuple(z.shape)))
    dt, dev = X.dtype, X.device
    _operands("sgp_stats", X, Y, z, ell, W, wfrag)
    N, d = X.shape
    M, P = z.shape[0], Y.shape[1]
    Phi = _empty((M, M), dtype=torch.float64, device=dev)
    b = _empty((P, M), dtype=torch.float64, device=dev)
    yy = _empty((P,), dtype=torch.float64, device=dev)
    a2sum = _empty((1,), dtype=torch.float64, device=dev)
    ws = _ws("sgp_stats", ws, dt, dev, sgp_stats_ws_elems(dt, N, M, d, P), "sgp_stats_ws_elems")
    _lib.lib().call("hb_sgp_stats" + _suf(X), KERN_RBF, _p(X), _p(Y), _p(z), _p(ell), ell.numel(), _p(W), _p(wfrag), _p(Phi),
                    _p(b), _p(yy), _p(a2sum), N, M, d, P, _p(ws), stream())
    return Phi, b, yy, a2sum


def sgp_psi_stats_ws_elems(dtype, N, M, d, P):
    """Scratch elements hb_sgp_psi_stats needs: the partial tiles of the splits of N -- the same for every N >= 1."""
    return _query("hb_sgp_psi_stats_ws_elems", N, M, d, P, _elem_bytes(dtype))


def sgp_psi_stats(Xmean, Xvar, Y, z, ell, ws=None):
    """Psi statistics of a data set with Gaussian inputs x_n ~ N(Xmean_n, diag(Xvar_n)) for the unit RBF kernel
    (hb_sgp_psi_stats): (Psi2 [M, M] = sum_n E k(z, x_n) k(x_n, z), C [P, M] = (E K(z, X) Y)^T, yy [P] = sum_n Y_np^2) as
    FLOAT64 device tensors, evaluated in double whatever the input dtype.  Xmean, Xvar [N, d] (Xvar >= 0, zeros included:
    the caller's duty), Y [N, P], z [M, d], ell [dl].  Psi2 is bitwise symmetric; two calls return the same bits.  Cost:
    N M (M + 1) / 2 double exponentials."""
    if (Xmean.dim() != 2 or Y.dim() != 2 or z.dim() != 2 or Xvar.shape != Xmean.shape or Xmean.shape[0] != Y.shape[0]
            or Xmean.shape[1] != z.shape[1]):
        raise ValueError("sgp_psi_stats: Xmean [N, d], Xvar [N, d], Y [N, P], z [M, d] expected, got %s %s %s %s"
                         % (tuple(Xmean.shape), tuple(Xvar.shape), tuple(Y.shape), tuple(z.shape)))
    dt, dev = Xmean.dtype, Xmean.device
    _operands("sgp_psi_stats", Xmean, Xvar, Y, z, ell)
    N, d = Xmean.shape
    M, P = z.shape[0], Y.shape[1]
    Psi2 = _empty((M, M), dtype=torch.float64, device=dev)
    C = _empty((P, M), dtype=torch.float64, device=dev)
    yy = _empty((P,), dtype=torch.float64, device=dev)
    ws = _ws("sgp_psi_stats", ws, dt, dev, sgp_psi_stats_ws_elems(dt, N, M, d, P), "sgp_psi_stats_ws_elems")
    _lib.lib().call("hb_sgp_psi_stats" + _suf(Xmean), KERN_RBF, _p(Xmean), _p(Xvar), _p(Y), _p(z), _p(ell), ell.numel(),
                    _p(Psi2), _p(C), _p(yy), N, M, d, P, _p(ws), stream())
    return Psi2, C, yy


def sgp_psi_predict_ws_elems(dtype, n, M, d):
    """Scratch elements hb_sgp_psi_predict needs: two partial sums per point and workgroup of the point."""
    return _query("hb_sgp_psi_predict_ws_elems", n, M, d, _elem_bytes(dtype))


def sgp_psi_predict(Xmean, Xvar, z, ell, beta, Q, ws=None):
    """(e1 [n], e2 [n]) as FLOAT64 device tensors (hb_sgp_psi_predict): e1_j = sum_m beta_m psi1_j(m), e2_j = sum_mm'
    Q_mm' psi2_j(m, m') at Gaussian inputs N(Xmean_j, diag(Xvar_j)).  Xmean, Xvar [n, d], z [M, d], ell [dl] in one dtype;
    beta [M] and Q [M, M] float64, Q symmetric (its lower triangle is read).  A point's result does not depend on the
    other points of the call, bit for bit."""
    if Xmean.dim() != 2 or z.dim() != 2 or Xvar.shape != Xmean.shape or Xmean.shape[1] != z.shape[1]:
        raise ValueError("sgp_psi_predict: Xmean [n, d], Xvar [n, d], z [M, d] expected, got %s %s %s"
                         % (tuple(Xmean.shape), tuple(Xvar.shape), tuple(z.shape)))
    dt, dev = Xmean.dtype, Xmean.device
    _operands("sgp_psi_predict", Xmean, Xvar, z, ell)
    _operands("sgp_psi_predict", torch.float64, beta, Q, what="beta and Q must be float64")
    n, d = Xmean.shape
    M = z.shape[0]
    _require(beta.numel() == M and tuple(Q.shape) == (M, M), "sgp_psi_predict",
             "beta [%d] and Q [%d, %d] expected, got %s %s" % (M, M, M, tuple(beta.shape), tuple(Q.shape)))
    e1 = _empty((n,), dtype=torch.float64, device=dev)
    e2 = _empty((n,), dtype=torch.float64, device=dev)
    ws = _ws("sgp_psi_predict", ws, dt, dev, sgp_psi_predict_ws_elems(dt, n, M, d), "sgp_psi_predict_ws_elems")
    _lib.lib().call("hb_sgp_psi_predict" + _suf(Xmean), KERN_RBF, _p(Xmean), _p(Xvar), _p(z), _p(ell), ell.numel(), _p(beta),
                    _p(Q), _p(e1), _p(e2), n, M, d, _p(ws), stream())
    return e1, e2


def sgp_psi_grad_ws_elems(dtype, N, M, d, P):
    """Scratch elements hb_sgp_psi_grad needs: the partials of its two passes -- the same for every N >= 1."""
    return _query("hb_sgp_psi_grad_ws_elems", N, M, d, P, _elem_bytes(dtype))


def sgp_psi_grad(Xmean, Xvar, Y, z, ell, Q, R, ws=None):
    """Gradients of the psi statistics (hb_sgp_psi_grad): for F = 1/2 sum_n sum_mm' Q_mm' psi2_n(m, m') + sum_n sum_m
    (R Y_n)_m psi1_n(m), returns (mubar [N, d], sbar [N, d], zbar [M, d], ellbar [dl]) = dF / d(Xmean, Xvar, z, ell) as
    FLOAT64 device tensors, evaluated in double whatever the input dtype.  Xmean, Xvar [N, d] (Xvar >= 0: the caller's
    duty), Y [N, P], z [M, d], ell [dl] in one dtype; Q [M, M] (symmetric: its lower triangle is read) and R [M, P]
    float64.  Two calls return the same bits, and a point's rows of mubar, sbar do not depend on the other points."""
    if (Xmean.dim() != 2 or Y.dim() != 2 or z.dim() != 2 or Xvar.shape != Xmean.shape or Xmean.shape[0] != Y.shape[0]
            or Xmean.shape[1] != z.shape[1]):
        raise ValueError("sgp_psi_grad: Xmean [N, d], Xvar [N, d], Y [N, P], z [M, d] expected, got %s %s %s %s"
                         % (tuple(Xmean.shape), tuple(Xvar.shape), tuple(Y.shape), tuple(z.shape)))
    dt, dev = Xmean.dtype, Xmean.device
    _operands("sgp_psi_grad", Xmean, Xvar, Y, z, ell)
    _operands("sgp_psi_grad", torch.float64, Q, R, what="Q and R must be float64")
    N, d = Xmean.shape
    M, P = z.shape[0], Y.shape[1]
    _require(ell.dim() == 1 and ell.numel() in (1, d) and tuple(Q.shape) == (M, M) and tuple(R.shape) == (M, P), "sgp_psi_grad",
             "ell [1] or [%d], Q [%d, %d], R [%d, %d] expected, got %s %s %s"
             % (d, M, M, M, P, tuple(ell.shape), tuple(Q.shape), tuple(R.shape)))
    mubar = _empty((N, d), dtype=torch.float64, device=dev)
    sbar = _empty((N, d), dtype=torch.float64, device=dev)
    zbar = _empty((M, d), dtype=torch.float64, device=dev)
    ellbar = _empty((ell.numel(),), dtype=torch.float64, device=dev)
    ws = _ws("sgp_psi_grad", ws, dt, dev, sgp_psi_grad_ws_elems(dt, N, M, d, P), "sgp_psi_grad_ws_elems")
    _lib.lib().call("hb_sgp_psi_grad" + _suf(Xmean), KERN_RBF, _p(Xmean), _p(Xvar), _p(Y), _p(z), _p(ell), ell.numel(), _p(Q),
                    _p(R), _p(mubar), _p(sbar), _p(zbar), _p(ellbar), N, M, d, P, _p(ws), stream())
    return mubar, sbar, zbar, ellbar


def sgp_wstats_ws_elems(dtype, N, M, d):
    """Scratch elements hb_sgp_wstats needs (those of hb_sgp_stats with P = 1; the same for every N above one chunk)."""
    return _query("hb_sgp_wstats_ws_elems", N, M, d, _elem_bytes(dtype))


def sgp_wstats(X, w, r, z, ell, W, wfrag=None, ws=None):
    """Weighted statistics (hb_sgp_wstats): with A = W K(z, X) [M, N], (Phi = A diag(w) A^T [M, M], b = (A r)^T [1, M],
    tr Phi [1]) as FLOAT64 device tensors.  X [N, d], w [N] (any sign, zeros included), r [N], z [M, d], ell [dl],
    W [M, M]; one expert.  Phi is bitwise symmetric; two calls return the same bits; w == 1 gives the bits of sgp_stats."""
    if X.dim() != 2 or z.dim() != 2 or X.shape[1] != z.shape[1] or w.numel() != X.shape[0] or r.numel() != X.shape[0]:
        raise ValueError("sgp_wstats: X [N, d], w [N], r [N], z [M, d] expected, got %s %s %s %s"
                         % (tuple(X.shape), tuple(w.shape), tuple(r.shape), tuple(z.shape)))
    dt, dev = X.dtype, X.device
    _operands("sgp_wstats", X, w, r, z, ell, W, wfrag)
    N, d = X.shape
    M = z.shape[0]
    Phi = _empty((M, M), dtype=torch.float64, device=dev)
    b = _empty((1, M), dtype=torch.float64, device=dev)
    tr = _empty((1,), dtype=torch.float64, device=dev)
    ws = _ws("sgp_wstats", ws, dt, dev, sgp_wstats_ws_elems(dt, N, M, d), "sgp_wstats_ws_elems")
    _lib.lib().call("hb_sgp_wstats" + _suf(X), KERN_RBF, _p(X), _p(w), _p(r), _p(z), _p(ell), ell.numel(), _p(W), _p(wfrag),
                    _p(Phi), _p(b), _p(tr), N, M, d, _p(ws), stream())
    return Phi, b, tr


def sgp_mwstats_ws_elems(dtype, N, M, d, C):
    """Scratch elements hb_sgp_mwstats needs: those of hb_sgp_wstats, whatever C (the partial tiles are reused set by set)."""
    return _query("hb_sgp_mwstats_ws_elems", N, M, d, C, _elem_bytes(dtype))


def sgp_mwstats(X, w, r, z, ell, W, wfrag=None, ws=None):
    """Weighted statistics of C weight sets from ONE A = W K(z, X) (hb_sgp_mwstats): w [C, N], r [C, N] ->
    (Phi [C, M, M], b [C, M], tr [C]) as FLOAT64 device tensors, Phi_c = A diag(w_c) A^T, b_c = (A r_c)^T.  A is formed once
    per column chunk, the rank update runs set by set over it: set c has the BITS of sgp_wstats(X, w[c], r[c], ..).  The
    rows of w and r may be padded (stride(0) >= N, stride(1) == 1); every row of w must start 16-byte aligned, which a
    contiguous [C, N] float32 pair meets when N % 4 == 0 -- otherwise w and r are copied once into rows padded to a
    multiple of 4."""
    if (X.dim() != 2 or z.dim() != 2 or X.shape[1] != z.shape[1] or w.dim() != 2 or w.shape != r.shape
            or w.shape[1] != X.shape[0] or w.shape[0] < 1):
        raise ValueError("sgp_mwstats: X [N, d], w [C, N], r [C, N], z [M, d] expected, got %s %s %s %s"
                         % (tuple(X.shape), tuple(w.shape), tuple(r.shape), tuple(z.shape)))
    dt, dev = X.dtype, X.device
    _operands("sgp_mwstats", X, z, ell, W, wfrag)
    if w.dtype != dt or r.dtype != dt or not (w.is_cuda and r.is_cuda):   # (their rows may be padded: not _operands)
        raise TypeError("sgp_mwstats: all operands must live on the GPU and share one dtype")
    N, d = X.shape
    M, C = z.shape[0], w.shape[0]
    per16 = 16 // _elem_bytes(dt)
    ldw = w.stride(0) if C > 1 else N
    if (w.stride(1) != 1 or r.stride(1) != 1 or (C > 1 and (r.stride(0) != ldw or ldw < N or ldw % per16))
            or w.data_ptr() % 16):
        ldw = -(-N // per16) * per16
        wp, rp = (_empty((C, ldw), dtype=dt, device=dev) for _ in range(2))
        wp[:, :N].copy_(w)
        rp[:, :N].copy_(r)
        w, r = wp, rp
    Phi = _empty((C, M, M), dtype=torch.float64, device=dev)
    b = _empty((C, M), dtype=torch.float64, device=dev)
    tr = _empty((C,), dtype=torch.float64, device=dev)
    ws = _ws("sgp_mwstats", ws, dt, dev, sgp_mwstats_ws_elems(dt, N, M, d, C), "sgp_mwstats_ws_elems")
    _lib.lib().call("hb_sgp_mwstats" + _suf(X), KERN_RBF, _p(X), _p(w), _p(r), ldw, _p(z), _p(ell), ell.numel(), _p(W),
                    _p(wfrag), _p(Phi), _p(b), _p(tr), N, M, d, C, _p(ws), stream())
    return Phi, b, tr


def sgp_pathwise(x, omega, z, ell, coef, scale=1.0, out=None):
    """S pathwise function draws at the rows of x (hb_sgp_pathwise): out [S, n] = scale coef [S, 2L + M] B(x) with
    B = [cos / sin (omega_l . x / ell) interleaved | K(z_m, x)] synthesised inside the ONE launch.  x [n, d], omega [L, d],
    z [M, d] or None (M = 0: the prior path alone), ell [1] or [d], coef [S, 2L + M], all of one dtype.  The value of a
    column does not depend on the other columns: two calls, or x in pieces, return the same bits."""
    n, d, L, M, S = _pathwise_shapes("sgp_pathwise", x, omega, z, ell, coef)
    out = _out("sgp_pathwise", out, (S, n), x.dtype, x.device)
    _lib.lib().call("hb_sgp_pathwise" + _suf(x), KERN_RBF, _p(x), _p(omega), _p(z if M else None), _p(ell), ell.numel(), _p(coef),
                    float(scale), _p(out), n, L, M, d, S, stream())
    return out


def _pathwise_shapes(who, x, omega, z, ell, coef):
    """(n, d, L, M, S) of the operands of a pathwise entry (sgp_pathwise, _grad, _argmax, _acq), checked:
    on the device, contiguous, shapes that fit, one dtype."""
    if x.dim() != 2 or omega.dim() != 2 or coef.dim() != 2 or omega.shape[1] != x.shape[1] or (
            z is not None and (z.dim() != 2 or z.shape[1] != x.shape[1])):
        raise ValueError("%s: x [n, d], omega [L, d], z [M, d] or None, coef [S, 2L + M] expected, got %s %s %s %s"
                         % (who, tuple(x.shape), tuple(omega.shape), None if z is None else tuple(z.shape), tuple(coef.shape)))
    n, d = x.shape
    L, M, S = omega.shape[0], 0 if z is None else z.shape[0], coef.shape[0]
    if coef.shape[1] != 2 * L + M:
        raise ValueError("%s: coef must hold 2L + M = %d columns, got %s" % (who, 2 * L + M, tuple(coef.shape)))
    _operands(who, x, omega, z, ell, coef)
    return n, d, L, M, S


def sgp_pathwise_grad(x, omega, z, ell, coef, scale=1.0, out=None, grad=None, values=True):
    """Values and input gradients of S pathwise function draws in ONE launch (hb_sgp_pathwise_grad): (out [S, n], grad
    [S, n, d]) with grad[s, j, k] = d out[s, j] / d x_jk, operands as for sgp_pathwise.  values=False: the values are not
    stored, `out` (if given) is left untouched and None is returned in its place.  `out` carries the bits of sgp_pathwise;
    out[s, j] and grad[s, j, :] depend neither on the other columns nor on the other draws: two calls, x in pieces, or a
    subset of the draws return the same bits."""
    who = "sgp_pathwise_grad"
    n, d, L, M, S = _pathwise_shapes(who, x, omega, z, ell, coef)
    if values:
        out = _out(who, out, (S, n), x.dtype, x.device)
    grad = _out(who, grad, (S, n, d), x.dtype, x.device, "grad")
    _lib.lib().call("hb_sgp_pathwise_grad" + _suf(x), KERN_RBF, _p(x), _p(omega), _p(z if M else None), _p(ell), ell.numel(),
                    _p(coef), float(scale), _p(out if values else None), _p(grad), n, L, M, d, S, stream())
    return (out if values else None), grad


def sgp_pathwise_argmax_ws_elems(dtype, n, S):
    """Scratch elements (of the operands' dtype, whichever it is) hb_sgp_pathwise_argmax needs: 2 S ceil(n / 128)."""
    return _query("hb_sgp_pathwise_argmax_ws_elems", n, S)


def sgp_pathwise_argmax(x, omega, z, ell, coef, scale=1.0, largest=True, ws=None):
    """The extremum of each of S pathwise function draws over the rows of x (hb_sgp_pathwise_argmax): (best [S], idx int64
    [S]) device tensors with best[s] = max_j (largest) or min_j of sgp_pathwise(...)[s, j] -- those bits -- and idx[s] its
    first column; the [S, n] values are never written.  A NaN is never chosen; a draw with no comparable value reports
    idx = -1 and best = -inf (+inf for the minimum).  n >= 1.  `ws`: sgp_pathwise_argmax_ws_elems elements (default: the
    shared scratch of the stream)."""
    n, d, L, M, S = _pathwise_shapes("sgp_pathwise_argmax", x, omega, z, ell, coef)
    if n < 1:
        raise ValueError("sgp_pathwise_argmax: at least one candidate expected, got x %s" % (tuple(x.shape),))
    best = _empty((S,), dtype=x.dtype, device=x.device)
    idx = _empty((S,), dtype=torch.int64, device=x.device)
    ws = _ws("sgp_pathwise_argmax", ws, x.dtype, x.device, sgp_pathwise_argmax_ws_elems(x.dtype, n, S),
             "sgp_pathwise_argmax_ws_elems")
    _lib.lib().call("hb_sgp_pathwise_argmax" + _suf(x), KERN_RBF, _p(x), _p(omega), _p(z if M else None), _p(ell), ell.numel(),
                    _p(coef), float(scale), 1 if largest else 0, _p(best), _p(idx), n, L, M, d, S, _p(ws), stream())
    return best, idx


def sgp_pathwise_acq_ws_elems(n, S):
    """Scratch DOUBLES (whatever the operands' dtype) hb_sgp_pathwise_acq needs: 2 ceil(n / 128) for S <= 64, and
    ceil(S / 64) n more beyond."""
    return _query("hb_sgp_pathwise_acq_ws_elems", n, S)


def sgp_pathwise_acq(x, omega, z, ell, coef, incumbent, scale=1.0, acq="ei", largest=True, values=True, ws=None, out=None):
    """The Monte-Carlo acquisition of S pathwise function draws over per-draw incumbents at the rows of x
    (hb_sgp_pathwise_acq): (value [n] or None, best [1], idx int64 [1]) device tensors with, for F = sgp_pathwise(...),
    value[j] = mean_s max(sigma (F[s, j] - incumbent[s]), 0) ('ei') or mean_s 1[sigma (F[s, j] - incumbent[s]) > 0] ('pi'),
    sigma = +1 (largest) or -1, summed in double and rounded once; idx the first row with the largest value, best the
    value there, bit for bit; F is never written.  values=False: value is not stored either (`out`, if given, is left untouched and
    None is returned) -- for S <= 64 nothing of size n is written.  `out`: value written in place.  A NaN is never chosen; no comparable value: idx = -1 and best = -inf.  n >= 1.
    incumbent [S] of the operands' dtype; other operands as for sgp_pathwise.  `ws`: sgp_pathwise_acq_ws_elems float64
    elements (default: the shared float64 scratch of the stream)."""
    who = "sgp_pathwise_acq"
    n, d, L, M, S = _pathwise_shapes(who, x, omega, z, ell, coef)
    if n < 1:
        raise ValueError("%s: at least one candidate expected, got x %s" % (who, tuple(x.shape)))
    code = _code(who, PWACQ, acq)
    if incumbent is None:
        raise ValueError("%s: incumbent [S] expected, got None" % who)
    _chk(incumbent, "incumbent")
    if tuple(incumbent.shape) != (S,) or incumbent.dtype != x.dtype:
        raise ValueError("%s: incumbent must be [%d] of the operands' dtype, got %s %s"
                         % (who, S, tuple(incumbent.shape), incumbent.dtype))
    value = _out(who, out, (n,), x.dtype, x.device) if values else None
    best = _empty((1,), dtype=x.dtype, device=x.device)
    idx = _empty((1,), dtype=torch.int64, device=x.device)
    ws = _ws(who, ws, torch.float64, x.device, sgp_pathwise_acq_ws_elems(n, S), "sgp_pathwise_acq_ws_elems")
    _lib.lib().call("hb_sgp_pathwise_acq" + _suf(x), KERN_RBF, _p(x), _p(omega), _p(z if M else None), _p(ell), ell.numel(),
                    _p(coef), float(scale), int(code), 1 if largest else 0, _p(incumbent), _p(value), _p(best), _p(idx), n, L, M, d,
                    S, _p(ws), stream())
    return value, best, idx


def gram_matvec_chunk():
    """Rows per workgroup of hb_gram_matvec: a compile-time constant of the library."""
    return _query("hb_gram_matvec_chunk")


def gram_matvec_ws_elems(dtype, n, N, S):
    """Scratch elements hb_gram_matvec needs: 0 when N fits one chunk, chunks x S x n up to 16 chunks, beyond that 16 S n
    plus S n doubles -- O(S n) whatever N."""
    return _query("hb_gram_matvec_ws_elems", n, N, S, _elem_bytes(dtype))


def gram_matvec(x, x2, ell, V, scale=1.0, shift=0.0, out=None, ws=None, kind=KERN_RBF):
    """Matrix-free kernel product (hb_gram_matvec): out [S, n] = scale V [S, N] K(x2, x) + shift V with K never written.
    x [n, d], x2 [N, d] or None (the symmetric form x2 = x; only then may shift be non-zero), ell [1] or [d], V [S, N], all
    of one dtype.  The value of an output element depends neither on the other columns nor on the other rows of V: two
    calls, x in pieces, or a subset of the rows return the same bits.  `ws`: gram_matvec_ws_elems elements (default: the
    shared scratch of the stream)."""
    if x.dim() != 2 or V.dim() != 2 or ell.dim() != 1 or (x2 is not None and (x2.dim() != 2 or x2.shape[1] != x.shape[1])):
        raise ValueError("gram_matvec: x [n, d], x2 [N, d] or None, ell [1] or [d], V [S, N] expected, got %s %s %s %s"
                         % (tuple(x.shape), None if x2 is None else tuple(x2.shape), tuple(ell.shape), tuple(V.shape)))
    n, d = x.shape
    N = n if x2 is None else x2.shape[0]
    S = V.shape[0]
    if V.shape[1] != N:
        raise ValueError("gram_matvec: V must hold N = %d columns, got %s" % (N, tuple(V.shape)))
    _operands("gram_matvec", x, x2, ell, V)
    out = _out("gram_matvec", out, (S, n), x.dtype, x.device)
    ws = _ws("gram_matvec", ws, x.dtype, x.device, gram_matvec_ws_elems(x.dtype, n, N, S), "gram_matvec_ws_elems")
    _lib.lib().call("hb_gram_matvec" + _suf(x), int(kind), _p(x), _p(x2), _p(ell), ell.numel(), _p(V), float(scale),
                    float(shift), _p(out), n, N, d, S, _p(ws), stream())
    return out


GRAM_PREDICT_WS_BYTES = 1 << 30   # gram_predict cuts x into pieces so that hb_gram_predict's workspace stays under this


def gram_predict_ws_elems(dtype, n, N, S):
    """Scratch elements hb_gram_predict needs: min(chunks, 16) x S x n partials (one chunk included), S n doubles beyond
    16 chunks, and a double and a long per 256 columns for the arg-max."""
    return _query("hb_gram_predict_ws_elems", n, N, S, _elem_bytes(dtype))


def _gram_piece(ws_elems_of_n, dtype, n):
    """Columns per call of gram_predict / gram_predict_grad: the largest multiple of 128 whose workspace
    (ws_elems_of_n(columns) elements) fits GRAM_PREDICT_WS_BYTES (at least 128), or n when all of x fits."""
    if ws_elems_of_n(n) * _elem_bytes(dtype) <= GRAM_PREDICT_WS_BYTES:
        return max(n, 1)
    per128 = ws_elems_of_n(128) * _elem_bytes(dtype)
    return max(int(GRAM_PREDICT_WS_BYTES) // per128, 1) * 128


def _gram_predict_piece(n, N, S, dtype):
    """Columns per call of gram_predict (_gram_piece for its workspace)."""
    return _gram_piece(lambda m: gram_predict_ws_elems(dtype, m, N, S), dtype, n)


def _gram_predict_operands(who, x, x2, ell, V, P, acq, var_floor):
    """(n, d, N, S, P, code) of the operands of gram_predict / gram_predict_grad, checked: on the device, contiguous,
    shapes that fit, one dtype, 1 <= P <= S; code: the acquisition's (-1 for None), which needs P == 1 and var_floor >= 0."""
    if x.dim() != 2 or V.dim() != 2 or ell.dim() != 1 or x2.dim() != 2 or x2.shape[1] != x.shape[1]:
        raise ValueError("%s: x [n, d], x2 [N, d], ell [1] or [d], V [S, N] expected, got %s %s %s %s"
                         % (who, tuple(x.shape), tuple(x2.shape), tuple(ell.shape), tuple(V.shape)))
    (n, d), N, S, P = x.shape, x2.shape[0], V.shape[0], int(P)
    if V.shape[1] != N or N < 1 or ell.numel() not in (1, d):
        raise ValueError("%s: V must hold N = %d >= 1 columns and ell 1 or %d entries, got %s %s"
                         % (who, N, d, tuple(V.shape), tuple(ell.shape)))
    _operands(who, x, x2, ell, V)
    if not 1 <= P <= S:
        raise ValueError("%s: 1 <= P <= S mean rows expected, got P=%d, S=%d" % (who, P, S))
    if acq is None:
        return n, d, N, S, P, -1
    code = _code(who, ACQ, acq)
    if P != 1:
        raise ValueError("%s: an acquisition is defined for one latent function only (P=%d)" % (who, P))
    if not float(var_floor) >= 0.0:
        raise ValueError("%s: var_floor >= 0 expected (got %r)" % (who, var_floor))
    return n, d, N, S, P, code


def gram_predict(x, x2, ell, V, P=1, scale=1.0, prior=1.0, acq=None, best=0.0, param=0.0, largest=True, var_floor=0.0,
                 mean=True, var=True, value=None, argmax=False, kind=KERN_RBF):
    """Predictive mean, cached predictive variance and closed-form acquisition from ONE kernel product (hb_gram_predict).
    x [n, d], x2 [N, d], ell [1] or [d], V [S, N] = P mean rows, then S - P cache rows, all of one dtype.  With
    t = scale V K(x2, x) held in double:  mean [P, n] = t[:P] (the bits of gram_matvec on those rows),
    var [n] = max(prior - sum_{s >= P} t[s]^2, 0), and with acq 'ei' / 'pi' (param = xi, improvement over `best`) or 'ucb'
    (param = beta) the tail of sgp_acq at (t[0], prior - sum ..) for maximising (largest) or minimising; an acquisition
    needs P == 1.  Returns (mean, var, val [n], best_val float64 [1], best_idx int64 [1]) device tensors, None for each
    output not asked for (mean / var / value / argmax; value=None: values exactly when an acquisition is given and no
    arg-max).  best_val = max_j val[j], best_idx its first column; a NaN is never chosen, no comparable value: -1 and
    -inf; with argmax alone nothing of size n is written.  A column's results do not depend on the other columns: x is cut
    into pieces of a multiple of 128 columns so that the workspace stays under GRAM_PREDICT_WS_BYTES, the pieces' arg-max
    combined by the same strict rule, and the bits are those of one call."""
    who = "gram_predict"
    n, d, N, S, P, code = _gram_predict_operands(who, x, x2, ell, V, P, acq, var_floor)
    if acq is None:
        if value or argmax:
            raise ValueError("%s: value and argmax need an acquisition" % who)
        value = False
    else:
        value = (not argmax) if value is None else bool(value)
    if not (mean or var or value or argmax):
        raise ValueError("%s: at least one of mean, var, value, argmax expected" % who)
    if argmax and n < 1:
        raise ValueError("%s: at least one candidate expected, got x %s" % (who, tuple(x.shape)))
    dt, dev = x.dtype, x.device
    piece = _gram_predict_piece(n, N, S, dt)
    o_mean = _empty((P, n), dtype=dt, device=dev) if mean else None
    o_var = _empty((n,), dtype=dt, device=dev) if var else None
    o_val = _empty((n,), dtype=dt, device=dev) if value else None
    ws = workspace(dt, dev, max(gram_predict_ws_elems(dt, min(n, piece), N, S), 1))
    bests = []
    for a in range(0, n, piece):
        b = min(a + piece, n)
        whole = a == 0 and b == n
        m_p = o_mean if whole or not mean else _empty((P, b - a), dtype=dt, device=dev)
        bv = _empty((1,), dtype=torch.float64, device=dev) if argmax else None
        bi = _empty((1,), dtype=torch.int64, device=dev) if argmax else None
        _lib.lib().call("hb_gram_predict" + _suf(x), int(kind), _p(x[a:b]), _p(x2), _p(ell), ell.numel(), _p(V), P, float(scale),
                        float(prior), int(code), float(best), float(param), 1 if largest else 0, float(var_floor), _p(m_p),
                        _p(None if o_var is None else o_var[a:b]), _p(None if o_val is None else o_val[a:b]), _p(bv), _p(bi),
                        b - a, N, d, S, _p(ws), stream())
        if mean and not whole:
            o_mean[:, a:b].copy_(m_p)
        bests.append((a, bv, bi))
    if not argmax:
        return o_mean, o_var, o_val, None, None
    if len(bests) == 1:
        return o_mean, o_var, o_val, bests[0][1], bests[0][2]
    keys = torch.cat([bv for _, bv, _ in bests]).cpu().numpy()   # ONE read-back pair for all the pieces
    cols = torch.cat([bi for _, _, bi in bests]).cpu().numpy()
    bk, bj = -np.inf, -1
    for (a, _, _), k, j in zip(bests, keys, cols):   # pw_takes: strict, ties to the lowest column, an empty piece never
        if j >= 0 and (bj < 0 or k > bk):
            bk, bj = float(k), a + int(j)
    return (o_mean, o_var, o_val, torch.as_tensor([bk], dtype=torch.float64).to(dev),
            torch.as_tensor([bj], dtype=torch.int64).to(dev))


def gram_predict_grad_ws_elems(dtype, n, N, d, S):
    """Scratch elements hb_gram_predict_grad needs: 1 + d times the min(chunks, 16) x S x n partials of gram_predict and,
    beyond 16 chunks, 1 + d times S n doubles; no arg-max partials."""
    return _query("hb_gram_predict_grad_ws_elems", n, N, d, S, _elem_bytes(dtype))


def _gram_predict_grad_piece(n, N, d, S, dtype):
    """Columns per call of gram_predict_grad (_gram_piece for its workspace)."""
    return _gram_piece(lambda m: gram_predict_grad_ws_elems(dtype, m, N, d, S), dtype, n)


def gram_predict_grad(x, x2, ell, V, P=1, scale=1.0, prior=1.0, acq=None, best=0.0, param=0.0, largest=True, var_floor=0.0,
                      mean=True, var=True, value=None, dmean=True, dvar=True, dvalue=None, kind=KERN_RBF):
    """gram_predict's outputs and their input gradients from ONE kernel product (hb_gram_predict_grad).  Operands and the
    tail's arguments as for gram_predict.  With t as there and u[s, j, k] = d t[s, j] / d x_jk held in double the same way:
    dmean [P, n, d] = u[:P], dvar [n, d] = -2 sum_{s >= P} t[s] u[s] (exactly 0 where the variance was clamped to 0 and
    without cache rows), dval [n, d] = sgn a_mu u[0] + a_v (-2 sum ..) with a_mu, a_v the derivatives of the tail (a_v = 0
    where var_floor clamps); an acquisition needs P == 1.  Returns (mean, var, val, dmean, dvar, dval) device tensors, None
    for each output not asked for (value / dvalue = None: exactly when an acquisition is given); mean, var and val are the
    bits of gram_predict.  A column's results do not depend on the other columns: x is cut into pieces of a multiple of
    128 columns so that the workspace stays under GRAM_PREDICT_WS_BYTES, and the bits are those of one call."""
    who = "gram_predict_grad"
    n, d, N, S, P, code = _gram_predict_operands(who, x, x2, ell, V, P, acq, var_floor)
    if acq is None:
        if value or dvalue:
            raise ValueError("%s: value and dvalue need an acquisition" % who)
        value = dvalue = False
    else:
        value = True if value is None else bool(value)
        dvalue = True if dvalue is None else bool(dvalue)
    if not (mean or var or value or dmean or dvar or dvalue):
        raise ValueError("%s: at least one of mean, var, value, dmean, dvar, dvalue expected" % who)
    dt, dev = x.dtype, x.device
    piece = _gram_predict_grad_piece(n, N, d, S, dt)
    o_mean = _empty((P, n), dtype=dt, device=dev) if mean else None
    o_var = _empty((n,), dtype=dt, device=dev) if var else None
    o_val = _empty((n,), dtype=dt, device=dev) if value else None
    o_dmean = _empty((P, n, d), dtype=dt, device=dev) if dmean else None
    o_dvar = _empty((n, d), dtype=dt, device=dev) if dvar else None
    o_dval = _empty((n, d), dtype=dt, device=dev) if dvalue else None
    ws = workspace(dt, dev, max(gram_predict_grad_ws_elems(dt, min(n, piece), N, d, S), 1))
    cut = lambda t, a, b: None if t is None else t[a:b]
    for a in range(0, n, piece):
        b = min(a + piece, n)
        whole = a == 0 and b == n
        m_p = o_mean if whole or not mean else _empty((P, b - a), dtype=dt, device=dev)
        dm_p = o_dmean if whole or not dmean else _empty((P, b - a, d), dtype=dt, device=dev)
        _lib.lib().call("hb_gram_predict_grad" + _suf(x), int(kind), _p(x[a:b]), _p(x2), _p(ell), ell.numel(), _p(V), P,
                        float(scale), float(prior), int(code), float(best), float(param), 1 if largest else 0, float(var_floor),
                        _p(m_p), _p(cut(o_var, a, b)), _p(cut(o_val, a, b)), _p(dm_p), _p(cut(o_dvar, a, b)),
                        _p(cut(o_dval, a, b)), b - a, N, d, S, _p(ws), stream())
        if mean and not whole:
            o_mean[:, a:b].copy_(m_p)
        if dmean and not whole:
            o_dmean[:, a:b].copy_(dm_p)
    return o_mean, o_var, o_val, o_dmean, o_dvar, o_dval


def pcg_dot(a, b, out=None):
    """out [S] float64 = sum_i a_si b_si (hb_pcg_dot), a, b [S, N]."""
    _chk(a), _chk(b)
    if a.dim() != 2 or a.shape != b.shape or a.dtype != b.dtype:
        raise ValueError("pcg_dot: a, b [S, N] of one dtype expected, got %s %s" % (tuple(a.shape), tuple(b.shape)))
    out = _out("pcg_dot", out, (a.shape[0],), torch.float64, a.device, exact=False)
    _lib.lib().call("hb_pcg_dot" + _suf(a), _p(a), _p(b), _p(out), a.shape[0], a.shape[1], stream())
    return out


def _pcg_check(who, mats, vecs):
    S, N = mats[0].shape
    for t in mats:
        if t is not None:
            _chk(t)
            if tuple(t.shape) != (S, N) or t.dtype != mats[0].dtype:
                raise ValueError("%s: the vectors must be [%d, %d] of one dtype" % (who, S, N))
    for t in vecs:
        _chk(t)
        if t.numel() != S or t.dtype != torch.float64:
            raise ValueError("%s: the scalars must be float64 [%d]" % (who, S))
    return S, N


def _pcg_coef(who, coef, it, S):
    _chk(coef)
    it = int(it)
    if coef.dtype != torch.float64 or coef.dim() != 2 or coef.shape[1] != S or not 0 <= it < coef.shape[0] // 2:
        raise ValueError("%s: coef must be float64 [2 iterations, %d] with it below its iterations" % (who, S))
    return it


def pcg_update(x, r, p, Ap, rz, rr, thr, coef=None, it=0):
    """One lockstep CG update in place (hb_pcg_update): alpha = rz / (p . Ap), x += alpha p, r -= alpha Ap, rr = |r|^2 for
    every row with rr > thr; x, r, p, Ap [S, N], rz, rr, thr float64 [S].  coef (float64 [2 iterations, S]): alpha is also
    stored in coef[2 it] (hb_pcg_update_coef); the vectors and scalars are the same bits."""
    S, N = _pcg_check("pcg_update", (x, r, p, Ap), (rz, rr, thr))
    if coef is None:
        _lib.lib().call("hb_pcg_update" + _suf(x), _p(x), _p(r), _p(p), _p(Ap), _p(rz), _p(rr), _p(thr), S, N, stream())
    else:
        it = _pcg_coef("pcg_update", coef, it, S)
        _lib.lib().call("hb_pcg_update_coef" + _suf(x), _p(x), _p(r), _p(p), _p(Ap), _p(rz), _p(rr), _p(thr), S, N, _p(coef), it,
                        stream())


def pcg_direction(r, w, p, rz, rr, thr, wscale=1.0, zscale=1.0, first=False, coef=None, it=0):
    """The next search directions in place (hb_pcg_direction): z = (r - wscale w) zscale (w None: z = r), beta = (r . z) /
    rz (first: 0), p = z + beta p, rz = r . z for every row with rr > thr.  coef (float64 [2 iterations, S]): beta is also
    stored in coef[2 it + 1] (hb_pcg_direction_coef)."""
    S, N = _pcg_check("pcg_direction", (r, w, p), (rz, rr, thr))
    if coef is None:
        _lib.lib().call("hb_pcg_direction" + _suf(r), _p(r), _p(w), _p(p), _p(rz), _p(rr), _p(thr), float(wscale), float(zscale),
                        int(bool(first)), S, N, stream())
    else:
        it = _pcg_coef("pcg_direction", coef, it, S)
        _lib.lib().call("hb_pcg_direction_coef" + _suf(r), _p(r), _p(w), _p(p), _p(rz), _p(rr), _p(thr), float(wscale),
                        float(zscale), int(bool(first)), S, N, _p(coef), it, stream())


def gram_bilinear_grad_ws_elems(N, dl):
    """Scratch DOUBLES hb_gram_bilinear_grad needs: min(chunks, 16) x strips x (1 + dl) -- O(N), whatever S."""
    return _query("hb_gram_bilinear_grad_ws_elems", N, dl)


def gram_bilinear_grad(x, ell, A, B, w, out=None, ws=None, kind=KERN_RBF):
    """g [1 + dl] float64 (hb_gram_bilinear_grad): g[0] = sum_s w_s A_s K(x, x) B_s^T and g[1 + k] = sum_s w_s sum_ij A_si
    B_sj K_ij (x_ik - x_jk)^2 / ell_k^3 (dl = 1: summed over k), with neither K nor sum_s w_s A_s (x) B_s written to memory.
    x [N, d], ell [1] or [d], A, B [S, N] of one dtype; w [S] float64 (a device tensor, or anything numpy converts).  Two
    calls return the same bits.  `ws`: gram_bilinear_grad_ws_elems doubles (default: the shared scratch of the stream)."""
    who = "gram_bilinear_grad"
    if x.dim() != 2 or ell.dim() != 1 or A.dim() != 2 or tuple(A.shape) != tuple(B.shape) or A.shape[1] != x.shape[0]:
        raise ValueError("gram_bilinear_grad: x [N, d], ell [1] or [d], A, B [S, N] expected, got %s %s %s %s"
                         % (tuple(x.shape), tuple(ell.shape), tuple(A.shape), tuple(B.shape)))
    _operands(who, x, ell, A, B, what="x, ell, A and B must share one dtype")
    N, d = x.shape
    S, dl = A.shape[0], ell.numel()
    if not torch.is_tensor(w):
        w = torch.as_tensor(np.ascontiguousarray(w, dtype=np.float64)).to(x.device)
    _chk(w)
    if w.dtype != torch.float64 or w.numel() != S:
        raise ValueError("gram_bilinear_grad: w must be float64 [%d]" % S)
    out = _out(who, out, (1 + dl,), torch.float64, x.device, exact=False)
    ws = _ws(who, ws, torch.float64, x.device, gram_bilinear_grad_ws_elems(N, dl), "gram_bilinear_grad_ws_elems")
    _lib.lib().call("hb_gram_bilinear_grad" + _suf(x), int(kind), _p(x), _p(ell), dl, _p(A), _p(B), _p(w), _p(out), N, d, S,
                    _p(ws), stream())
    return out




def lik_sites(lik, y, mean, var, param=1.0, mscale=1.0, vscale=1.0, out=None):
    """Sites of a factorising likelihood under f_j ~ N(mscale mean_j, vscale var_j) (hb_lik_sites): (lam [N], beta [N]) in
    the dtype of the inputs and sum_j E[log p(y_j | f_j)] as a float64 device tensor [1].  lik: LIK_GAUSSIAN (param = the
    variance), LIK_BERNOULLI (logit link), LIK_POISSON (exp link), LIK_LAPLACE (param = the scale), LIK_GAMMA (exp link,
    param = the shape, y > 0), LIK_NEGBINOMIAL (exp link, param = the dispersion), LIK_BINOMIAL (logit link, param = the
    total count).  Double arithmetic; two calls return the same bits."""
    N = _lik_inputs("lik_sites", y, mean, var)
    lam, beta = _outs("lik_sites", out, ((N,),) * 2, y.dtype, y.device, ("lam", "beta"), exact=False)
    ell = _empty((1,), dtype=torch.float64, device=y.device)
    ws = workspace(torch.float64, y.device, _query("hb_lik_sites_ws_elems", N))
    _lib.lib().call("hb_lik_sites" + _suf(y), int(lik), _p(y), _p(mean), _p(var), float(mscale), float(vscale), float(param),
                    _p(lam), _p(beta), _p(ell), N, _p(ws), stream())
    return lam, beta, ell


def _lik_inputs(who, y, mean, var):
    for t in (y, mean, var):
        _chk(t)
    N = y.numel()
    if mean.numel() != N or var.numel() != N or mean.dtype != y.dtype or var.dtype != y.dtype:
        raise ValueError("%s: y, mean, var must hold N elements of one dtype" % who)
    return N


def lik_param_grad(lik, y, mean, var, param=1.0, mscale=1.0, vscale=1.0):
    """(sum_j E[log p(y_j | f_j)], its derivative with respect to the likelihood's own parameter at fixed moments) as a
    float64 device tensor [2], for f_j ~ N(mscale mean_j, vscale var_j) (hb_lik_param_grad).  lik: LIK_GAUSSIAN (d/dvar),
    LIK_LAPLACE (d/dscale), LIK_GAMMA (d/dshape), LIK_NEGBINOMIAL (d/ddispersion); the others have no continuous
    parameter and are refused.  Double arithmetic; two calls return the same bits."""
    N = _lik_inputs("lik_param_grad", y, mean, var)
    out = _empty((2,), dtype=torch.float64, device=y.device)
    ws = workspace(torch.float64, y.device, _query("hb_lik_param_grad_ws_elems", N))
    _lib.lib().call("hb_lik_param_grad" + _suf(y), int(lik), _p(y), _p(mean), _p(var), float(mscale), float(vscale),
                    float(param), _p(out), N, _p(ws), stream())
    return out


def lik_logdens(lik, y, mean, var, param=1.0, mscale=1.0, vscale=1.0, pointwise=True):
    """Predictive log density log E p(y_j | f_j), f_j ~ N(mscale mean_j, vscale var_j), of any LIK_* (hb_lik_logdens):
    (per point [N] in the dtype of the inputs, or None with pointwise=False; their sum as a float64 device tensor [1]).
    Closed form for LIK_GAUSSIAN and LIK_LAPLACE, the 20-node rule combined by log-sum-exp for the others."""
    N = _lik_inputs("lik_logdens", y, mean, var)
    out = _empty((N,), dtype=y.dtype, device=y.device) if pointwise else None
    total = _empty((1,), dtype=torch.float64, device=y.device)
    ws = workspace(torch.float64, y.device, _query("hb_lik_sites_ws_elems", N))
    _lib.lib().call("hb_lik_logdens" + _suf(y), int(lik), _p(y), _p(mean), _p(var), float(mscale), float(vscale), float(param),
                    _p(out), _p(total), N, _p(ws), stream())
    return out, total


def lik_predict(lik, mean, var, param=1.0):
    """(mean, variance) of a new observation y given f ~ N(mean, var) elementwise (hb_lik_predict), shaped like `mean`."""
    _chk(mean)
    _chk(var)
    if mean.shape != var.shape or mean.dtype != var.dtype:
        raise ValueError("lik_predict: mean and var must share shape and dtype")
    ym, yv = _empty_like(mean), _empty_like(mean)
    _lib.lib().call("hb_lik_predict" + _suf(mean), int(lik), _p(mean), _p(var), float(param), _p(ym), _p(yv), mean.numel(),
                    stream())
    return ym, yv


def _softmax_inputs(who, y, mean, var, nodes):
    """(N, C, S) of mean, var [C, N], nodes [S, C] float64 and, when given, y [N]."""
    for t in (mean, var, nodes) + (() if y is None else (y,)):
        _chk(t)
    if mean.dim() != 2 or var.shape != mean.shape or var.dtype != mean.dtype:
        raise ValueError("%s: mean and var must be [C, N] of one dtype, got %s %s" % (who, tuple(mean.shape), tuple(var.shape)))
    C, N = mean.shape
    if nodes.dim() != 2 or nodes.shape[1] != C or nodes.dtype != torch.float64:
        raise ValueError("%s: nodes must be float64 [S, %d], got %s %s" % (who, C, nodes.dtype, tuple(nodes.shape)))
    if y is not None and (y.numel() != N or y.dtype != mean.dtype):
        raise ValueError("%s: y must hold N = %d labels in the dtype of mean" % (who, N))
    return N, C, nodes.shape[0]


def lik_softmax_sites(y, mean, var, nodes, mscale=1.0, vscale=1.0, out=None):
    """Sites of the softmax likelihood under C independent marginals f_jc ~ N(mscale mean[c, j], vscale var[c, j])
    (hb_lik_softmax_sites): (lam [C, N], beta [C, N]) in the dtype of the inputs and sum_j E[log softmax(f_j)_{y_j}] as a
    float64 device tensor [1], the expectations taken over the S standard-normal nodes [S, C] (float64) shared by all
    points.  y [N]: labels 0 .. C-1 stored in the dtype of mean.  lam = mean_s p (1 - p) >= 0.  Double arithmetic; two
    calls return the same bits."""
    N, C, S = _softmax_inputs("lik_softmax_sites", y, mean, var, nodes)
    lam, beta = _outs("lik_softmax_sites", out, ((C, N),) * 2, mean.dtype, mean.device, ("lam", "beta"))
    lsum = _empty((1,), dtype=torch.float64, device=mean.device)
    ws = workspace(torch.float64, mean.device, _query("hb_lik_softmax_ws_elems", N, C))
    _lib.lib().call("hb_lik_softmax_sites" + _suf(mean), _p(y), _p(mean), _p(var), float(mscale), float(vscale), _p(nodes), S,
                    _p(lam), _p(beta), _p(lsum), N, C, _p(ws), stream())
    return lam, beta, lsum


def lik_softmax_grad(y, mean, var, nodes, mscale=1.0, vscale=1.0, out=None):
    """Weights of the hyper-parameter gradient of the softmax ELBO at fixed q (hb_lik_softmax_grad): (w [C, N], r [C, N],
    lsum [1]) as FLOAT64 device tensors whatever the dtype of the inputs, which are those of lik_softmax_sites.  r = g =
    mean_s ([c = y] - p_s) = dl/dmu and w = -mean_s(([c = y] - p_s) nodes[s, c]) / sqrt(v) = -2 dl/dv are the exact partial
    derivatives of the fixed-node value (w has either sign; where v <= 0 it is mean_s p (1 - p)).  lsum has the bits of
    lik_softmax_sites's.  out=(w, r): float64 [C, N] views whose rows may be padded (one stride(0) >= N for both,
    stride(1) == 1), written in place.  Two calls return the same bits."""
    N, C, S = _softmax_inputs("lik_softmax_grad", y, mean, var, nodes)
    if out is None:
        w, r = (_empty((C, N), dtype=torch.float64, device=mean.device) for _ in range(2))
    else:
        w, r = out
        for t in (w, r):
            if (not t.is_cuda or t.dtype != torch.float64 or tuple(t.shape) != (C, N) or t.stride(1) != 1
                    or t.stride(0) != w.stride(0) or t.stride(0) < N):
                raise ValueError("lik_softmax_grad: out = (w, r) must be float64 [%d, %d] device tensors with unit column "
                                 "stride and one row stride >= N" % (C, N))
    lsum = _empty((1,), dtype=torch.float64, device=mean.device)
    ws = workspace(torch.float64, mean.device, _query("hb_lik_softmax_ws_elems", N, C))
    _lib.lib().call("hb_lik_softmax_grad" + _suf(mean), _p(y), _p(mean), _p(var), float(mscale), float(vscale), _p(nodes), S,
                    _p(w), _p(r), max(int(w.stride(0)), N), _p(lsum), N, C, _p(ws), stream())
    return w, r, lsum


def lik_softmax_predict(mean, var, nodes, y=None, mscale=1.0, vscale=1.0, prob=True, pointwise=True):
    """Predictive of the softmax likelihood (hb_lik_softmax_predict): (prob [C, n] = mean_s softmax(f_s), or None with
    prob=False; logdens [n] = log mean_s softmax(f_s)_{y_j}, or None without y or with pointwise=False; their sum as a
    float64 device tensor [1], or None without y).  Inputs as for lik_softmax_sites."""
    n, C, S = _softmax_inputs("lik_softmax_predict", y, mean, var, nodes)
    if y is None and not prob:
        raise ValueError("lik_softmax_predict: nothing asked for (no y and prob=False)")
    pr = _empty_like(mean) if prob else None
    ld = _empty((n,), dtype=mean.dtype, device=mean.device) if (y is not None and pointwise) else None
    total = _empty((1,), dtype=torch.float64, device=mean.device) if y is not None else None
    ws = workspace(torch.float64, mean.device, _query("hb_lik_softmax_ws_elems", n, C))
    _lib.lib().call("hb_lik_softmax_predict" + _suf(mean), _p(y), _p(mean), _p(var), float(mscale), float(vscale), _p(nodes), S,
                    _p(pr), _p(ld), _p(total), n, C, _p(ws), stream())
    return pr, ld, total


def _hetgauss_inputs(who, y, mean, var):
    """(N, ld) of mean, var [2, N] views with one row stride ld >= N and unit column stride, and, when given, y [N]."""
    for t in (mean, var):
        if (not t.is_cuda or t.dim() != 2 or t.shape[0] != 2 or t.shape != mean.shape or t.dtype != mean.dtype
                or t.stride(1) != 1 or t.stride(0) != mean.stride(0) or t.stride(0) < t.shape[1]):
            raise ValueError("%s: mean and var must be [2, N] device tensors of one dtype with unit column stride and one "
                             "row stride >= N" % who)
    N = mean.shape[1]
    if y is not None and (_chk(y).numel() != N or y.dtype != mean.dtype):
        raise ValueError("%s: y must hold N = %d values in the dtype of mean" % (who, N))
    return N, max(int(mean.stride(0)), N)


def _hetgauss_rows(who, ts, names, N, ld, dtype, device):
    """[2, N] result views whose rows are ld apart (given), or fresh ones of row stride ld (None)."""
    res = []
    for t, name in zip(ts, names):
        if t is None:
            t = _empty((2, ld), dtype=dtype, device=device)[:, :N]
        elif (not t.is_cuda or t.dtype != dtype or tuple(t.shape) != (2, N) or t.stride(1) != 1
              or max(int(t.stride(0)), N) != ld):
            raise ValueError("%s: %s must be a [2, %d] device tensor of the inputs' dtype with unit column stride and the "
                             "row stride of mean (%d)" % (who, name, N, ld))
        res.append(t)
    return res


def lik_hetgauss_sites(y, mean, var, param=0.0, mscale=1.0, vscale=1.0, out=None, grad=False):
    """Sites of the heteroscedastic Gaussian likelihood y ~ N(f, exp(g + param)) under independent marginals of f (row 0
    of mean, var [2, N]) and g (row 1), scaled by mscale / vscale (hb_lik_hetgauss_sites): (lam [2, N], beta [2, N], r or
    None, lsum float64 [1]).  Closed form, lam >= 0 and lam = -2 dl/dv exactly; grad=True also returns r = dl/dmu [2, N]
    (sum_j r[1, j] is the derivative of lsum in param).  mean and var may be views of padded rows (one row stride >= N);
    the results share that row stride: out = (lam, beta) or (lam, beta, r) such views, or None for fresh ones.  Double
    arithmetic; two calls return the same bits."""
    who = "lik_hetgauss_sites"
    N, ld = _hetgauss_inputs(who, y, mean, var)
    names = ("lam", "beta", "r") if grad else ("lam", "beta")
    ts = (None,) * len(names) if out is None else tuple(out)
    if len(ts) != len(names):
        raise ValueError("%s: out must be (%s)" % (who, ", ".join(names)))
    res = _hetgauss_rows(who, ts, names, N, ld, mean.dtype, mean.device)
    lam, beta, r = res[0], res[1], (res[2] if grad else None)
    lsum = _empty((1,), dtype=torch.float64, device=mean.device)
    ws = workspace(torch.float64, mean.device, _query("hb_lik_hetgauss_ws_elems", N))
    _lib.lib().call("hb_lik_hetgauss_sites" + _suf(mean), _p(y), _p(mean), _p(var), ld, float(mscale), float(vscale),
                    float(param), _p(lam), _p(beta), _p(r), _p(lsum), N, _p(ws), stream())
    return lam, beta, r, lsum


def lik_hetgauss_predict(mean, var, param=0.0):
    """(mean [n], variance [n]) of a new observation under the heteroscedastic Gaussian likelihood given the (already
    scaled) marginals mean, var [2, n] of f and g (hb_lik_hetgauss_predict): (mu_f, v_f + exp(mu_g + param + v_g / 2))."""
    n, ld = _hetgauss_inputs("lik_hetgauss_predict", None, mean, var)
    ym, yv = (_empty((n,), dtype=mean.dtype, device=mean.device) for _ in range(2))
    _lib.lib().call("hb_lik_hetgauss_predict" + _suf(mean), _p(mean), _p(var), ld, float(param), _p(ym), _p(yv), n, stream())
    return ym, yv


def lik_hetgauss_logdens(y, mean, var, param=0.0, mscale=1.0, vscale=1.0, pointwise=True):
    """Predictive log density of the heteroscedastic Gaussian likelihood (hb_lik_hetgauss_logdens): (per point [N] in the
    dtype of the inputs, or None with pointwise=False; their sum as a float64 device tensor [1]).  f is integrated in
    closed form, g by the 20-node rule combined by log-sum-exp.  Inputs as for lik_hetgauss_sites."""
    N, ld = _hetgauss_inputs("lik_hetgauss_logdens", y, mean, var)
    out = _empty((N,), dtype=mean.dtype, device=mean.device) if pointwise else None
    total = _empty((1,), dtype=torch.float64, device=mean.device)
    ws = workspace(torch.float64, mean.device, _query("hb_lik_hetgauss_ws_elems", N))
    _lib.lib().call("hb_lik_hetgauss_logdens" + _suf(mean), _p(y), _p(mean), _p(var), ld, float(mscale), float(vscale),
                    float(param), _p(out), _p(total), N, _p(ws), stream())
    return out, total


def sgp_kgrad_ws_elems(N, M, d, P):
    """Scratch DOUBLES hb_sgp_kgrad needs: the repacked Q and one partial per strip -- independent of N."""
    return _query("hb_sgp_kgrad_ws_elems", N, M, d, P)


def sgp_kgrad(X, Y, z, ell, Q, R, ws=None, x_grad=False):
    """Streamed part of the gradient of the collapsed bound (hb_sgp_kgrad): with K = K(z, X), Kbar = Q K + R Y^T and
    E = Kbar o K, returns (zbar [M, d], ellbar [dl]) = (-sum_j E_ij (z_i - x_j) / ell^2, sum_ij E_ij (z_i - x_j)^2 / ell^3)
    as float64 device tensors.  X [N, d] and Y [N, P] share one storage dtype (float32 or float64); z [M, d], ell [dl],
    Q [M, M], R [M, P] are float64 and all arithmetic is float64.  Two calls on the same inputs return the same bits.
    x_grad=True (hb_sgp_kgrad_x): returns (zbar, ellbar, xbar) with the input gradient xbar [N, d] = +sum_i E_ij
    (z_i - x_j) / ell^2, float64, from the same pass; zbar and ellbar are the bits of x_grad=False."""
    if X.dim() != 2 or Y.dim() != 2 or z.dim() != 2 or X.shape[0] != Y.shape[0] or X.shape[1] != z.shape[1]:
        raise ValueError("sgp_kgrad: X [N, d], Y [N, P], z [M, d] expected, got %s %s %s"
                         % (tuple(X.shape), tuple(Y.shape), tuple(z.shape)))
    N, d = X.shape
    M, P = z.shape[0], Y.shape[1]
    if ell.dim() != 1 or ell.numel() not in (1, d) or tuple(Q.shape) != (M, M) or tuple(R.shape) != (M, P):
        raise ValueError("sgp_kgrad: ell [1] or [d], Q [M, M], R [M, P] expected, got %s %s %s"
                         % (tuple(ell.shape), tuple(Q.shape), tuple(R.shape)))
    what = "X and Y share one storage dtype; z, ell, Q, R must be float64"
    _operands("sgp_kgrad", X, Y, what=what)
    _operands("sgp_kgrad", torch.float64, z, ell, Q, R, what=what)
    dev = X.device
    zbar = _empty((M, d), dtype=torch.float64, device=dev)
    ellbar = _empty((ell.numel(),), dtype=torch.float64, device=dev)
    ws = _ws("sgp_kgrad", ws, torch.float64, dev, sgp_kgrad_ws_elems(N, M, d, P), "sgp_kgrad_ws_elems")
    if x_grad:
        xbar = _empty((N, d), dtype=torch.float64, device=dev)
        _lib.lib().call("hb_sgp_kgrad_x" + _suf(X), KERN_RBF, _p(X), _p(Y), _p(z), _p(ell), ell.numel(), _p(Q), _p(R),
                        _p(zbar), _p(ellbar), _p(xbar), N, M, d, P, _p(ws), stream())
        return zbar, ellbar, xbar
    _lib.lib().call("hb_sgp_kgrad" + _suf(X), KERN_RBF, _p(X), _p(Y), _p(z), _p(ell), ell.numel(), _p(Q), _p(R), _p(zbar),
                    _p(ellbar), N, M, d, P, _p(ws), stream())
    return zbar, ellbar


def sgp_wkgrad(X, w, r, z, ell, Q, R, ws=None, x_grad=False):
    """Column-weighted form of sgp_kgrad (hb_sgp_wkgrad): Kbar_ij = w_j (Q K)_ij + R_i r_j, one latent function.  X [N, d]
    in its storage dtype (float32 or float64); w [N], r [N], z [M, d], ell [dl], Q [M, M], R [M, 1] are float64 and all
    arithmetic is float64.  Returns (zbar [M, d], ellbar [dl]) as sgp_kgrad does; w == 1, r = Y[:, 0] returns its bits at
    P = 1; two calls on the same inputs return the same bits.  x_grad=True (hb_sgp_wkgrad_x): (zbar, ellbar, xbar) with the
    input gradient xbar [N, d] as sgp_kgrad returns it (E carries w and r)."""
    if X.dim() != 2 or z.dim() != 2 or X.shape[1] != z.shape[1] or tuple(w.shape) != (X.shape[0],) or tuple(r.shape) != w.shape:
        raise ValueError("sgp_wkgrad: X [N, d], w [N], r [N], z [M, d] expected, got %s %s %s %s"
                         % (tuple(X.shape), tuple(w.shape), tuple(r.shape), tuple(z.shape)))
    N, d = X.shape
    M = z.shape[0]
    if ell.dim() != 1 or ell.numel() not in (1, d) or tuple(Q.shape) != (M, M) or tuple(R.shape) != (M, 1):
        raise ValueError("sgp_wkgrad: ell [1] or [d], Q [M, M], R [M, 1] expected, got %s %s %s"
                         % (tuple(ell.shape), tuple(Q.shape), tuple(R.shape)))
    _operands("sgp_wkgrad", X)
    _operands("sgp_wkgrad", torch.float64, w, r, z, ell, Q, R, what="X in its storage dtype; w, r, z, ell, Q, R must be float64")
    dev = X.device
    zbar = _empty((M, d), dtype=torch.float64, device=dev)
    ellbar = _empty((ell.numel(),), dtype=torch.float64, device=dev)
    ws = _ws("sgp_wkgrad", ws, torch.float64, dev, sgp_kgrad_ws_elems(N, M, d, 1), "sgp_kgrad_ws_elems")
    if x_grad:
        xbar = _empty((N, d), dtype=torch.float64, device=dev)
        _lib.lib().call("hb_sgp_wkgrad_x" + _suf(X), KERN_RBF, _p(X), _p(w), _p(r), _p(z), _p(ell), ell.numel(), _p(Q), _p(R),
                        _p(zbar), _p(ellbar), _p(xbar), N, M, d, _p(ws), stream())
        return zbar, ellbar, xbar
    _lib.lib().call("hb_sgp_wkgrad" + _suf(X), KERN_RBF, _p(X), _p(w), _p(r), _p(z), _p(ell), ell.numel(), _p(Q), _p(R),
                    _p(zbar), _p(ellbar), N, M, d, _p(ws), stream())
    return zbar, ellbar


def sgp_select_ws_elems(dtype, N, M, d):
    """Scratch elements hb_sgp_select needs: the history C [M, N], dvar [N] and the arg-max partials -- O(M N)."""
    return _query("hb_sgp_select_ws_elems", N, M, d, _elem_bytes(dtype))


def sgp_select(X, ell, M, threshold=0.0, ws=None):
    """Greedy conditional-variance selection of M inducing points out of X [N, d] (hb_sgp_select: a pivoted incomplete
    Cholesky of K(X, X), one launch per chosen point, no read-back).  Returns device tensors (idx int64 [M], pivots [M]
    in the dtype of X, count int64 [1], trace float64 [1]): the chosen rows in selection order (exact ties of the
    conditional variance go to the lowest index, so idx[0] == 0), the conditional variance each had when chosen, how many
    were chosen before the largest conditional variance fell to `threshold` or below (idx / pivots from there on hold
    -1 / 0), and the residual sum of conditional variances tr(K_XX - K_XZ K_ZZ^-1 K_ZX).  ell [1] or [d]; one expert.
    Two calls on the same inputs return the same bits.  The workspace is O(M N) elements (sgp_select_ws_elems): when
    `ws` is not given it is allocated for this call alone and released with it, not taken from the shared scratch."""
    if X.dim() != 2 or ell.dim() != 1 or ell.numel() not in (1, X.shape[1]):
        raise ValueError("sgp_select: X [N, d] and ell [1] or [d] expected, got %s %s" % (tuple(X.shape), tuple(ell.shape)))
    dt, dev = X.dtype, X.device
    _operands("sgp_select", X, ell)
    N, d = X.shape
    M = int(M)
    if not 1 <= M <= N:
        raise ValueError("sgp_select: 1 <= M <= N expected, got M=%d, N=%d" % (M, N))
    if not float(threshold) >= 0.0:
        raise ValueError("sgp_select: threshold must be >= 0, got %r" % (threshold,))
    idx = _empty((M,), dtype=torch.int64, device=dev)
    pivots = _empty((M,), dtype=dt, device=dev)
    count = _empty((1,), dtype=torch.int64, device=dev)
    trace = _empty((1,), dtype=torch.float64, device=dev)
    need = sgp_select_ws_elems(dt, N, M, d)
    ws = _ws("sgp_select", _empty((need,), dtype=dt, device=dev) if ws is None else ws, dt, dev, need, "sgp_select_ws_elems")
    _lib.lib().call("hb_sgp_select" + _suf(X), KERN_RBF, _p(X), _p(ell), ell.numel(), N, M, d, float(threshold), _p(idx),
                    _p(pivots), _p(count), _p(trace), _p(ws), stream())
    return idx, pivots, count, trace


def sgp_bwd(x, z, ell, W, u, eps, A, v, fbar, mode=SGP_DIAGONAL, need_xbar=False, out=None, wfrag=None,
            prec=PREC_NATIVE, a_frag=None, kbar_frag=None):
    """Returns (Lbar, ubar, zbar, ellbar, xbar|None)."""
    E, n, M, d, P, sx = _sgp_dims(x, z, u)
    dev, dt = x.device, x.dtype
    dl = ell.numel() // E
    if out is None:
        Kbar = _empty_like(A) if a_frag is None else None
        Lbar = _empty_like(W)
        ubar = _empty_like(u)
        zbar = _empty_like(z)
        ellbar = _empty_like(ell)
        xbar = _empty((E, n, d), dtype=dt, device=dev) if need_xbar else None
    else:
        Kbar, Lbar, ubar, zbar, ellbar, xbar = out
    ws = workspace(dt, dev, sgp_ws_elems(E, n, M, d, P))
    if a_frag is not None and kbar_frag is None:
        kbar_frag = _empty(a_frag.numel(), dtype=dt, device=dev)
    _lib.lib().call("hb_sgp_bwd" + _suf(x), KERN_RBF, mode, _p(x), sx, _p(z), _p(ell), dl, _p(W), _p(wfrag), int(prec), _p(u), _p(eps),
                    _p(A) if a_frag is None else None, _p(a_frag), _p(v), _p(fbar), _p(Kbar) if a_frag is None else None,
                    _p(kbar_frag), _p(Lbar), _p(ubar), _p(zbar), _p(ellbar), _p(xbar), E, n, M, d, P, _p(ws), stream())
    return Lbar, ubar, zbar, ellbar, xbar


def sgp_bwd_phi_supported(E, n, M, d, P):
    """True when sgp_bwd_phi serves this shape (column-strip form in native precision) and the diagnostic switch
    sgp_phi_direct is not 0.  The planner asks when it builds a plan."""
    return bool(_query("hb_sgp_bwd_phi_supported", E, n, M, d, P))


def sgp_bwd_phi(x, z, ell, W, u, eps, v, fbar, wfrag, a_frag, mode=SGP_DIAGONAL, out=None, abar_frag=None):
    """sgp_bwd whose first result is the Cholesky VJP's operand Phi = Phisym(-Abar A^T) (= Phisym(L^T Lbar), both
    triangles) instead of Lbar: hb_sgp_bwd_phi_f32.  fp32, fragment-major W and A.  Returns (Phi, ubar, zbar, ellbar)."""
    E, n, M, d, P, sx = _sgp_dims(x, z, u)
    dev, dt = x.device, x.dtype
    _require(dt == torch.float32 and wfrag is not None and a_frag is not None, "sgp_bwd_phi", "float32 operands, wfrag and a_frag expected")
    dl = ell.numel() // E
    if out is None:
        Phi, ubar, zbar, ellbar = _empty_like(W), _empty_like(u), _empty_like(z), _empty_like(ell)
    else:
        Phi, ubar, zbar, ellbar = out
    ws = workspace(dt, dev, sgp_ws_elems(E, n, M, d, P))
    if abar_frag is None:
        abar_frag = _empty(a_frag.numel(), dtype=dt, device=dev)
    _ws("sgp_bwd_phi", abar_frag, dt, dev, sgp_frag_elems(E, n, M), "sgp_frag_elems", "abar_frag")
    _lib.lib().call("hb_sgp_bwd_phi_f32", KERN_RBF, mode, _p(x), sx, _p(z), _p(ell), dl, _p(W), _p(wfrag), _p(u), _p(eps), _p(a_frag),
                    _p(v), _p(fbar), _p(abar_frag), _p(Phi), _p(ubar), _p(zbar), _p(ellbar), E, n, M, d, P, _p(ws), stream())
    return Phi, ubar, zbar, ellbar


# ---- K9 Adam ---------------------------------------------------------------------
def adam_step(theta, g, m, v, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, gscale=1.0, tick=True, info=None, dpflag=None,
              fail=None):
    """In-place TF-1 Adam on flat buffers; `t` is a 1-element int64 device tensor (advanced when `tick`).
    `info` (int32 status words of this step's factorisations), `dpflag` (one element of theta's dtype: the
    all-reduced failure flag) and `fail` (int64[2], sticky) make the update a no-op when a factorisation failed."""
    _require(t.dtype == torch.int64, "adam_step", "t must be int64")
    n_info = 0
    if info is not None:
        _require(info.dtype == torch.int32 and info.is_contiguous(), "adam_step", "info must be contiguous int32")
        n_info = info.numel()
    if fail is not None:
        _require(fail.dtype == torch.int64 and fail.numel() == 2, "adam_step", "fail must be int64 [2]")
    if dpflag is not None:
        _require(dpflag.dtype == theta.dtype and dpflag.numel() == 1, "adam_step", "dpflag must be one element of theta's dtype")
    _lib.lib().call("hb_adam_step" + _suf(theta), _p(theta), _p(g), _p(m), _p(v), theta.numel(), float(lr), float(b1),
                    float(b2), float(eps), float(gscale), _p(t), int(bool(tick)), _p(info) if n_info else None, n_info,
                    _p(dpflag) if dpflag is not None else None, _p(fail) if fail is not None else None, stream())


# ---- data-parallel exchange ---------------------------------------------------------
def allreduce_sum(flat, comm_handle):
    """In-place RCCL all-reduce (sum) of a contiguous device buffer on the current stream."""
    _chk(flat)
    _lib.lib().call("hb_allreduce_sum" + _suf(flat), _p(flat), flat.numel(), comm_handle, stream())


def dp_pack(tail, objective, info):
    """tail[0] = objective, tail[1] = any(info != 0)  (hb_dp_pack)."""
    _require(tail.numel() == 2, "dp_pack", "tail must hold 2 elements")
    n_info = 0 if info is None else info.numel()
    _lib.lib().call("hb_dp_pack" + _suf(tail), _p(tail), _p(objective), _p(info) if n_info else None, n_info, stream())


# ---- hipGraph capture ---------------------------------------------------------------
class CapturedGraph:
    """A replayable hipGraph of whatever was launched between begin() and end()."""

    def __init__(self):
        self._exec = c_void_p(None)

    def begin(self):
        _lib.lib().call("hb_graph_begin_capture", stream())
        set_capturing(True)

    def end(self):
        set_capturing(False)
        _lib.lib().call("hb_graph_end_capture", stream(), ctypes.byref(self._exec))

    def launch(self):
        _lib.lib().call("hb_graph_launch", self._exec, stream())

    def __del__(self):
        try:
            if self._exec:
                _lib.lib().raw("hb_graph_destroy")(self._exec)
        except Exception:
            pass


def device_info():
    buf = ctypes.create_string_buffer(256)
    cus = ctypes.c_int(0)
    _lib.lib().call("hb_device_info", buf, 256, ctypes.byref(cus))
    return buf.value.decode(), cus.value
