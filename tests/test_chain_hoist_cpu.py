"""The hoisted form of a serial chain (csrc/jit.hip, chain_source_hoist), checked on the host: jobs recorded with fake
pointers (nothing is launched), the generated text inspected and compiled for gfx950 with hiprtc."""
import ctypes
import os
from ctypes import c_double, c_int, c_long, c_void_p

import pytest

from henbun_amd import _lib, hip_ops as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "chain_plain_cfg2_tail_f32.txt")
R, NB, N = 70, 37, 143     # rows of the lengthscale fold, units of the likelihood fold, parameters


def _program(lib, suf, code, ins, istr, outs, oregs, ostr, shape):
    E = H.EW
    flat = []
    for op, dst, a, b, c in code:
        flat += [E[op], dst, a, b, c]
    cd = (c_int * len(flat))(*flat)
    pr = (c_double * (2 * len(code)))(*[0.0] * (2 * len(code)))
    handle, n, red = c_void_p(None), c_long(0), c_int(0)
    lib.call("hb_ewise_jit_build" + suf, len(code), cd, pr, len(ins), (c_void_p * len(ins))(*ins),
             (c_long * len(istr))(*istr), len(outs), (c_void_p * len(outs))(*outs), (c_int * len(oregs))(*oregs),
             (c_long * len(ostr))(*ostr), len(shape), (c_long * len(shape))(*shape), ctypes.byref(handle), ctypes.byref(n),
             ctypes.byref(red), None, 0)
    return handle


def _record_tail(lib, base, suf="_f32", esz=4, n=None, rows=R, nb=NB, grad=True, ntrail=3, trail_vec=0, over=True):
    """The tail of an SVGP step: lengthscale fold -> likelihood fold -> gradient program -> Adam -> transform program ->
    a program over the three sums and a fourth value next to them.  Returns the program handles (to destroy).
    ntrail: one-element parameter inputs of the transform program; trail_vec: instead, one input of that many parameters."""
    n = N if n is None else n
    at = lambda k: base + 0x40000 * k
    part_ell, ellbar, part_ll, stats = at(0), at(1), at(2), at(3)      # stats: ll, dscale, dvar, one external value
    va, vb, g, theta, m, v, t, info, fail, tr, st2 = (at(k) for k in range(4, 15))
    handles = []
    lib.call("hb_gram_ell_fold" + suf, part_ell, rows, 1, 1, 1, ellbar, None)
    lib.call("hb_gauss_ll_fold" + suf, part_ll, nb, stats, stats + esz, stats + 2 * esz, None)
    if grad:
        # gradient program over (R, 1): r0 ellbar, r1 ll, r2 dscale, r3 dvar (hand-offs), r4 / r5 external vectors
        handles.append(_program(lib, suf, [("MUL", 6, 4, 0, 0), ("MUL", 7, 5, 2, 0), ("ADD", 8, 6, 7, 0), ("MUL", 9, 0, 3, 0),
                                           ("ADD", 10, 1, 2, 0), ("MUL", 11, 8, 3, 0)],
                                [ellbar, stats, stats + esz, stats + 2 * esz, va, vb], [0, 0] * 4 + [1, 0] * 2,
                                [g + 5 * esz, g + esz, g + 2 * esz, g + 3 * esz], [8, 9, 10, 11 + H.EW_PROG_SUM],
                                [1, 0, 0, 0, 0, 0, 0, 0], [R, 1]))
        lib.call("hb_ewise_jit_run", handles[-1], None)
    lib.call("hb_adam_step" + suf, theta, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, -1.0, t, 1, info, 2, None, fail, None)
    if trail_vec:
        handles.append(_program(lib, suf, [("SOFTPLUS", 1, 0, 0, 0)], [theta], [1], [tr], [1], [1], [trail_vec]))
    else:
        K = ntrail
        last = theta + (n - K) * esz
        code = [("SOFTPLUS", K, K - 1, 0, 0), ("MUL", K + 1, 0, 1, 0)] + [("ADD", K + j, K + j - 1, j, 0) for j in range(2, K - 1)]
        handles.append(_program(lib, suf, code, [last + k * esz for k in range(K)], [0] * K, [tr, tr + esz],
                                [K, K + len(code) - 1], [0, 0], [1]))
    lib.call("hb_ewise_jit_run", handles[-1], None)
    if over:
        # four elements from `stats` on: three of them outputs of the fold (which only fills LDS slots), one external
        handles.append(_program(lib, suf, [("ADD", 1, 0, 0, 0)], [stats], [1], [st2], [1], [1], [4]))
        lib.call("hb_ewise_jit_run", handles[-1], None)
    return handles


def _source(lib, base, hoist=None, suf="_f32", esz=4, compile_it=False, **tail):
    assert lib.raw("hb_chain_discard")() == 0
    if hoist is not None:
        lib.call("hb_debug_set", b"chain_hoist", hoist)
    lib.call("hb_chain_begin")
    handles = []
    try:
        handles = _record_tail(lib, base, suf, esz, **tail)
        buf = ctypes.create_string_buffer(1 << 17)
        lib.call("hb_chain_source", buf, 1 << 17)
        if compile_it:
            lib.call("hb_chain_compile_dry")
        return buf.value.decode()
    finally:
        lib.raw("hb_chain_discard")()
        lib.call("hb_debug_clear")
        for h in handles:
            lib.raw("hb_ewise_jit_destroy")(h)


@pytest.fixture(scope="module")
def lib():
    L = _lib.lib()
    if not L.raw("hb_ewise_jit_available")():
        pytest.skip("hiprtc is not loadable in this process")
    return L


@pytest.mark.parametrize("suf, esz", [("_f32", 4), ("_f64", 8)])
def test_hoisted_chain_classifies_every_input_and_compiles_for_gfx950(lib, suf, esz):
    src = _source(lib, 0x1000000, suf=suf, esz=esz, compile_it=True)
    jobs = src.split("  __syncthreads();\n")
    assert len(jobs) == 6                                       # one barrier between jobs, as in the plain form
    top = src[:src.index("hb_chain_sync();")]
    # external operands of ALL jobs are requested in the load phase, in front of the first job
    assert "hb_gram_ell_load<T, 1>" in top and "hb_gauss_fold_load<T, 1>" in top and "hb_adam_status_load<T>" in top and "hb_adam_load_tmv<T, 1>" in top
    # the step size too (it needs only the step counter): one wave works it out and leaves it in a slot for Adam
    assert "hb_adam_lr<T>" in top and "hb_slot[4] = h3lr;" in top and "const T h3lr = hb_slot[4];" in jobs[3]
    assert "const T h2_4 = " in top and "const T h2_5 = " in top        # the gradient program's two external vectors
    assert "h2_0" not in top and "h2_1" not in top                    # ... not its hand-offs
    # internal scalars: the folds fill LDS slots, the gradient program reads them
    assert "__shared__ T hb_slot[5];" in src
    assert "smem, hb_slot + " in jobs[0] and "smem, hb_slot + " in jobs[1]
    for k in range(4):
        assert "T r%d = hb_slot[" % k in jobs[2]
    assert "T r4 = h2_4;" in jobs[2] and "T r5 = h2_5;" in jobs[2]
    # internal arrays: Adam's gradient is an LDS window the gradient program's four outputs are mirrored into, at an offset
    # worked out from the pointer arguments; the transform program reads windows over theta that Adam's stores fill
    assert "__shared__ T hb_win0[256];" in src and "hb_chain_win_load<T, 1>" in top
    assert jobs[2].count("hb_chain_mirror<T>(") == 4 and "hb_win0);" in jobs[2]
    assert "hb_adam_load_g<T, 1>(hb_win0," in jobs[3] and "hb_adam_body<T>(" in jobs[3]
    assert jobs[3].count("hb_chain_mirror<T>(hp, hv,") == 3
    for k in range(3):
        assert "T r%d = hb_win%d[0];" % (k, k + 1) in jobs[4]
    # a range that only partly consists of earlier outputs, written where no window can follow: the plain path
    assert "T r0 = in0[0 + x0 * 1L];" in jobs[5] and "hb_win4" not in src
    assert "0x" not in src.replace("0x0p+0", "")               # no addresses (0x0p+0 is the literal of a zero parameter)


def test_hoisted_chain_text_does_not_depend_on_the_addresses(lib):
    assert _source(lib, 0x1000000) == _source(lib, 0x7f0000200000)


def test_chain_hoist_0_gives_the_plain_text(lib):
    """hb_debug_set("chain_hoist", 0) emits the form in which every job loads after its barrier: the text recorded in
    tests/golden from the generator as it was before the hoisted form existed."""
    plain = _source(lib, 0x1000000, hoist=0)
    assert plain == open(GOLDEN).read()
    assert plain != _source(lib, 0x1000000) and "hb_slot" not in plain and "hb_win" not in plain


def test_transform_program_over_many_parameters_compiles(lib):
    """Seven one-element windows over theta behind Adam's gradient window (eight windows, the most a chain takes): Adam's
    stores carry one mirror per window in a single generated statement."""
    src = _source(lib, 0x1000000, ntrail=7, compile_it=True)
    adam = src.split("  __syncthreads();\n")[3]
    assert adam.count("hb_chain_mirror<T>(hp, hv,") == 7 and "hb_win7);" in adam and "hb_adam_tick(" in adam
    for k in range(7):
        assert "T r%d = hb_win%d[0];" % (k, k + 1) in src


def test_windows_past_the_count_limit_take_the_plain_path(lib):
    """Nine parameter inputs: the gradient and the first seven get the eight windows, the last two load after the barrier."""
    src = _source(lib, 0x1000000, ntrail=9, compile_it=True)
    trail = src.split("  __syncthreads();\n")[4]
    assert "__shared__ T hb_win7[1];" in src and "hb_win8" not in src
    assert "T r6 = hb_win7[0];" in trail and "T r7 = in7[0];" in trail and "T r8 = in8[0];" in trail
    assert src.split("  __syncthreads();\n")[3].count("hb_chain_mirror<T>(hp, hv,") == 7


def test_window_past_the_lds_budget_takes_the_plain_path(lib):
    """float64, 4096 parameters: the gradient window is 32 KB of the 40 KB a chain may use, so a transform program that
    reads 2048 parameters (16 KB) keeps the global load after the barrier."""
    src = _source(lib, 0x1000000, suf="_f64", esz=8, n=4096, trail_vec=2048, compile_it=True)
    adam, trail = src.split("  __syncthreads();\n")[3:5]
    assert "__shared__ T hb_win0[4096];" in src and "hb_win1" not in src
    assert "HbNoMirror()" in adam and "T r0 = in0[0 + x0 * 1L];" in trail


def test_load_phase_keeps_to_its_register_budget(lib):
    """The largest jobs a chain admits (16384 lengthscale partials, 4096 likelihood units, 4096 parameters) would hold
    16 + 12 + 16 values per thread in front of the first job.  The load phase may hold 40 registers, Adam goes first: in
    float32 the likelihood fold no longer fits and loads after its barrier; in float64 (two registers per value) both
    folds do.  Both compile."""
    kw = dict(n=4096, rows=16384, nb=4096, grad=False, over=False, compile_it=True)
    src = _source(lib, 0x1000000, **kw)
    top = src[:src.index("  {\n")]
    assert "hb_adam_load_tmv<T, 4>" in top and "hb_gram_ell_load<T, 16>" in top and "hb_gauss_fold_load" not in src
    src = _source(lib, 0x1000000, suf="_f64", esz=8, **kw)
    top = src[:src.index("  {\n")]
    assert "hb_adam_load_tmv<T, 4>" in top and "hb_adam_load_g<T, 4>" in top
    assert "hb_gram_ell_load" not in src and "hb_gauss_fold_load" not in src and "hb_gauss_fold_body<T>(" in src


def test_chain_without_a_parameter_update_keeps_the_plain_form(lib):
    """Folds and elementwise programs alone have one short round trip per job to give: such a chain is generated in the
    plain form whatever the switch says (csrc/jit.hip, chain_source)."""
    def text(hoist):
        assert lib.raw("hb_chain_discard")() == 0
        lib.call("hb_debug_set", b"chain_hoist", hoist)
        lib.call("hb_chain_begin")
        h = None
        try:
            at = lambda k: 0x1000000 + 0x40000 * k
            lib.call("hb_gauss_ll_fold_f32", at(0), NB, at(1), at(1) + 4, at(1) + 8, None)
            h = _program(lib, "_f32", [("ADD", 2, 0, 1, 0)], [at(1), at(2)], [0, 1], [at(3)], [2], [1], [R])
            lib.call("hb_ewise_jit_run", h, None)
            buf = ctypes.create_string_buffer(1 << 16)
            lib.call("hb_chain_source", buf, 1 << 16)
            lib.call("hb_chain_compile_dry")
            return buf.value.decode()
        finally:
            lib.raw("hb_chain_discard")()
            lib.call("hb_debug_clear")
            if h is not None:
                lib.raw("hb_ewise_jit_destroy")(h)
    assert text(1) == text(0) and "hb_slot" not in text(1) and "T r0 = in0[0];" in text(1)
