"""The fold of a Gram VJP's tile partials as the head of a serial chain (hb_gram_tiles_fold_f32; csrc/chain_bodies.cuh,
csrc/jit.hip), checked on the host: the jobs of the benchmark's last chain recorded with fake pointers (nothing is
launched), the generated text inspected, compiled for gfx950 with hipcc and its code object's resource notes read; the
chain of the switched-off path is the text the generator gave before the fold existed; the eligibility rule against
its restatement in Python."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import test_chain_hoist_cpu as CH
from henbun_amd import _build, _lib, hip_ops as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "henbun_amd", "csrc")
M, D, NB, NPAR = 512, 1, 256, 1540       # the benchmark's chain: 16384 tile partials, 256 likelihood units, 1540 parameters


@pytest.fixture(scope="module")
def lib():
    L = _lib.lib()
    if not L.raw("hb_ewise_jit_available")():
        pytest.skip("hiprtc is not loadable in this process")
    return L


def _record(lib, base, m=M, d=D, dl=1, nb=NB, n=NPAR):
    """tile fold -> likelihood fold -> gradient program (Xbar + an external vector, the scalars) -> Adam -> transforms."""
    esz = 4
    at = lambda k: base + 0x40000 * k
    part, xbar, ellbar, part_ll, stats, zb, va, g, theta, mm, vv, t, info, fail, tr = (at(k) for k in range(15))
    handles = []
    lib.call("hb_gram_tiles_fold_f32", part, 1, m, d, dl, xbar, ellbar, None)
    lib.call("hb_gauss_ll_fold_f32", part_ll, nb, stats, stats + esz, stats + 2 * esz, None)
    rows = m * d
    # r0 Xbar (written by the fold: a window), r1 external vector, r2 ellbar, r3..r5 the three sums (slots), r6 external scalar
    code = [("ADD", 7, 0, 1, 0), ("MUL", 8, 2, 6, 0), ("ADD", 9, 3, 4, 0), ("MUL", 10, 5, 6, 0)]
    handles.append(CH._program(lib, "_f32", code, [xbar, zb, ellbar, stats, stats + esz, stats + 2 * esz, va],
                               [1, 0, 1, 0] + [0, 0] * 5, [g, g + rows * esz, g + (rows + 1) * esz, g + (rows + 2) * esz],
                               [7, 8, 9, 10], [1, 0, 0, 0, 0, 0, 0, 0], [rows, 1]))
    lib.call("hb_ewise_jit_run", handles[-1], None)
    lib.call("hb_adam_step_f32", theta, g, mm, vv, n, 1e-3, 0.9, 0.999, 1e-8, -1.0, t, 1, info, 2, None, fail, None)
    last = theta + (n - 3) * esz
    handles.append(CH._program(lib, "_f32", [("SOFTPLUS", 3, 2, 0, 0), ("MUL", 4, 0, 1, 0)], [last, last + esz, last + 2 * esz], [0] * 3,
                               [tr, tr + esz], [3, 4], [0, 0], [1]))
    lib.call("hb_ewise_jit_run", handles[-1], None)
    return handles


def _source(lib, base, hoist=None, compile_it=False, **kw):
    assert lib.raw("hb_chain_discard")() == 0
    if hoist is not None:
        lib.call("hb_debug_set", b"chain_hoist", hoist)
    lib.call("hb_chain_begin")
    handles = []
    try:
        handles = _record(lib, base, **kw)
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


def _prelude():
    """The text in front of every generated kernel, as henbun_amd/_build.py assembles it from the sources."""
    header = open(os.path.join(ROOT, "include", "henbun_hip.h")).read()
    parts = [re.search(r"enum \{\s*/\* unary \*/.*?HB_EW_GAUSS_LOGPDF_GRAD[^}]*\};", header, re.S).group(0)]
    parts += [open(os.path.join(CSRC, n)).read() for n in ("ew_math.cuh", "ew_apply.cuh", "rng_core.cuh", "chain_bodies.cuh")]
    return "\n".join(parts)


def _resources(text, tmp_path):
    """hipcc --offload-arch=gfx950 on prelude + text; the kernel's notes (llvm-readelf --notes) as a dict of integers."""
    hipcc = _build._hipcc()
    readelf = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin", "llvm-readelf")
    if not os.path.exists(readelf):
        readelf = shutil.which("llvm-readelf")
    assert readelf, "llvm-readelf not found next to hipcc"
    src, obj = tmp_path / "chain.hip", tmp_path / "chain.co"
    src.write_text("#include <hip/hip_runtime.h>\n#include <cstdint>\n" + _prelude() + text)   # (what hiprtc declares by itself)
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "--no-gpu-bundle-output", "-c", str(src), "-o", str(obj)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    notes = subprocess.run([readelf, "--notes", str(obj)], capture_output=True, text=True, check=True).stdout
    assert ".name:           hb_jit_kernel" in notes, notes[-2000:]
    return {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", notes)}


def test_tile_fold_joins_the_load_phase_and_hands_over_through_lds(lib):
    src = _source(lib, 0x1000000, compile_it=True)
    jobs = src.split("  __syncthreads();\n")
    assert len(jobs) == 5
    top = src[:src.index("hb_chain_sync();")]
    # sixteen shares per thread (one output, sixteen tiles), requested with every other external operand of the chain
    assert "T h0p[16]; hb_gram_tiles_load<T, 1, 16>(" in top and "hb_gauss_fold_load<T, 1>" in top and "hb_adam_load_tmv<T, 2>" in top
    assert "hb_gram_tiles_body<T, 1, 16>(h0p," in jobs[0]
    # Xbar reaches the gradient program through an LDS window the fold's stores are mirrored into, ellbar through a slot
    assert "hb_chain_mirror<T>(hp, hv," in jobs[0] and "smem, [&](const T* hp, T hv)" in jobs[0] and "hb_slot + 0);" in jobs[0]
    assert re.search(r"T r0 = hb_win\d\[0 \+ x0 \* 1L\];", jobs[2]) and "T r2 = hb_slot[0];" in jobs[2]
    assert "0x" not in src.replace("0x0p+0", "")
    assert src == _source(lib, 0x7f0000200000)                    # the text does not depend on the addresses


def test_chain_with_the_tile_fold_compiles_for_gfx950_without_scratch(lib, tmp_path):
    """The benchmark's chain, and the largest fold the rule admits next to the largest Adam (two outputs of eight tiles per
    thread: M = 256, d = 4): no spilled register, no private segment, inside the 128 registers of a 1024-thread workgroup."""
    for kw in (dict(), dict(m=256, d=4, dl=4, n=4096)):
        res = _resources(_source(lib, 0x1000000, **kw), tmp_path)
        print("gram_tiles chain %s: %s" % (kw or "cfg2", res))
        assert res["vgpr_spill_count"] == 0 and res["private_segment_fixed_size"] == 0, res
        assert res["vgpr_count"] <= 128, res


def test_plain_form_and_the_untouched_chains(lib, tmp_path):
    """chain_hoist 0: the fold loads after its barrier like every job of the plain form, and compiles.  A chain without the
    fold -- what the planner records under hb_debug_set("gram_vjp_tiles", 0) -- is generated as before the fold existed: the
    plain text recorded in tests/golden, and the same hoisted text under either value of the switch."""
    plain = _source(lib, 0x1000000, hoist=0, compile_it=True)
    assert "hb_gram_tiles_body<T>(" in plain and "hb_slot" not in plain and "hb_win" not in plain
    texts = []
    for sw in (0, 1):
        lib.call("hb_debug_set", b"gram_vjp_tiles", sw)
        assert CH._source(lib, 0x1000000, hoist=0) == open(CH.GOLDEN).read()      # (CH._source clears the switches)
        lib.call("hb_debug_set", b"gram_vjp_tiles", sw)
        texts.append(CH._source(lib, 0x1000000))
    assert texts[0] == texts[1] and "hb_gram_tiles" not in texts[0]


def _tiles_ok(Mm, K, batch, d):
    """hb_matmul_gram_vjp_tiles_ok restated: the in-workgroup split-K form of a square product (M % 32 == 0, K % 128 == 0,
    128 <= K <= 4096, at most 1024 tiles, batch <= 65535), 1 <= d <= 4, at most 16384 tile partials."""
    if Mm % 32 or K % 128 or K < 128 or K > 4096 or (Mm // 32) ** 2 * batch > 1024 or batch > 65535 or not 1 <= d <= 4:
        return False
    return batch * (Mm // 32) ** 2 * 32 * 2 * d <= 16384


def test_rule_matches_its_restatement():
    import torch

    H.debug_clear()
    table = [(Mm, K, b, d) for Mm in (96, 128, 256, 384, 512, 1024) for K in (64, 128, 192, 512) for b in (1, 2, 4, 8, 16, 17) for d in (1, 2, 3, 4, 5)]
    table += [(512, 512, 1, 1), (512, 512, 8, 1), (512, 512, 1, 2), (128, 128, 16, 1), (128, 128, 4, 4), (128, 128, 5, 4), (256, 256, 1, 4)]
    raw = _lib.lib().raw("hb_matmul_gram_vjp_tiles_ok")
    for Mm, K, b, d in table:
        assert bool(raw(Mm, K, b, d)) == _tiles_ok(Mm, K, b, d) == H.matmul_gram_vjp_tiles_ok(Mm, K, b, d, torch.float32), (Mm, K, b, d)
    assert H.matmul_gram_vjp_tiles_ok(512, 512, 1, 1, torch.float32) and not H.matmul_gram_vjp_tiles_ok(512, 512, 8, 1, torch.float32)
    assert not H.matmul_gram_vjp_tiles_ok(512, 512, 1, 1, torch.float64)
    try:
        H.debug_set("gram_vjp_tiles", 0)
        assert not H.matmul_gram_vjp_tiles_ok(512, 512, 1, 1, torch.float32) and H.matmul_gram_vjp_ok(512, 512, 1, 1, torch.float32)
    finally:
        H.debug_clear()
