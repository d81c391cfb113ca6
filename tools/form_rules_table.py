#!/usr/bin/env python
"""Print every answer of the library's form and size rules over a fixed grid, one line per (query, arguments, switch
setting).  Host code only: no GPU is needed.  Two builds compute the same rules exactly when their tables are
byte-identical:

    python tools/form_rules_table.py | sha256sum
    python tools/form_rules_table.py --ws | sha256sum      (the workspace size rules alone: the last section of the table)

Rules a planner once restated in Python are compared against that restatement: where `hip_ops` has no query for one
(an older build), the expression the planner used then stands in for it, verbatim.
"""
import itertools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from henbun_amd import _lib  # noqa: E402
from henbun_amd import hip_ops as H  # noqa: E402

ES = (1, 2, 8)
MS = (0, 16, 32, 48, 64, 96, 384, 512, 544, 1024)
NS = (0, 1, 31, 32, 33, 1024, 8192, 65536)
DS = (1, 2, 3, 4, 5)
PS = (0, 1, 2, 4, 5)
PRECS = (H.PREC_NATIVE, H.PREC_BF16X3)
DTYPES = (torch.float32, torch.float64)
# (switch, flipped value): every switch the sparse-GP form rules read, each flipped alone
SWITCHES = (None, ("sgp_no_strip", 1), ("sgp_force_strip", 1), ("sgp_tiled_crossover", 1), ("sgp_strip_form2", 1),
            ("sgp_no_fused_finish", 1), ("sgp_form16", 1), ("sgp_early", 0), ("sgp_phi_direct", 0), ("sgp_fwd_kbar", 0))


def _frag_image_elems(B, M, bf3):
    if hasattr(H, "cholesky_frag_elems"):
        return H.cholesky_frag_elems(B, M, bf3)
    return (5 if bf3 else 2) * B * M * M


def _wgk_shape(M, N, K, batch):
    if hasattr(H, "matmul_wgk_shape"):
        return H.matmul_wgk_shape(M, N, K, batch)
    ysh, kk = (batch, M, N), K
    return (ysh[-1] % 32 == 0 and ysh[-2] % 32 == 0 and kk % 128 == 0
            and 128 <= kk <= 4096 and (ysh[-1] // 32) * (ysh[-2] // 32) * int(np.prod(ysh[:-2]) if len(ysh) > 2 else 1) <= 1024)


def _gram_vjp_part(B, n, d):
    if hasattr(H, "matmul_gram_vjp_ws_elems"):
        return H.matmul_gram_vjp_ws_elems(B, n, d)
    return B * (n // 32) * (n // 32) * 32 * 2 * d


def rows():
    raw = _lib.lib().raw
    head_units, rider, ws_elems = raw("hb_sgp_head_units"), raw("hb_sgp_rider_supported"), raw("hb_sgp_ws_elems")
    fwd_kbar = raw("hb_sgp_fwd_kbar_supported")   # (rows of this query and the sgp_fwd_kbar section are additions: without them the table is the one before)
    shapes = list(itertools.product(ES, NS, MS, DS, PS))
    for E, n, M, d, P in shapes:
        for prec in PRECS:
            yield "sgp_strip_path", (E, n, M, d, P, prec), int(H.sgp_strip_path(E, n, M, d, P, prec))
            need = (E * n + 1) // 2
            for wf, draw, lanes in itertools.product((0, 1), (0, 1), (0, need - 1, need)):
                a = (E, n, M, d, P, prec, wf, draw, lanes)
                yield "sgp_head_units", a, int(head_units(*a))
                yield "sgp_rider_supported", a, int(rider(*a))
                yield "sgp_fwd_kbar_supported", a, int(fwd_kbar(*a))
        yield "sgp_bwd_phi_supported", (E, n, M, d, P), int(H.sgp_bwd_phi_supported(E, n, M, d, P))
        yield "sgp_ws_elems", (E, n, M, d, P), int(ws_elems(E, n, M, d, P))
        for dt, sk, wf in itertools.product(DTYPES, (H.SGP_S_DIAG, H.SGP_S_TRIL), (0, 1)):
            yield "sgp_predict_fused", (H._elem_bytes(dt), E, n, M, d, P, sk, wf), int(H.sgp_predict_fused(dt, E, n, M, d, P, sk, wf))
    for E, n, M in itertools.product(ES, NS, MS):
        for prec in PRECS:
            yield "sgp_frag_elems", (E, n, M, prec), int(H.sgp_frag_elems(E, n, M, prec))
    for B, M in itertools.product(ES, MS):
        for dt in DTYPES:
            yield "cholesky_persistent_shape", (B, M, H._elem_bytes(dt)), int(H.cholesky_persistent_shape(B, M, dt))
            yield "cholesky_ws_elems", (B, M, H._elem_bytes(dt)), int(H.cholesky_ws_elems(B, M, dt))
        for bf3 in (0, 1):
            yield "cholesky_frag_elems", (B, M, bf3), int(_frag_image_elems(B, M, bool(bf3)))
        for d in DS:
            yield "matmul_gram_vjp_ws_elems", (B, M, d), int(_gram_vjp_part(B, M, d))
        for N, K in itertools.product(MS, sorted(set(MS) | set(NS))):
            yield "matmul_wgk_shape", (M, N, K, B), int(bool(_wgk_shape(M, N, K, B)))


# the grid of the workspace size rules: every branch of the column-chunk rule (n = 0, below / at / above one strip of 32,
# at / above the 32768-column cap, beyond the element budget), both element sizes, with and without Wfrag
WS_NS = (0, 1, 31, 32, 33, 32768, 32769, 100000)
WS_MS = (32, 48, 512, 1024)
WS_PS = (1, 4, 5)
WS_CS = (1, 3)
WS_DS = (2, 5)
WS_ES = (1, 2)
WS_BYTES = (4, 8)


def ws_rows():
    """Every exported *_ws_elems rule of the chunked sparse-GP entries, asked through the C exports themselves (so that
    any build answers, whatever its `hip_ops` wraps)."""
    raw = _lib.lib().raw
    q = lambda name, *a: (name, a, int(raw("hb_" + name)(*a)))
    sks = (H.SGP_S_DIAG, H.SGP_S_TRIL)
    for n, M, d in itertools.product(WS_NS, WS_MS, WS_DS):
        for es in WS_BYTES:
            for P in WS_PS:
                yield q("sgp_stats_ws_elems", n, M, d, P, es)
            yield q("sgp_wstats_ws_elems", n, M, d, es)
            for C in WS_CS:
                yield q("sgp_mwstats_ws_elems", n, M, d, C, es)
            yield q("sgp_select_ws_elems", n, M, d, es)
            for sk, wf in itertools.product(sks, (0, 1)):
                yield q("sgp_predict_grad_ws_elems", n, M, d, sk, wf, es)
                yield q("sgp_acq_ws_elems", n, M, d, sk, wf, es)
                for E, P in itertools.product(WS_ES, WS_PS):
                    yield q("sgp_predict_ws_elems", E, n, M, d, P, sk, wf, es)
            for E, P, sk in itertools.product(WS_ES, WS_PS, sks):
                yield q("sgp_predict_cov_ws_elems", E, n, M, P, sk, es)
        for P in WS_PS:
            yield q("sgp_kgrad_ws_elems", n, M, d, P)


def main():
    out = sys.stdout
    if "--ws" in sys.argv:   # the workspace size rules alone
        out.write("".join("ws %s %s %d\n" % (name, ",".join(map(str, args)), val) for name, args, val in ws_rows()))
        return
    for sw in SWITCHES:
        H.debug_clear()
        tag = "default"
        if sw is not None:
            H.debug_set(*sw)
            tag = "%s=%d" % sw
        try:
            buf = []
            for name, args, val in rows():
                buf.append("%s %s %s %d\n" % (tag, name, ",".join(map(str, args)), val))
                if len(buf) >= 65536:
                    out.write("".join(buf))
                    buf = []
            out.write("".join(buf))
        finally:
            H.debug_clear()
    out.write("".join("ws %s %s %d\n" % (name, ",".join(map(str, args)), val) for name, args, val in ws_rows()))


if __name__ == "__main__":
    main()
