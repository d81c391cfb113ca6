"""Time the acquisition over pathwise function draws (hb_sgp_pathwise_acq, values=False) beside the kernel it shares its
whole synthesis and K-loop with, the per-draw arg-max (hb_sgp_pathwise_argmax), and beside the storing kernel
(hb_sgp_pathwise into [S, n]), in ONE process.

    python tools/bench_sgp_pathwise_acq.py [--reps 7] [--iters 3] [--quick] [--out profiles/sgp_pathwise_acq.txt]

Shapes: n = 10^6 candidates, L = 1024 features, M = 512 inducing points, d = 2, float32; S = 64 draws (one tile: the
acquisition finishes inside the main kernel) and S = 256 (four tiles: their partial sums go through the workspace).
Forms per shape (device events around `iters` calls; `reps` rounds, ALTERNATING between the forms so that each sees the
same clocks and neighbours; median and (min .. max) of the rounds; every form is warmed up first):
  argmax   hb_sgp_pathwise_argmax (both launches)                 -- the yardstick: the same K-loop, reduced over columns
  acq      hb_sgp_pathwise_acq 'ei', values=False (all launches)  -- the K-loop, reduced over the draws in double
  value    hb_sgp_pathwise into [S, n]                            -- the K-loop with the store epilogue
Printed per shape: acq / argmax, value / argmax, and whether the reducing epilogue costs more over argmax than the store
epilogue does (acq - argmax against value - argmax, with the run-to-run spread beside it).  No pass / fail ratio.  The
result is also checked: idx and best against the acquisition taken in numpy of the stored values at the arg-max column
and against a second call."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from henbun_amd import hip_ops as H  # noqa: E402


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="a hundredth of the points: checks the tool, measures nothing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    n, L, M, d, dtype = (10000 if args.quick else 1000000), 1024, 512, 2, torch.float32
    lines = ["device %s; n=%d L=%d M=%d d=%d float32; median of %d rounds of %d calls (min .. max), ms"
             % (H.device_info()[0], n, L, M, d, args.reps, args.iters)]
    rng = np.random.default_rng(d)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()
    X, z = up(rng.uniform(0, 16.0, (n, d))), up(rng.uniform(0, 16.0, (M, d)))
    omega, ell = up(rng.standard_normal((L, d))), up(np.ones(d))
    rows = []
    for S in (64, 256):
        c = rng.standard_normal((S, 2 * L + M))
        c[:, 2 * L:] *= 1e3
        coef = up(c)
        out = torch.empty((S, n), dtype=dtype, device="cuda")
        H.sgp_pathwise(X, omega, z, ell, coef, scale=1.3, out=out)
        inc = torch.quantile(out[:, :: max(n // 4096, 1)].double(), 0.99, dim=1).to(dtype).contiguous()   # few columns improve
        ws = torch.empty(max(H.sgp_pathwise_acq_ws_elems(n, S), 1), dtype=torch.float64, device="cuda")
        res = {}

        def f_acq():
            res["acq"] = H.sgp_pathwise_acq(X, omega, z, ell, coef, inc, scale=1.3, acq="ei", values=False, ws=ws)

        forms = dict(argmax=lambda: H.sgp_pathwise_argmax(X, omega, z, ell, coef, scale=1.3), acq=f_acq,
                     value=lambda: H.sgp_pathwise(X, omega, z, ell, coef, scale=1.3, out=out))
        for fn in forms.values():          # warm-up: every timed shape, code objects loaded
            fn()
            fn()
        torch.cuda.synchronize()
        _, best, idx = res["acq"]
        j, bv = int(idx.cpu()[0]), best.cpu().numpy()[0]
        col = out[:, j].cpu().numpy().astype(np.float64) - inc.cpu().numpy().astype(np.float64)
        want = np.float32(np.maximum(col, 0.0).sum() / S)
        f_acq()
        same = bool(abs(float(bv) - float(want)) <= float(np.spacing(want))) and torch.equal(res["acq"][1], best) and torch.equal(res["acq"][2], idx)
        times = {k: [] for k in forms}
        for _ in range(args.reps):
            for k, fn in forms.items():
                times[k].append(timed(fn, args.iters))
        st = {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in times.items()}
        spread = max(v[2] - v[1] for v in st.values())
        extra_acq, extra_val = st["acq"][0] - st["argmax"][0], st["value"][0] - st["argmax"][0]
        rows.append(dict(n=n, L=L, M=M, d=d, S=S, dtype="float32", result_checked=same, idx=j, best=float(bv),
                         ws_doubles=int(H.sgp_pathwise_acq_ws_elems(n, S)), **{k: [round(t, 4) for t in v] for k, v in st.items()}))
        lines.append("S=%3d: argmax %8.3f (%.3f .. %.3f) | acq %8.3f (%.3f .. %.3f) = x %.3f of argmax | value %8.3f (%.3f .. %.3f) "
                     "= x %.3f of argmax | epilogue over argmax: acq %+.3f ms, store %+.3f ms, spread %.3f ms: the reducing epilogue "
                     "costs %s the store epilogue%s"
                     % ((S,) + st["argmax"] + st["acq"] + (st["acq"][0] / st["argmax"][0],) + st["value"]
                        + (st["value"][0] / st["argmax"][0], extra_acq, extra_val, spread,
                           "MORE than" if extra_acq > extra_val + spread else "no more than", "" if same else "  RESULT NOT CONFIRMED")))
        print(lines[-1], flush=True)
        del out, coef, ws
    print(json.dumps(dict(rows=rows)), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
