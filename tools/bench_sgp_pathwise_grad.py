"""Time the input gradient and the arg-max of pathwise function draws (hb_sgp_pathwise_grad, hb_sgp_pathwise_argmax) in ONE
process, beside what they are measured against.

    python tools/bench_sgp_pathwise_grad.py [--reps 5] [--iters 3] [--quick] [--out profiles/pathwise_grad_bench.txt]

Shapes: the sparse one, (L, M) = (1024, 512) at n = 10^6 candidates, and the exact GP's, (L, M) = (1024, 10^5) at n = 10^4;
float32 and float64; d = 1, 2, 4; S = 1, 16, 64 draws.  Forms per shape (device events around `iters` calls; `reps` rounds,
ALTERNATING between the forms so that each sees the same clocks and neighbours; median and (min .. max) of the rounds):
  value    hb_sgp_pathwise alone                               -- the baseline of (a)
  grad     hb_sgp_pathwise_grad, values and gradients          -- (a): grad / value; the derivative products add d MFMA
                                                                  contractions and no transcendental: below 1 + d expected
  argmax   hb_sgp_pathwise_argmax (both launches)              -- (b)
  max      hb_sgp_pathwise into [S, n], then torch.max(dim=1)  -- the route without the fused kernel: the baseline of (b)
The one requirement: argmax is not slower than max by more than the run-to-run spread (max - min over the rounds, the
larger of the two forms') at n = 10^6, S = 64; the verdict is printed per dtype and d."""
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="a hundredth of the points: checks the tool, measures nothing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    shapes = [("sparse", 1000000, 1024, 512), ("exact", 10000, 1024, 100000)]
    if args.quick:
        shapes = [("sparse", 10000, 1024, 512), ("exact", 1000, 1024, 10000)]
    lines = ["device %s; median of %d rounds of %d calls (min .. max), ms" % (H.device_info()[0], args.reps, args.iters)]
    rows, verdicts = [], []
    for name, n, L, M in shapes:
        for dtype in (torch.float32, torch.float64):
            for d in (1, 2, 4):
                rng = np.random.default_rng(d)
                up = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()
                X, z = up(rng.uniform(0, 16.0, (n, d))), up(rng.uniform(0, 16.0, (M, d)))
                omega, ell = up(rng.standard_normal((L, d))), up(np.ones(d))
                for S in (1, 16, 64):
                    c = rng.standard_normal((S, 2 * L + M))
                    c[:, 2 * L:] *= 1e3
                    coef = up(c)
                    out = torch.empty((S, n), dtype=dtype, device="cuda")
                    grad = torch.empty((S, n, d), dtype=dtype, device="cuda")
                    res = {}

                    def f_max():
                        H.sgp_pathwise(X, omega, z, ell, coef, scale=1.3, out=out)
                        res["max"] = torch.max(out, dim=1)

                    def f_argmax():
                        res["argmax"] = H.sgp_pathwise_argmax(X, omega, z, ell, coef, scale=1.3)

                    forms = dict(value=lambda: H.sgp_pathwise(X, omega, z, ell, coef, scale=1.3, out=out),
                                 grad=lambda: H.sgp_pathwise_grad(X, omega, z, ell, coef, scale=1.3, out=out, grad=grad),
                                 argmax=f_argmax, max=f_max)
                    for fn in forms.values():          # warm-up: every timed shape, code objects loaded
                        fn()
                        fn()
                    torch.cuda.synchronize()
                    same = bool(torch.equal(res["argmax"][0], res["max"].values) and torch.equal(res["argmax"][1], res["max"].indices))
                    times = {k: [] for k in forms}
                    for _ in range(args.reps):
                        for k, fn in forms.items():
                            times[k].append(timed(fn, args.iters))
                    st = {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in times.items()}
                    spread = max(st["argmax"][2] - st["argmax"][1], st["max"][2] - st["max"][1])
                    row = dict(shape=name, n=n, L=L, M=M, dtype=str(dtype).split(".")[-1], d=d, S=S, same_result=same,
                               **{k: [round(t, 4) for t in v] for k, v in st.items()})
                    rows.append(row)
                    lines.append("%-6s n=%7d L=%d M=%6d %s d=%d S=%2d: value %8.3f (%.3f .. %.3f) | grad %8.3f (%.3f .. %.3f) = x %.2f "
                                 "of value (1 + d = %d) | argmax %8.3f (%.3f .. %.3f) | value + torch.max %8.3f (%.3f .. %.3f) | "
                                 "argmax / that = %.3f%s"
                                 % ((name, n, L, M, row["dtype"], d, S) + st["value"] + st["grad"] + (st["grad"][0] / st["value"][0], 1 + d)
                                    + st["argmax"] + st["max"] + (st["argmax"][0] / st["max"][0], "" if same else "  RESULTS DIFFER")))
                    if name == "sparse" and S == 64:
                        ok = st["argmax"][0] <= st["max"][0] + spread
                        verdicts.append("requirement at n=%d S=64 %s d=%d: argmax %.3f ms against %.3f ms, spread %.3f ms: %s"
                                        % (n, row["dtype"], d, st["argmax"][0], st["max"][0], spread, "holds" if ok else "FAILS"))
                    del out, grad, coef
                    print(lines[-1], flush=True)
    text = "\n".join(lines + verdicts) + "\n"
    print("\n".join(verdicts), flush=True)
    print(json.dumps(dict(rows=rows)), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
