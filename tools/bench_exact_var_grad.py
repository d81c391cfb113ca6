"""Time the input gradients of the exact GP's cached predictive against its values, in ONE process.

    python tools/bench_exact_var_grad.py [--N 10000,100000] [--n 64,100000] [--d 1,2,4] [--S 257] [--dtype float32]
                                         [--reps 5] [--iters 2] [--out profiles/exact_var_grad.txt]

Operands: x ~ U(0, side)^d [n, d], x2 ~ U(0, side)^d [N, d] with side = (N / 40)^(1 / d) lengthscales (about 40 rows per unit
volume), ell = 1, V ~ N(0, 1) [S, N] = one mean row and S - 1 cache rows.  For every (N, n, d):
  values     hb_gram_predict      mean + cached variance
  gradients  hb_gram_predict_grad  mean, variance and ALL gradients (dmean, dvar; with an EI tail also val and dval)
through hip_ops, so a workspace beyond GRAM_PREDICT_WS_BYTES is cut into pieces as a caller's would be.  Device events
around `iters` calls, `reps` rounds ALTERNATING between the forms after two warm-up calls each; median (min .. max) of the
rounds.  The MFMA work of the gradient entry is (1 + d) x that of the values, its exp2 work the same, its workspace and
fold traffic (1 + d) x: the ratio is recorded beside 1 + d and marked where it exceeds it.  No ratio is a pass condition."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def ab(forms, reps, iters):
    """{name: [ms per call] over the rounds}, the forms alternating inside every round, after two warm-up calls each."""
    for fn in forms.values():
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            times[k].append(timed(fn, iters))
    return times


def main():
    ints = lambda s: [int(v) for v in s.split(",")]
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=ints, default=[10000, 100000])
    ap.add_argument("--n", type=ints, default=[64, 100000])
    ap.add_argument("--d", type=ints, default=[1, 2, 4])
    ap.add_argument("--S", type=int, default=257)
    ap.add_argument("--dtype", default="float32", choices=["float32", "float64"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_var_grad.txt"))
    a = ap.parse_args()
    dt = getattr(torch, a.dtype)
    rng = np.random.default_rng(0)
    up = lambda v: torch.as_tensor(v, dtype=dt).cuda().contiguous()
    med = lambda ts: "%9.3f ms (%.3f .. %.3f)" % (np.median(ts), np.min(ts), np.max(ts))
    lines = ["exact GP, input gradients of the cached predictive: S = %d rows of V, %s (%s)" % (a.S, a.dtype, torch.cuda.get_device_name(0)),
             "values = hb_gram_predict (mean, var); gradients = hb_gram_predict_grad (mean, var, dmean, dvar); + EI tail: val / val, dval"]
    for N in a.N:
        for d in a.d:
            side = float((N / 40.0) ** (1.0 / d))
            x2, ell, V = up(rng.uniform(0.0, side, (N, d))), up(np.ones(1)), up(rng.standard_normal((a.S, N)))
            for n in a.n:
                x = up(rng.uniform(0.0, side, (n, d)))
                tail = dict(acq="ei", best=1.0, param=0.01, var_floor=1e-5)
                forms = dict(
                    values=lambda: H.gram_predict(x, x2, ell, V, prior=1.0),
                    gradients=lambda: H.gram_predict_grad(x, x2, ell, V, prior=1.0),
                    values_ei=lambda: H.gram_predict(x, x2, ell, V, prior=1.0, mean=False, var=False, value=True, **tail),
                    gradients_ei=lambda: H.gram_predict_grad(x, x2, ell, V, prior=1.0, mean=False, var=False, dmean=False, dvar=False,
                                                             **tail))
                t = ab(forms, a.reps, a.iters)
                r, r_ei = (np.median(t[k]) / np.median(t[v]) for k, v in (("gradients", "values"), ("gradients_ei", "values_ei")))
                pieces = -(-n // H._gram_predict_grad_piece(n, N, d, a.S, dt))
                mark = lambda q: "  ABOVE 1 + d" if q > 1 + d else ""
                lines += ["N = %d, n = %d, d = %d (side %.1f; the gradient call in %d piece%s of x)" % (N, n, d, side, pieces, "" if pieces == 1 else "s"),
                          "    values               %s" % med(t["values"]),
                          "    gradients            %s   ratio %.2f (1 + d = %d)%s" % (med(t["gradients"]), r, 1 + d, mark(r)),
                          "    EI value             %s" % med(t["values_ei"]),
                          "    EI value + gradient  %s   ratio %.2f (1 + d = %d)%s" % (med(t["gradients_ei"]), r_ei, 1 + d, mark(r_ei))]
                print("\n".join(lines[-5:]), flush=True)
                del x
            del x2, V
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
