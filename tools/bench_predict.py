"""Time SparseGP.predict_f: the fused streaming kernel against the chunked form (and the generic graph composition
where its materialised A fits comfortably), in ONE process, alternating between the forms.

    python tools/bench_predict.py [--n 100000 1000000] [--reps 7] [--iters 10]

One JSON line per (case, form): ms per prediction (the whole plan: Gram + Cholesky of z, then the prediction),
points/s and the achieved TF/s on the algorithmic work -- the triangular product A = W K counted as M^2 N flop, plus
M^2 N for S^T A with a full-rank q(u).  Kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_predict.py ...` (sgp_predict_strip_kernel, the chunked form's
sgp_A_* / matmul / pred_colstat_kernel)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import henbun_amd as hb  # noqa: E402
from henbun_amd.gp.gp import _posterior_of  # noqa: E402
from henbun_amd.models import SVGP, svgp_data  # noqa: E402


def make_plan(m, xs, form):
    q = object.__getattribute__(m, "u")
    cfg = hb.settings.get_settings()
    cfg.runtime.fused_predict = form == "fused"
    with hb.settings.temp_settings(cfg):
        with m.tf_mode():
            if form == "generic":
                mm, s, kind = _posterior_of(q)
                mean, var = m.gp._predict_generic(hb.graph.as_tensor(xs), mm, s, kind, "diagonal",
                                                  hb.settings.numerics.jitter_level)
            else:
                mean, var = m.gp.predict_f(xs, q, q_shape="diagonal")
        plan = m._session.make_plan([mean, var])
    plan.run()
    plan.check()
    return plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    cases = [(512, "diagonal"), (512, "fullrank"), (1024, "fullrank")]
    for N in args.n:
        for M, qs in cases:
            X, Y, Z = svgp_data(4096, M, 0, dtype=np.float32)
            m = SVGP(X=X, Y=Y, Z=Z, q_shape=qs)
            m.initialize()
            xs = np.linspace(-2.0, 0.5 * M + 2.0, N)[:, None]
            forms = ["fused", "chunked"] + (["generic"] if N * M <= 512 * 100000 else [])
            plans = {f: make_plan(m, xs, f) for f in forms}
            notes = {f: [e[2] for e in p.explain if e[0].startswith("fused streaming prediction")] for f, p in plans.items()}
            times = {f: [] for f in forms}
            for _ in range(args.reps):
                for f in forms:           # alternating: every form sees the same clocks and the same neighbours
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        plans[f].run()
                    torch.cuda.synchronize()
                    times[f].append((time.perf_counter() - t0) * 1e3 / args.iters)
            flop = M * M * N * (2 if qs == "fullrank" else 1)
            for f in forms:
                ms = float(np.median(times[f]))
                print(json.dumps(dict(N=N, M=M, q_shape=qs, form=f, fused_kernel=any(notes[f]), ms=round(ms, 4),
                                      ms_min=round(float(np.min(times[f])), 4), points_per_s=round(N / (ms * 1e-3), 1),
                                      tflops=round(flop / (ms * 1e-3) / 1e12, 2))), flush=True)
            del plans, m
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
