"""Time SparseGP.predict_f(full_cov=True): the fused covariance (hb_sgp_predict_cov) against the generic graph composition
(settings.runtime.fused_predict = False: K(x, x), the products of A, the adds as separate launches), in ONE process,
alternating between the forms.

    python tools/bench_predict_cov.py [--n 2048 8192] [--M 512] [--reps 7] [--iters 10]

One JSON line per (case, form): ms per covariance (the whole plan: Gram + Cholesky of z, then the covariance) and the
achieved TF/s on the algorithmic work -- M n^2 flop for the symmetric product (2 M n^2 with a full-rank q(u): A^T A and
C^T C), plus M^2 n for A = W K.  Residual 'fullrank' (what predict_f_samples factorises).  Kernel times come from a
separate run under `rocprofv3 --kernel-trace --stats -- python tools/bench_predict_cov.py ...` (sgp_predict_cov_kernel,
the sgp_A_* kernel of pass 1)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import henbun_amd as hb  # noqa: E402
from henbun_amd.models import SVGP, svgp_data  # noqa: E402


def make_plan(m, xs, form):
    q = object.__getattribute__(m, "u")
    cfg = hb.settings.get_settings()
    cfg.runtime.fused_predict = form == "fused"
    with hb.settings.temp_settings(cfg):
        with m.tf_mode():
            _, cov = m.gp.predict_f(xs, q, q_shape="fullrank", full_cov=True)
        plan = m._session.make_plan([cov])
    plan.run()
    plan.check()
    return plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2048, 8192])
    ap.add_argument("--M", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    M = args.M
    for n in args.n:
        for qs in ("diagonal", "fullrank"):
            X, Y, Z = svgp_data(4096, M, 0, dtype=np.float32)
            m = SVGP(X=X, Y=Y, Z=Z, q_shape=qs)
            m.initialize()
            xs = np.linspace(-2.0, 0.5 * M + 2.0, n)[:, None]
            forms = ["fused", "composed"]
            plans = {f: make_plan(m, xs, f) for f in forms}
            fired = {f: any(e[2] for e in p.explain if e[0].startswith("fused predictive covariance"))
                     for f, p in plans.items()}
            times = {f: [] for f in forms}
            for _ in range(args.reps):
                for f in forms:           # alternating: every form sees the same clocks and the same neighbours
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        plans[f].run()
                    torch.cuda.synchronize()
                    times[f].append((time.perf_counter() - t0) * 1e3 / args.iters)
            flop_sym = M * n * n * (2 if qs == "fullrank" else 1)
            flop_A = M * M * n
            for f in forms:
                ms = float(np.median(times[f]))
                print(json.dumps(dict(n=n, M=M, q_shape=qs, form=f, fused_kernel=fired[f], ms=round(ms, 4),
                                      ms_min=round(float(np.min(times[f])), 4), gflop_sym=round(flop_sym / 1e9, 2),
                                      gflop_A=round(flop_A / 1e9, 2),
                                      tflops=round((flop_sym + flop_A) / (ms * 1e-3) / 1e12, 2))), flush=True)
            del plans, m
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
