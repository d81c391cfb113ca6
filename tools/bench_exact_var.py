"""Time the exact GP's cached predictive variance against the solve route, in ONE process.

    python tools/bench_exact_var.py [--N 100000] [--n 100000] [--ranks 64,256] [--reps 5] [--iters 3]
                                    [--out profiles/exact_var_cache.txt]

Data: X ~ U(0, sqrt(N / 40))^2 (about 40 points per squared lengthscale), Y = sin(sum x) + 0.3 noise, ell = 1, k_var = 1,
noise_var = 0.09, float32 session, ExactGPR.fit() at its defaults.  For each rank r:
1. build_cache(rank=r): wall time (synchronised), the rows produced, the jitter that factorised.
2. hb_gram_predict over n candidates, V = [alpha; R_c]: mean + variance, and the EI arg-max alone, beside hb_gram_matvec of
   the mean alone (S = 1).  Device events around `iters` calls, `reps` rounds ALTERNATING between the forms; median
   (min .. max) of the rounds.
3. max(v_cache - v_exact) on 64 of the candidates, v_exact from predict_f(var=True): ONE lockstep solve, whose wall time
   is reported per point.
No speed ratio is a pass condition: the numbers are recorded, not promised."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from henbun_amd import hip_ops as H  # noqa: E402
from henbun_amd.models import ExactGPR  # noqa: E402


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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100000)
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--ranks", default="64,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_var_cache.txt"))
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    side = float(np.sqrt(a.N / 40.0))
    X = rng.uniform(0.0, side, (a.N, 2))
    Y = np.sin(X.sum(1, keepdims=True)) + 0.3 * rng.standard_normal((a.N, 1))
    Xc = rng.uniform(0.0, side, (a.n, 2))
    m = ExactGPR(X=X, Y=Y, dtype="float32")
    m.gp.kern.lengthscales = np.ones(1)
    m.k_var = np.ones(1)
    m.var = np.ones(1) * 0.09
    _, t_fit = wall(m.fit)
    post = object.__getattribute__(m, "posterior")
    lines = ["exact GP, cached predictive variance: N = %d, n = %d candidates, d = 2, side %.1f lengthscales, float32 (%s)"
             % (a.N, a.n, side, torch.cuda.get_device_name(0)),
             "fit (rank-64 preconditioner, tol 1e-3): %.2f s, %d iterations" % (t_fit, post.info["iterations"])]
    (_, v_exact), t_solve = wall(lambda: post.predict_f(Xc[:64], var=True))
    lines.append("predict_f(var=True) on 64 points: %.3f s, one solve = %.2f ms per point" % (t_solve, 1e3 * t_solve / 64))
    Xd = post._new_points(Xc)
    out_m = torch.empty((1, a.n), dtype=torch.float32, device="cuda")
    gws = torch.empty(max(H.gram_matvec_ws_elems(torch.float32, a.n, a.N, 1), 1), dtype=torch.float32, device="cuda")
    med = lambda ts: "%8.2f ms (%.2f .. %.2f)" % (np.median(ts), np.min(ts), np.max(ts))
    for rank in [int(r) for r in a.ranks.split(",")]:
        _, t_build = wall(lambda: post.build_cache(rank=rank))
        info = post.cache_info
        V, kv = post._V, post.k_var
        forms = dict(
            mean_only=lambda: H.gram_matvec(Xd, post._X, post._ell, post._alpha, scale=kv, out=out_m, ws=gws),
            predict=lambda: H.gram_predict(Xd, post._X, post._ell, V, scale=kv, prior=kv),
            argmax=lambda: H.gram_predict(Xd, post._X, post._ell, V, scale=kv, prior=kv, acq="ei", best=1.0, var_floor=1e-5,
                                          mean=False, var=False, argmax=True))
        t = ab(forms, a.reps, a.iters)
        _, v_cache = post.predict_f(Xc[:64], var="cache")
        gap = v_cache.astype(np.float64) - v_exact.astype(np.float64)
        lines += ["rank %d -> %d rows (jitter %.0e): build_cache %.2f s" % (rank, info["rank"], info["jitter"], t_build),
                  "    mean alone (hb_gram_matvec, S = 1)      %s" % med(t["mean_only"]),
                  "    mean + cached variance (hb_gram_predict) %s = %.3f us per point" % (med(t["predict"]),
                                                                                          1e3 * np.median(t["predict"]) / a.n),
                  "    EI arg-max alone (hb_gram_predict)       %s" % med(t["argmax"]),
                  "    v_cache - v_exact on 64 points: min %.3e, max %.3e (v_exact in [%.3g, %.3g])"
                  % (gap.min(), gap.max(), v_exact.min(), v_exact.max())]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
