"""Time the marginals of C full-rank latent functions from one pass (hb_sgp_predict_multi_f32) against C calls of
hb_sgp_predict_f32, and one natural-gradient step of models.SVGPHetero, in ONE process; write profiles/sgp_predict_multi.txt.

    python tools/bench_predict_multi.py [--N 1000000] [--M 512] [--latents 2 3 10] [--reps 7] [--iters 3]
                                        [--window-ms 300] [--out profiles/sgp_predict_multi.txt]

fp32, d = 1, inducing points on a grid half a lengthscale apart.  Per latent count C (device events around a window of
calls -- as many as fill `window-ms`, at least `iters` -- sized per form from one probe; `reps` rounds, ALTERNATING between
the forms; median and range of the per-call time):
    multi       ONE hb_sgp_predict_multi_f32: the pack launch (C S^T images) and the strip kernel, A = W K formed once
    separate    C calls of hb_sgp_predict_f32(HB_SGP_S_TRIL): a pack launch and a strip kernel each
The outputs are compared bit for bit at this size before anything is timed.  The product count says multi / separate should
tend to (C + 1) / 2 C (one A_strip instead of C); the file records that figure beside the measured one.
    fit_q step  the wall-clock time of SVGPHetero.fit_q(steps=k) minus that of steps=0, over k (float32 session, C = 2):
                one marginals pass, the sites launch, one weighted statistics pass, two float64 tails with their read-backs."""
import argparse
import json
import os
import sys
import time

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


def bench(N, M, C, reps, iters, window_ms):
    rng = np.random.RandomState(C)
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    span = 0.5 * M
    x, z, ell = f32(rng.uniform(0.0, span, (N, 1))), f32(np.linspace(0.0, span, M)[:, None]), f32(np.ones(1))
    frag = torch.empty(2 * M * M, dtype=torch.float32, device="cuda")
    _, W, info = H.cholesky_inverse(H.gram_fwd(z, z, ell, diag_add=1e-3), frag=frag)
    assert int(info.cpu()[0]) == 0
    m = f32(rng.randn(C, M))
    S = f32(np.tril(0.3 * rng.randn(C, M, M) / np.sqrt(M)) + np.eye(M) * rng.uniform(0.2, 0.9, (C, M, 1)))
    assert H.sgp_predict_multi_fused(torch.float32, N, M, 1, C, True)
    ws = torch.empty(H.sgp_predict_multi_ws_elems(torch.float32, N, M, 1, C, True), dtype=torch.float32, device="cuda")
    mean, var, mean1, var1 = (torch.empty((C, N), dtype=torch.float32, device="cuda") for _ in range(4))

    def multi():
        H.sgp_predict_multi(x, z, ell, W, m, S, out=(mean, var), wfrag=frag, ws=ws)

    def separate():
        for c in range(C):
            H.sgp_predict(x, z, ell, W, m[c:c + 1], S[c], s_kind=H.SGP_S_TRIL, out=(mean1[c:c + 1], var1[c:c + 1]), wfrag=frag,
                          ws=ws)

    multi()
    separate()
    torch.cuda.synchronize()
    same = bool(torch.equal(mean, mean1) and torch.equal(var, var1))
    assert same, "hb_sgp_predict_multi does not return the bits of hb_sgp_predict at N=%d M=%d C=%d" % (N, M, C)
    forms = dict(multi=multi, separate=separate)
    for fn in forms.values():              # warm-up: every timed shape, code objects loaded
        fn()
        fn()
    torch.cuda.synchronize()
    calls = {k: max(iters, int(np.ceil(window_ms / max(timed(fn, 2), 1e-3)))) for k, fn in forms.items()}
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():        # alternating: every form sees the same clocks and the same neighbours
            times[k].append(timed(fn, calls[k]))
    row = dict(N=N, M=M, d=1, C=C, calls_per_window=calls, reps=reps, bits_equal=same)
    for k, v in times.items():
        row[k + "_ms"] = round(float(np.median(v)), 3)
        row[k + "_ms_min_max"] = [round(float(np.min(v)), 3), round(float(np.max(v)), 3)]
    row["multi_over_separate"] = round(row["multi_ms"] / row["separate_ms"], 4)
    row["multi_over_separate_per_round"] = [round(a / b, 4) for a, b in zip(times["multi"], times["separate"])]
    row["product_count_ratio"] = round((C + 1.0) / (2.0 * C), 4)
    return row


def fit_q_step(N, M, steps, reps):
    """Wall-clock milliseconds per natural-gradient step of SVGPHetero.fit_q in a float32 session (median over `reps` of
    (time of `steps` steps - time of 0 steps) / steps; tol = 0 so that every step is taken)."""
    from henbun_amd.models import SVGPHetero

    rng = np.random.RandomState(0)
    span = 0.5 * M
    X = rng.uniform(0.0, span, (N, 1))
    sd = 0.1 + 0.4 / (1.0 + np.exp(-(X[:, 0] - 0.5 * span) / (0.1 * span)))
    Y = (np.sin(X[:, 0]) + sd * rng.randn(N))[:, None]
    m = SVGPHetero(X=X.astype(np.float32), Y=Y.astype(np.float32), Z=np.linspace(0.0, span, M)[:, None].astype(np.float32),
                   dtype="float32")
    m.gp.kern.lengthscales = np.ones(1)
    m.k_var = np.ones(1)
    m.initialize()

    def run(k):
        m.reset_q()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.fit_q(steps=k, tol=0.0)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    run(1)
    per = [(run(steps) - run(0)) / steps for _ in range(reps)]
    return dict(N=N, M=M, steps=steps, reps=reps, fit_q_step_ms=round(float(np.median(per)), 2),
                fit_q_step_ms_min_max=[round(float(np.min(per)), 2), round(float(np.max(per)), 2)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000000)
    ap.add_argument("--M", type=int, default=512)
    ap.add_argument("--latents", type=int, nargs="+", default=[2, 3, 10])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--fit-steps", type=int, default=4)
    ap.add_argument("--out", default=os.path.join("profiles", "sgp_predict_multi.txt"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rows = [bench(args.N, args.M, C, args.reps, args.iters, args.window_ms) for C in args.latents]
    fit = fit_q_step(args.N, args.M, args.fit_steps, min(args.reps, 5))
    lines = ["Marginals of C full-rank latent functions from one pass (tools/bench_predict_multi.py) on %s" % H.device_info()[0],
             "fp32, N = %d, M = %d, d = 1; device events around windows of >= %.0f ms, %d alternating rounds, median [min, max] ms per call"
             % (args.N, args.M, args.window_ms, args.reps), ""]
    for r in rows:
        lines.append("C = %d   (multi bits == separate bits: %s; calls per window: %s)" % (r["C"], r["bits_equal"], r["calls_per_window"]))
        for k in ("multi", "separate"):
            lines.append("  %-10s %9.3f  [%.3f, %.3f]" % ((k, r[k + "_ms"]) + tuple(r[k + "_ms_min_max"])))
        lines.append("  multi / separate = %.4f measured (per round %s); (C + 1) / 2 C = %.4f by product count"
                     % (r["multi_over_separate"], r["multi_over_separate_per_round"], r["product_count_ratio"]))
        lines.append("")
    lines.append("SVGPHetero.fit_q, float32 session, N = %d, M = %d: %.2f ms per natural-gradient step [%.2f, %.2f] (wall clock, "
                 "%d steps minus 0 steps, %d rounds)" % ((fit["N"], fit["M"], fit["fit_q_step_ms"]) + tuple(fit["fit_q_step_ms_min_max"])
                                                         + (fit["steps"], fit["reps"])))
    lines.append("")
    for r in rows + [fit]:
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines))
        print("\n".join(lines))


if __name__ == "__main__":
    main()
