"""Time the evaluation of pathwise posterior function draws (hb_sgp_pathwise_f32) in ONE process.

    python tools/bench_sgp_pathwise.py [--N 1000000] [--M 512] [--L 1024] [--reps 7] [--iters 5] [--out profiles/pathwise_bench.txt]

Forms, fp32, d = 1 (device events around `iters` calls; `reps` rounds, ALTERNATING between the forms; the median is
reported): S = 1, 16, 64 draws at N points.  Per form: ms per call; basis values per second ((2L + M) N per call: every one
is a sincos half or an exp2, synthesised once whatever S); MFMA TFLOP/s as issued (2 (2L + M) N S16, S16 = S rounded up to
the 16-row tile) and useful (the same with S), against the two ceilings of the chip: the fp32 MFMA rate (157.3 TF) and the
HBM rate for the bytes that must move (x read, out written; 8 TB/s spec, 6.3 TB/s achievable).
Then, at the one point where the joint route can run at all (n = 4096, S = 16, float32 session): SVGP.predict_f_samples
(cholesky of the [n, n] covariance; jitter 1e-3, then 1e-2, as a dense grid needs in fp32) beside
SVGP.sample_functions(...)(X); host clock around a synchronise, after a warm-up call, each call as the API makes it
(predict_f_samples builds its plan per call)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import henbun_amd as hb  # noqa: E402
from henbun_amd import hip_ops as H  # noqa: E402
from henbun_amd.models import SVGP, svgp_data  # noqa: E402

MFMA_F32_TF, HBM_SPEC_TBS = 157.3, 8.0


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
    ap.add_argument("--N", type=int, default=1000000)
    ap.add_argument("--M", type=int, default=512)
    ap.add_argument("--L", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--joint-n", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, M, L = args.N, args.M, args.L
    torch.cuda.set_device(0)
    rng = np.random.default_rng(0)
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    X = f32(rng.uniform(0, 0.5 * M, (N, 1)))
    z, ell, omega = f32(np.linspace(0, 0.5 * M, M)[:, None]), f32(np.ones(1)), f32(rng.standard_normal((L, 1)))
    draws = (1, 16, 64)
    coef, out = {}, {}
    for S in draws:
        c = rng.standard_normal((S, 2 * L + M))
        c[:, 2 * L:] *= 1e3
        coef[S], out[S] = f32(c), torch.empty((S, N), dtype=torch.float32, device="cuda")
    forms = {S: (lambda S=S: H.sgp_pathwise(X, omega, z, ell, coef[S], scale=1.3, out=out[S])) for S in draws}
    for fn in forms.values():              # warm-up: every timed shape, code objects loaded
        fn()
        fn()
    torch.cuda.synchronize()
    times = {S: [] for S in draws}
    for _ in range(args.reps):
        for S, fn in forms.items():        # alternating: every form sees the same clocks and the same neighbours
            times[S].append(timed(fn, args.iters))
    lines = ["device %s; hb_sgp_pathwise_f32, N=%d M=%d L=%d d=1; median of %d rounds of %d calls (min .. max)"
             % (H.device_info()[0], N, M, L, args.reps, args.iters)]
    rows = []
    K = 2 * L + M
    for S in draws:
        ms = float(np.median(times[S]))
        S16 = 16 * ((S + 15) // 16)
        row = dict(S=S, ms=round(ms, 4), ms_min_max=[round(float(np.min(times[S])), 4), round(float(np.max(times[S])), 4)],
                   basis_values_per_s=K * N / (ms * 1e-3), mfma_tf_issued=2.0 * K * N * S16 / (ms * 1e-3) / 1e12,
                   mfma_tf_useful=2.0 * K * N * S / (ms * 1e-3) / 1e12, hbm_tb_per_s=4.0 * N * (1 + S) / (ms * 1e-3) / 1e12)
        rows.append(row)
        lines.append("S=%2d: %8.3f ms (%.3f .. %.3f)  basis %.3e values/s  MFMA %.1f TF issued = %.0f %% of %.1f (useful %.1f)  "
                     "HBM %.3f TB/s = %.1f %% of %.1f"
                     % (S, ms, row["ms_min_max"][0], row["ms_min_max"][1], row["basis_values_per_s"], row["mfma_tf_issued"],
                        100 * row["mfma_tf_issued"] / MFMA_F32_TF, MFMA_F32_TF, row["mfma_tf_useful"], row["hbm_tb_per_s"],
                        100 * row["hbm_tb_per_s"] / HBM_SPEC_TBS, HBM_SPEC_TBS))
    lines.append("S = 1 -> 16: x %.2f;  S = 16 -> 64: x %.2f  (the basis is synthesised once whatever S)"
                 % (rows[1]["ms"] / rows[0]["ms"], rows[2]["ms"] / rows[1]["ms"]))

    # the joint route at the one size it can run: n = 4096, S = 16.  Its Cholesky of the [n, n] covariance needs extra
    # jitter on a grid this dense in fp32: the levels are tried in turn and every outcome is reported
    n, S = args.joint_n, 16
    Xh, Yh, Zh = svgp_data(20000, M)
    grid = np.linspace(0.0, 0.5 * M, n)[:, None]
    walls = {}

    def wall(name, fn):
        try:
            fn()                           # warm-up: code objects loaded
        except hb.graph.CholeskyError as e:
            lines.append("n=%d S=%d float32 session: %-42s failed: %s" % (n, S, name, e))
            return
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        assert r.shape == (S, n) and np.all(np.isfinite(r))
        walls[name] = float(np.median(ts))
        lines.append("n=%d S=%d float32 session: %-42s %9.3f ms wall (median of %d, to numpy)" % (n, S, name, walls[name], args.reps))

    for jitter in (1e-3, 1e-2):
        cfg = hb.settings.get_settings()
        cfg.numerics.jitter_level = jitter
        with hb.settings.temp_settings(cfg):
            # (residual 'fullrank' is the covariance the pathwise draws carry; it has no closed-form fit_q, and the time
            # of neither route depends on q, so q(u) stays as initialised)
            model = SVGP(X=Xh, Y=Yh, Z=Zh, q_shape="fullrank", residual="fullrank", dtype="float32")
            model.initialize()
            wall("predict_f_samples, jitter %g" % jitter, lambda: model.predict_f_samples(grid, S))
            if jitter == 1e-3:
                wall("sample_functions + evaluate", lambda: model.sample_functions(S, num_features=L)(grid))
                draws16 = model.sample_functions(S, num_features=L)
                wall("evaluate alone", lambda: draws16(grid))
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    print(json.dumps(dict(N=N, M=M, L=L, rows=rows, joint=walls)), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
