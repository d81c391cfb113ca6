"""Time hb_sgp_stats_f32 (the one-pass sufficient statistics of SparseGP.optimal_q / collapsed_bound) in ONE process.

    python tools/bench_sgp_stats.py [--N 65536 1000000] [--M 512 1024] [--reps 7] [--iters 5] [--out profiles/sgp_stats_bench.json]

Per (N, M), after a warm-up of every timed form, `reps` rounds alternate between
    whole   hb_sgp_stats_f32                                       (A pass + SYRK pass + fold + finish)
    a_pass  the same call with the second pass switched off        (hb_debug_set sgp_stats_no_syrk)
    syrk    the same call with the A pass switched off             (sgp_stats_no_A: SYRK + fold on the last chunk's A)
    sgp_A   hb_sgp_A_f32 stand-alone on the same chunks             (the yardstick of the A pass)
each timed with device events around `iters` calls.  Reported: the median and the min / max over the rounds (the
spread), milliseconds per call, and TF/s and the fraction of the fp32 MFMA peak (157.3 TF/s) on the algorithmic flop:
M^2 N for A = W K (W triangular) and M^2 N for the lower triangle of A A^T.  One JSON line per case; --out collects
them in a file.  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python
tools/bench_sgp_stats.py ...` (sgp_stats_syrk_kernel, sgp_stats_fold_kernel, the sgp_A_* kernel of the A pass)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from henbun_amd import hip_ops as H  # noqa: E402

PEAK_TF = 157.3
CHUNK = 32768


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
    ap.add_argument("--N", type=int, nargs="+", default=[65536, 1000000])
    ap.add_argument("--M", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    results = []
    for M in args.M:
        for N in args.N:
            rng = np.random.RandomState(0)
            f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
            X = f32(rng.uniform(0, 0.5 * M, (N, 1)))
            Y = f32(np.sin(X.cpu().numpy()) + 0.3 * rng.randn(N, 1))
            z = f32(np.linspace(0, 0.5 * M, M)[:, None])
            ell = f32(np.ones(1))
            frag = torch.empty(2 * M * M, dtype=torch.float32, device="cuda")
            _, W, info = H.cholesky_inverse(H.gram_fwd(z, z, ell, diag_add=1e-5), frag=frag)
            assert int(info.cpu()[0]) == 0
            ws = torch.empty(H.sgp_stats_ws_elems(torch.float32, N, M, 1, 1), dtype=torch.float32, device="cuda")
            nc = min(CHUNK, (1 << 24) // M)
            Abuf = torch.empty((M, min(nc, N)), dtype=torch.float32, device="cuda")

            def whole():
                H.sgp_stats(X, Y, z, ell, W, wfrag=frag, ws=ws)

            def switched(key):
                def run():
                    H.debug_set(key, 1)
                    try:
                        H.sgp_stats(X, Y, z, ell, W, wfrag=frag, ws=ws)
                    finally:
                        H.debug_clear()
                return run

            def sgp_A():
                for c0 in range(0, N, nc):
                    n = min(nc, N - c0)
                    H.sgp_A(X[c0:c0 + n], z, ell, W, out=Abuf.view(-1)[:M * n].view(M, n), wfrag=frag)

            forms = {"whole": whole, "a_pass": switched("sgp_stats_no_syrk"), "syrk": switched("sgp_stats_no_A"),
                     "sgp_A": sgp_A}
            for fn in forms.values():           # warm-up: every timed shape, code objects loaded
                fn()
                fn()
            torch.cuda.synchronize()
            times = {k: [] for k in forms}
            for _ in range(args.reps):
                for k, fn in forms.items():     # alternating: every form sees the same clocks and the same neighbours
                    times[k].append(timed(fn, args.iters))
            flop = float(M) * M * N
            row = dict(N=N, M=M, iters=args.iters, reps=args.reps, gflop_each_pass=round(flop / 1e9, 2))
            for k, v in times.items():
                ms = float(np.median(v))
                row[k + "_ms"] = round(ms, 4)
                row[k + "_ms_min_max"] = [round(float(np.min(v)), 4), round(float(np.max(v)), 4)]
                tf = (2 * flop if k == "whole" else flop) / (ms * 1e-3) / 1e12
                row[k + "_tflops"] = round(tf, 2)
                row[k + "_of_peak"] = round(tf / PEAK_TF, 3)
            row["a_pass_us_per_1k_columns"] = round(row["a_pass_ms"] * 1e3 / (N / 1000.0), 3)
            row["sgp_A_us_per_1k_columns"] = round(row["sgp_A_ms"] * 1e3 / (N / 1000.0), 3)
            print(json.dumps(row), flush=True)
            results.append(row)
            del X, Y, ws, Abuf
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=H.device_info()[0], peak_fp32_mfma_tflops=PEAK_TF, results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
