"""Time the psi statistics (uncertain inputs) in ONE process.

    python tools/bench_sgp_psi.py [--N 100000 1000000] [--M 128 512] [--d 1 2] [--reps 3] [--out profiles/sgp_psi.txt]

Per (N, M, d), float32 storage, after a warm-up of every timed form, `reps` rounds alternate between
    psi      hb_sgp_psi_stats_f32                       (psi2 partial tiles + psi1 partials + fold)
    certain  the float64 certain-input statistics on the same sizes, in the composition of SparseGP._statistics_f64:
             row chunks up-converted, hb_sgp_A_f64, three hb_matmul_f64, the chunks' results added in chunk order
each timed with device events around one call.  Reported: the median and min / max over the rounds in milliseconds, the
pair-evaluations per second of psi (N M (M + 1) / 2 per call: what the algorithm needs, the register blocks above the
diagonal that a diagonal tile still evaluates not counted), and its share of the ceiling.

The ceiling is measured here and independently of the library: a bare double-exp loop (tools/exp_ceiling.hip, built into
tools/_bin/ on first use; one fma, one exp, one add per evaluation, 16 independent sums per thread), as evaluations per
second, alternated with itself over `reps` rounds.

Then hb_sgp_psi_predict_f32 at n = 1 and 10^4 (M, d as above), the same way: milliseconds and pair-evaluations per second."""
import argparse
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from henbun_amd import hip_ops as H  # noqa: E402
from henbun_amd.gp import _host  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def rounds(forms, reps):
    for fn in forms.values():            # warm-up: every timed shape, code objects loaded
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():      # alternating: every form sees the same clocks and the same neighbours
            times[k].append(timed(fn))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in times.items()}


def exp_ceiling(reps):
    """evaluations per second of the bare double-exp loop"""
    src, out = os.path.join(ROOT, "tools", "exp_ceiling.hip"), os.path.join(ROOT, "tools", "_bin", "libexp_ceiling.so")
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.run(["hipcc", "-O3", "-fPIC", "-shared", "--offload-arch=gfx950", src, "-o", out], check=True)
    lib = ctypes.CDLL(out)
    lib.exp_ceiling_launch.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_long, ctypes.c_void_p, ctypes.c_long,
                                       ctypes.c_void_p]
    blocks, iters = 4096, 2048
    base = torch.as_tensor(np.random.RandomState(0).uniform(-3.0, 0.0, 1024)).cuda()
    sink = torch.empty(blocks * 256, dtype=torch.float64, device="cuda")

    def run():
        rc = lib.exp_ceiling_launch(base.data_ptr(), -1e-3, iters, sink.data_ptr(), blocks, H.stream())
        assert rc == 0, rc

    ms, lo, hi = rounds({"exp": run}, reps)["exp"]
    evals = blocks * 256 * 16 * iters
    assert bool(torch.isfinite(sink).all().cpu())
    return evals / (ms * 1e-3), evals, (ms, lo, hi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--M", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--d", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--n", type=int, nargs="+", default=[1, 10000])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lines = ["psi statistics (tools/bench_sgp_psi.py) on %s; float32 storage, double arithmetic; device events, median "
             "[min, max] of %d alternating rounds" % (H.device_info()[0], args.reps)]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    ceil_rate, evals, (ms, lo, hi) = exp_ceiling(max(args.reps, 5))
    say("ceiling: bare double-exp loop, %.3g evaluations in %.3f ms [%.3f, %.3f] = %.1f G evaluations / s"
        % (evals, ms, lo, hi, ceil_rate / 1e9))
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    for d in args.d:
        for M in args.M:
            rng = np.random.RandomState(0)
            side = 0.5 * M if d == 1 else 0.5 * np.sqrt(M)            # inducing points about half a lengthscale apart
            z = f32(np.linspace(0, side, M)[:, None] if d == 1 else rng.uniform(0, side, (M, d)))
            ell = f32(np.ones(d))
            z64, ell64 = z.double(), ell.double()
            L, info = H.cholesky(H.gram_fwd(z64, z64, ell64, diag_add=1e-3))
            assert int(info.cpu()[0]) == 0
            W64 = H.trinv(L)
            for N in args.N:
                X = f32(rng.uniform(0, side, (N, d)))
                V = f32(rng.uniform(0, 0.36, (N, d)))
                Y = f32(np.sin(X.cpu().numpy().sum(1, keepdims=True)) + 0.3 * rng.randn(N, 1))
                ws = torch.empty(H.sgp_psi_stats_ws_elems(torch.float32, N, M, d, 1), dtype=torch.float32, device="cuda")
                chunk = _host.f64_chunk_rows(M)

                def psi():
                    H.sgp_psi_stats(X, V, Y, z, ell, ws=ws)

                def certain():
                    total = None
                    for c0 in range(0, N, chunk):
                        Xc, Yc = X[c0:c0 + chunk].double().contiguous(), Y[c0:c0 + chunk].double().contiguous()
                        A = H.sgp_A(Xc, z64, ell64, W64)
                        parts = (H.matmul(A, A, transB=True), H.matmul(Yc, A, transA=True, transB=True),
                                 H.matmul(Yc, Yc, transA=True))
                        total = parts if total is None else tuple(a + b for a, b in zip(total, parts))
                    return total

                t = rounds({"psi": psi, "certain": certain}, args.reps)
                pairs = N * M * (M + 1) / 2.0
                rate = pairs / (t["psi"][0] * 1e-3)
                say("stats N=%d M=%d d=%d: psi %.3f ms [%.3f, %.3f]; certain (float64) %.3f ms [%.3f, %.3f]; psi / certain "
                    "%.1f x; %.1f G pair-evaluations / s = %.0f %% of the ceiling"
                    % ((N, M, d) + t["psi"] + t["certain"] + (t["psi"][0] / t["certain"][0], rate / 1e9,
                                                               100.0 * rate / ceil_rate)))
                del X, V, Y, ws
                torch.cuda.empty_cache()
            beta = torch.as_tensor(rng.randn(M)).cuda()
            Q = torch.as_tensor(rng.randn(M, M)).cuda()
            Q = (Q + Q.t()).contiguous()
            for n in args.n:
                X = f32(rng.uniform(0, side, (n, d)))
                V = f32(rng.uniform(0, 0.36, (n, d)))
                ws = torch.empty(H.sgp_psi_predict_ws_elems(torch.float32, n, M, d), dtype=torch.float32, device="cuda")
                ms, lo, hi = rounds({"p": lambda: H.sgp_psi_predict(X, V, z, ell, beta, Q, ws=ws)}, max(args.reps, 5))["p"]
                say("predict n=%d M=%d d=%d: %.4f ms [%.4f, %.4f]; %.2f G pair-evaluations / s"
                    % (n, M, d, ms, lo, hi, n * M * (M + 1) / 2.0 / (ms * 1e-3) / 1e9))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
