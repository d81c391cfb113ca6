"""Time the matrix-free kernel product (hb_gram_matvec) and the exact-GP solve built on it, in ONE process.

    python tools/bench_gram_matvec.py [--sizes 8192,100000] [--reps 5] [--iters 3] [--solve-n 100000] [--big-n 1000000]
                                      [--out profiles/exact_gp_bench.txt]

1. Product: kernel evaluations per second (n N per call) at n = N in --sizes, S = 1, 16, 64, float32 and float64, d = 2,
   beside the baseline: hb_sgp_pathwise with L = 1, M = N on the same points -- the same synthesis and the same MFMA
   contraction with every row in one workgroup (no row chunks, two trig rows more).  Device events around `iters` calls
   (40 x `iters` for N <= 50000, where a call is a fraction of a millisecond),
   `reps` rounds ALTERNATING between the two forms; median (min .. max) of the rounds.
2. Against the materialised route at N = 16384, float32, S = 16: hb_gram_fwd once plus hb_matmul per product, beside the
   matrix-free product; totals for k = 1 and k = 50 products.
3. Solve: svgp_data(--solve-n, 512), float32, ell = 1, k_var = 1, noise_var = 0.09, tol 1e-3, at ranks 0 / 16 / 64 / 128:
   iterations, wall time (preconditioner included), true residual.  One product at --big-n rows is timed as well (the
   cost of ONE iteration there; 0 skips it).
4. The float32 residual floor on the 600-point case of tests/exact_gp_ref.py: the smallest tol of a descending ladder
   that still converges within 1000 iterations at rank 64."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import henbun_amd as hb  # noqa: E402
from henbun_amd import hip_ops as H  # noqa: E402
from henbun_amd.models import ExactGPR, svgp_data  # noqa: E402


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


def stat(ts):
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def product_table(lines, sizes, reps, iters):
    rng = np.random.default_rng(0)
    for N in sizes:
        for dt, name in ((torch.float32, "float32"), (torch.float64, "float64")):
            up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dt).cuda()
            X = up(rng.uniform(0.0, np.sqrt(N / 40.0), (N, 2)))           # about 40 points per squared lengthscale
            ell, omega = up(np.ones(1)), up(rng.standard_normal((1, 2)))
            for S in (1, 16, 64):
                V = up(rng.standard_normal((S, N)))
                coef = torch.cat([torch.zeros((S, 2), dtype=dt, device="cuda"), V], dim=1).contiguous()
                out_a, out_b = torch.empty((S, N), dtype=dt, device="cuda"), torch.empty((S, N), dtype=dt, device="cuda")
                ws = torch.empty(max(H.gram_matvec_ws_elems(dt, N, N, S), 1), dtype=dt, device="cuda")
                forms = dict(matvec=lambda: H.gram_matvec(X, X, ell, V, out=out_a, ws=ws),
                             pathwise=lambda: H.sgp_pathwise(X, omega, X, ell, coef, out=out_b))
                t = ab(forms, reps, iters * (1 if N > 50000 else 40))      # sub-millisecond calls: 40 x as many per round
                torch.cuda.synchronize()
                diff = float((out_a - out_b).abs().max() / out_b.abs().max())
                (ma, lo_a, hi_a), (mb, lo_b, hi_b) = stat(t["matvec"]), stat(t["pathwise"])
                lines.append("N=%7d %s S=%2d: gram_matvec %9.3f ms (%.3f .. %.3f) = %.3e evals/s | pathwise L=1 M=N %9.3f ms "
                             "(%.3f .. %.3f) = %.3e evals/s | baseline / new = %.2f | max diff %.1e of max|out|"
                             % (N, name, S, ma, lo_a, hi_a, N * N / (ma * 1e-3), mb, lo_b, hi_b, N * N / (mb * 1e-3), mb / ma, diff))
                print(lines[-1], flush=True)
                del V, coef, out_a, out_b, ws


def materialised(lines, reps, iters, N=16384, S=16):
    rng = np.random.default_rng(1)
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    X, ell, V = up(rng.uniform(0.0, np.sqrt(N / 40.0), (N, 2))), up(np.ones(1)), up(rng.standard_normal((S, N)))
    K = torch.empty((N, N), dtype=torch.float32, device="cuda")
    o1, o2 = torch.empty((S, N), dtype=torch.float32, device="cuda"), torch.empty((S, N), dtype=torch.float32, device="cuda")
    ws = torch.empty(max(H.gram_matvec_ws_elems(torch.float32, N, N, S), 1), dtype=torch.float32, device="cuda")
    t = ab(dict(gram=lambda: H.gram_fwd(X, X, ell, out=K), matmul=lambda: H.matmul(V, K, out=o1),
                matvec=lambda: H.gram_matvec(X, None, ell, V, out=o2, ws=ws)), reps, 10 * iters)
    g, mm, mv = (stat(t[k])[0] for k in ("gram", "matmul", "matvec"))
    lines.append("N=%d float32 S=%d: hb_gram_fwd %.3f ms (K is %.2f GB), hb_matmul %.3f ms per product, hb_gram_matvec %.3f ms "
                 "per product" % (N, S, g, 4.0 * N * N / 1e9, mm, mv))
    for k in (1, 50):
        lines.append("  k=%2d products: materialised %.3f ms, matrix-free %.3f ms" % (k, g + k * mm, k * mv))
    print("\n".join(lines[-3:]), flush=True)


def solves(lines, N, big_n):
    X, Y, _ = svgp_data(N, 512)
    m = ExactGPR(X=X, Y=Y, dtype="float32")
    m.gp.kern.lengthscales = np.ones(1)
    m.k_var = np.ones(1)
    m.var = np.ones(1) * 0.09
    m.initialize()
    lines.append("solve: svgp_data(%d, 512), float32, ell=1 k_var=1 noise_var=0.09, tol 1e-3, max_iter 3000" % N)
    for rank in (0, 16, 64, 128, 0):          # (the first solve also loads the code objects: rank 0 is timed again)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            info = m.fit(precond_rank=rank, max_iter=3000).posterior.info
        except hb.gp.NotConverged as e:
            info = e.info
        torch.cuda.synchronize()
        lines.append("  rank %3d (used %3d): %4d iterations, %8.3f s wall, true residual %.3e, converged %s"
                     % (rank, info["precond_rank"], info["iterations"], time.perf_counter() - t0, float(info["residual"].max()),
                        info["converged"]))
        print(lines[-1], flush=True)
    if big_n:
        Xb = torch.as_tensor(svgp_data(big_n, 512)[0].astype(np.float32)).cuda()
        V = torch.ones((1, big_n), dtype=torch.float32, device="cuda")
        ell = torch.ones(1, dtype=torch.float32, device="cuda")
        out = torch.empty_like(V)
        ws = torch.empty(H.gram_matvec_ws_elems(torch.float32, big_n, big_n, 1), dtype=torch.float32, device="cuda")
        fn = lambda: H.gram_matvec(Xb, None, ell, V, out=out, ws=ws)
        fn()
        ms = timed(fn, 2)
        lines.append("one product at N=%d, S=1, d=1, float32: %.1f ms = %.3e evals/s (ONE iteration of a solve there; the solve "
                     "itself was not run)" % (big_n, ms, float(big_n) ** 2 / (ms * 1e-3)))
        print(lines[-1], flush=True)


def residual_floor(lines):
    import exact_gp_ref as E

    X, Y, ell, k_var, noise_var = E.plane_case()
    m = ExactGPR(X=X, Y=Y, dtype="float32")
    m.gp.kern.lengthscales = ell.copy()
    m.k_var = np.ones(1) * k_var
    m.var = np.ones(1) * noise_var
    m.initialize()
    lines.append("float32 residual floor, 600-point case, rank 64, max_iter 1000:")
    for tol in (1e-3, 3e-4, 1e-4, 3e-5, 1e-5, 3e-6, 1e-6, 3e-7):
        try:
            info = m.fit(tol=tol).posterior.info
        except hb.gp.NotConverged as e:
            info = e.info
        lines.append("  tol %.0e: %4d iterations, true residual %.3e, converged %s"
                     % (tol, info["iterations"], float(info["residual"].max()), info["converged"]))
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,100000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--solve-n", type=int, default=100000)
    ap.add_argument("--big-n", type=int, default=1000000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lines = ["device %s; GMV_CHUNK = %d; median of %d rounds of %d calls (40 x as many per round for N <= 50000, 10 x for the materialised route; min .. max), the forms alternating"
             % (H.device_info()[0], H.gram_matvec_chunk(), args.reps, args.iters)]
    print(lines[0], flush=True)

    def flush():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    residual_floor(lines)
    flush()
    product_table(lines, [int(s) for s in args.sizes.split(",") if s], args.reps, args.iters)
    flush()
    materialised(lines, args.reps, args.iters)
    flush()
    if args.solve_n:
        solves(lines, args.solve_n, args.big_n)
    flush()


if __name__ == "__main__":
    main()
