"""Time the bilinear kernel contraction (hb_gram_bilinear_grad) and one evaluation of the exact GP's log marginal
likelihood with its gradient, in ONE process.

    python tools/bench_exact_mll.py [--sizes 8192,100000] [--reps 5] [--iters 3] [--mll-n 100000] [--out profiles/exact_mll_bench.txt]

1. Contraction: N in --sizes, d = 2, ARD lengthscales, S = 17 and 64 pairs, float32 and float64, beside the route the
   products alone can compose: with K_ij (x_ik - x_jk)^2 = x_ik^2 K_ij - 2 x_ik K_ij x_jk + K_ij x_jk^2,
       g[0] = sum_s w_s A_s . (K B_s),
       g[1 + k] = sum_s w_s [ (A_s x_k^2) . (K B_s) - 2 (A_s x_k) . (K (B_s x_k)) + A_s . (K (B_s x_k^2)) ] / ell_k^3
   -- 1 + 2 d hb_gram_matvec products (K B is shared by the three terms; composing term by term would take 3 d + 1), the
   elementwise scalings and 1 + 3 d hb_pcg_dot, every buffer of both forms allocated outside the timed region.  Device
   events around `iters` calls (40 x `iters` for N <= 50000), `reps` rounds ALTERNATING between the two forms; median (min .. max) of the rounds.  The difference between the two results is
   reported per component, relative to the new result: it shows the cancellation of the composed form.
2. One log_marginal_likelihood_and_grad at --mll-n points (svgp_data, float32, 16 probes, rank 64, tol 1e-3) beside the
   condition() solve alone: wall time of each, the solve's iterations, the share of the contraction."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

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


def composed_buffers(X, S, dt):
    """Everything the composed route touches, allocated ONCE outside the timed region as the new kernel's g and ws are:
    the product's workspace, K B, a scaled operand, its product, the coordinate rows x_k and x_k^2 and the dot outputs."""
    N, d = X.shape
    new = lambda: torch.empty((S, N), dtype=dt, device="cuda")
    xk = [X[:, k].contiguous().reshape(1, N) for k in range(d)]
    return dict(gws=torch.empty(max(H.gram_matvec_ws_elems(dt, N, N, S), 1), dtype=dt, device="cuda"), KB=new(), sc=new(), KS=new(),
                xk=xk, xk2=[H.ewise("MUL", [v, v]) for v in xk],
                dots=[torch.empty(S, dtype=torch.float64, device="cuda") for _ in range(1 + 3 * d)])


def composed(X, ell, A, B, bufs):
    """The contraction from products: device work only, no allocation (the 1 + 3 d dot vectors [S] stay on the device)."""
    d = X.shape[1]
    gws, KB, sc, KS, dots = bufs["gws"], bufs["KB"], bufs["sc"], bufs["KS"], bufs["dots"]
    prod = lambda V, out: H.gram_matvec(X, None, ell, V, out=out, ws=gws)
    prod(B, KB)
    H.pcg_dot(A, KB, out=dots[0])
    for k in range(d):
        xk, xk2 = bufs["xk"][k], bufs["xk2"][k]
        H.pcg_dot(H.ewise("MUL", [A, xk2], out=sc), KB, out=dots[1 + 3 * k])
        prod(H.ewise("MUL", [B, xk], out=sc), KS)
        H.pcg_dot(H.ewise("MUL", [A, xk], out=sc), KS, out=dots[2 + 3 * k])
        prod(H.ewise("MUL", [B, xk2], out=sc), KS)
        H.pcg_dot(A, KS, out=dots[3 + 3 * k])
    return dots


def composed_result(dots, w, ell):
    v = [t.cpu().numpy() for t in dots]
    g = [float(w @ v[0])]
    for k in range(len(ell)):
        a, b, c = v[1 + 3 * k:4 + 3 * k]
        g.append(float(w @ (a - 2.0 * b + c)) / ell[k] ** 3)
    return np.array(g)


def contraction_table(lines, sizes, reps, iters):
    rng = np.random.default_rng(0)
    for N in sizes:
        for dt, name in ((torch.float32, "float32"), (torch.float64, "float64")):
            up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(dt).cuda()
            X = up(rng.uniform(0.0, np.sqrt(N / 40.0), (N, 2)))           # about 40 points per squared lengthscale
            ell_h = np.array([0.9, 1.1])
            ell = up(ell_h)
            for S in (17, 64):
                A, B = up(rng.standard_normal((S, N))), up(rng.standard_normal((S, N)))
                w_h = rng.uniform(0.5, 1.5, S) * np.where(np.arange(S) % 3 == 1, -1.0, 1.0)
                w = torch.as_tensor(w_h).cuda()
                g = torch.empty(3, dtype=torch.float64, device="cuda")
                ws = torch.empty(H.gram_bilinear_grad_ws_elems(N, 2), dtype=torch.float64, device="cuda")
                new = lambda: H.gram_bilinear_grad(X, ell, A, B, w, out=g, ws=ws)
                bufs = composed_buffers(X, S, dt)
                old = lambda: composed(X, ell, A, B, bufs)
                t = ab(dict(new=new, composed=old), reps, iters * (1 if N > 50000 else 40))
                torch.cuda.synchronize()
                g_new, g_old = g.cpu().numpy(), composed_result(old(), w_h, ell_h)
                (ma, lo_a, hi_a), (mb, lo_b, hi_b) = stat(t["new"]), stat(t["composed"])
                lines.append("N=%7d %s S=%2d: gram_bilinear_grad %9.3f ms (%.3f .. %.3f) = %.3e evals/s | composed (5 products) "
                             "%9.3f ms (%.3f .. %.3f) | composed / new = %.2f | |composed - new| / |new| per component %s"
                             % (N, name, S, ma, lo_a, hi_a, N * N / (ma * 1e-3), mb, lo_b, hi_b, mb / ma,
                                np.array2string(np.abs(g_old - g_new) / np.abs(g_new), precision=1)))
                print(lines[-1], flush=True)
                del A, B, bufs, ws


def objective(lines, N):
    X, Y, _ = svgp_data(N, 512)
    m = ExactGPR(X=X, Y=Y, dtype="float32")
    m.gp.kern.lengthscales = np.ones(1)
    m.k_var = np.ones(1)
    m.var = np.ones(1) * 0.09
    m.initialize()
    g = lambda k: object.__getattribute__(m, k)
    lines.append("objective: svgp_data(%d, 512), float32, ell=1 k_var=1 noise_var=0.09, tol 1e-3, rank 64, 16 probes" % N)
    for rep in range(2):                      # (the first round also loads the code objects)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = m.fit().posterior.info
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        value, grad, minfo = g("gp").log_marginal_likelihood_and_grad(g("X"), g("Y"), 0.09, k_var=1.0)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        lines.append("  round %d: condition %8.3f s (%d iterations) | log_marginal_likelihood_and_grad %8.3f s (%d iterations, %d "
                     "restarts, lanczos steps %d .. %d) value %.3f logdet %.3f grad ell %.3f k_var %.3f noise_var %.3f"
                     % (rep, t1 - t0, info["iterations"], t2 - t1, minfo["iterations"], minfo["restarts"],
                        minfo["lanczos_steps"].min(), minfo["lanczos_steps"].max(), value, minfo["logdet"],
                        grad["lengthscales"][0], grad["k_var"], grad["noise_var"]))
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="8192,100000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--mll-n", type=int, default=100000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lines = ["device %s; median of %d rounds of %d calls (40 x as many per round for N <= 50000; min .. max), the forms alternating"
             % (H.device_info()[0], args.reps, args.iters)]
    print(lines[0], flush=True)

    def flush():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    contraction_table(lines, [int(s) for s in args.sizes.split(",") if s], args.reps, args.iters)
    flush()
    if args.mll_n:
        objective(lines, args.mll_n)
    flush()


if __name__ == "__main__":
    main()
