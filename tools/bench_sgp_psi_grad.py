"""Time the gradients of the psi statistics against the statistics themselves, in ONE process.

    python tools/bench_sgp_psi_grad.py [--N 100000 1000000] [--M 128 512] [--d 1 2] [--extra 6:128] [--reps 3]
                                       [--out profiles/sgp_psi_grad.txt]

Per (N, M, d) of tools/bench_sgp_psi.py, plus d = 6 at M = 128 (`--extra d:M`, the loop form: a latent space of the common
size), float32 storage, after a warm-up of every timed form, `reps` rounds alternate between
    stats    hb_sgp_psi_stats_f32    (psi2 partial tiles + psi1 partials + fold)
    grad     hb_sgp_psi_grad_f32     (pair-major passes + fold, then the point-major pass + fold per chunk of points)
each timed with device events around one call.  Reported: the median and min / max over the rounds in milliseconds, their
ratio, and the pair-evaluations per second of grad counted as 2 N M (M + 1) / 2 (two passes of one exponential per point
and pair; the exponentials a loop form repeats per block of dimensions are not counted).  Q and R are those of the collapsed
bound's tail at jitter 1e-3 on the same data.

Then one models.BayesianGPLVM.bound_and_grad() at N = 10^4, M = 64, Q = 6, P = 12 (`--gplvm N M Q P`), wall clock around the
call with a device synchronisation, after one warm-up call: the median and min / max of `reps` calls."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import henbun_amd as hb  # noqa: E402
from henbun_amd import hip_ops as H  # noqa: E402
from henbun_amd.models import BayesianGPLVM  # noqa: E402

from bench_sgp_psi import rounds  # noqa: E402


def tail_weights(X, V, Y, z, ell, jitter=1e-3, s2=0.09):
    """(Q, R) of the collapsed bound at k_var = 1 from float32-stored inputs, float64 on the device"""
    z64, ell64 = z.double(), ell.double()
    L, info = H.cholesky(H.gram_fwd(z64, z64, ell64, diag_add=jitter))
    assert int(info.cpu()[0]) == 0
    W = H.trinv(L)
    Psi2, C, _ = H.sgp_psi_stats(X, V, Y, z, ell)
    Phi = H.matutil(H.matmul(W, H.matmul(Psi2, W, transB=True)), H.MATUTIL_SYM)
    b = H.matmul(C, W, transB=True)
    M, P = z.shape[0], Y.shape[1]
    Lam = torch.eye(M, dtype=torch.float64, device="cuda") + Phi / s2
    Li = torch.linalg.inv(Lam)
    m = (b / s2) @ Li
    G = (-0.5 * m.t() @ m - 0.5 * P * Li) / s2 + (P / (2.0 * s2)) * torch.eye(M, dtype=torch.float64, device="cuda")
    Q = 2.0 * W.t() @ G @ W
    return (0.5 * (Q + Q.t())).contiguous(), (W.t() @ (m / s2).t()).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--M", type=int, nargs="+", default=[128, 512])
    ap.add_argument("--d", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--extra", nargs="*", default=["6:128"])
    ap.add_argument("--gplvm", type=int, nargs=4, default=[10000, 64, 6, 12])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lines = ["gradients of the psi statistics (tools/bench_sgp_psi_grad.py) on %s; float32 storage, double arithmetic; device "
             "events, median [min, max] of %d alternating rounds" % (H.device_info()[0], args.reps)]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    shapes = [(d, M) for d in args.d for M in args.M] + [tuple(int(v) for v in e.split(":")) for e in args.extra]
    for d, M in shapes:
        rng = np.random.RandomState(0)
        side = 0.5 * M if d == 1 else 0.5 * M ** (1.0 / min(d, 2))        # as tools/bench_sgp_psi.py
        z = f32(np.linspace(0, side, M)[:, None] if d == 1 else rng.uniform(0, side, (M, d)))
        ell = f32(np.ones(d))
        for N in args.N:
            X = f32(rng.uniform(0, side, (N, d)))
            V = f32(rng.uniform(0, 0.36, (N, d)))
            Y = f32(np.sin(X.cpu().numpy().sum(1, keepdims=True)) + 0.3 * rng.randn(N, 1))
            Q, R = tail_weights(X, V, Y, z, ell)
            ws = torch.empty(H.sgp_psi_stats_ws_elems(torch.float32, N, M, d, 1), dtype=torch.float32, device="cuda")
            wg = torch.empty(H.sgp_psi_grad_ws_elems(torch.float32, N, M, d, 1), dtype=torch.float32, device="cuda")
            t = rounds({"stats": lambda: H.sgp_psi_stats(X, V, Y, z, ell, ws=ws),
                        "grad": lambda: H.sgp_psi_grad(X, V, Y, z, ell, Q, R, ws=wg)}, args.reps)
            rate = 2.0 * N * M * (M + 1) / 2.0 / (t["grad"][0] * 1e-3)
            say("N=%d M=%d d=%d: stats %.3f ms [%.3f, %.3f]; grad %.3f ms [%.3f, %.3f]; grad / stats %.2f x; grad %.1f G "
                "pair-evaluations / s" % ((N, M, d) + t["stats"] + t["grad"] + (t["grad"][0] / t["stats"][0], rate / 1e9)))
            del X, V, Y, ws, wg
            torch.cuda.empty_cache()
    N, M, Qd, P = args.gplvm
    rng = np.random.RandomState(1)
    lat = rng.randn(N, 2)
    Yg = np.stack([np.sin(lat[:, 0] * (1 + 0.1 * p) + p) + np.cos(lat[:, 1] - 0.2 * p) for p in range(P)], 1) + 0.1 * rng.randn(N, P)
    cfg = hb.settings.get_settings()
    cfg.numerics.jitter_level = 1e-3
    with hb.settings.temp_settings(cfg):
        m = BayesianGPLVM(Y=Yg, latent_dim=Qd, M=M, dtype="float32")
        m.initialize()
        m.bound_and_grad()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            val, _ = m.bound_and_grad()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
    say("BayesianGPLVM.bound_and_grad() N=%d M=%d Q=%d P=%d (float32 session): %.2f ms [%.2f, %.2f] wall clock; bound %.4f"
        % (N, M, Qd, P, float(np.median(ts)), min(ts), max(ts), val))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
