"""CPU study behind the precision decision of hb_sgp_stats_f32 (csrc/sgp_stats.hip): is a float32 A = Lm^-1 K(z, X), with
float32 products over bounded column blocks summed in float64, good enough for the closed-form optimal q(u)?

    python tools/sgp_stats_errors.py [--N 100000] [--M 128] [--jitter 1e-5] [--out profiles/sgp_stats_errors.txt]

Compares, on the svgp_data set, the all-float64 statistics with (a) the float32 form of the kernel (float32 Cholesky
factor, float32 A, float32 block products of at most --ksplit columns, float64 sum) and (b) the same with the block sums
ALSO kept in float32 (what the double outputs avoid): min eig(Lambda), the optimal mean, the predictive mean / variance
on a grid -- each q* evaluated through the A of its own precision, as the model that owns it would -- and the bound."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import optimal_q_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100000)
    ap.add_argument("--M", type=int, default=128)
    ap.add_argument("--jitter", type=float, default=1e-5)
    ap.add_argument("--ksplit", type=int, default=432)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, M, jit = args.N, args.M, args.jitter
    rng = np.random.RandomState(0)
    dom = 0.5 * M
    X = rng.uniform(0, dom, (N, 1))
    Y = np.sin(X) + 0.3 * rng.randn(N, 1)
    z = np.linspace(0, dom, M)[:, None]
    ell = np.ones(1)
    xs = np.linspace(-1.0, dom + 1.0, 400)[:, None]
    lines = ["sgp_stats precision study (tools/sgp_stats_errors.py): N=%d M=%d jitter=%g ksplit=%d, svgp_data" % (N, M, jit, args.ksplit)]

    _, W64 = R.chol_factor(z, ell, jit)
    s64 = R.stats_from_W(X, Y, z, ell, W64)
    z32, ell32 = z.astype(np.float32), ell.astype(np.float32)
    _, W32 = R.chol_factor(z32, ell32, np.float32(jit))
    s32 = R.stats_from_W(X, Y, z32, ell32, W32, dtype=np.float32, ksplit=args.ksplit)
    # (b): float32 running sums of the block products as well
    Phi_b = np.zeros((M, M), np.float32)
    b_b = np.zeros((1, M), np.float32)
    X32, Y32 = X.astype(np.float32), Y.astype(np.float32)
    for j0 in range(0, N, args.ksplit):
        A = R.A_of(W32, z32, X32[j0:j0 + args.ksplit], ell32)
        Phi_b += A @ A.T
        b_b += (A @ Y32[j0:j0 + args.ksplit]).T
    s32b = (Phi_b.astype(np.float64), b_b.astype(np.float64), s64[2], float(np.trace(Phi_b.astype(np.float64))))
    # arithmetic error alone: the float32 form against float64 on the SAME float32 W
    sW = R.stats_from_W(X32, Y32, z32, ell32, W32)
    lines.append("arithmetic error of the float32 form (same float32 inputs and W, float64 products as reference):")
    lines.append("  max|dPhi| / max|Phi| = %.3e   max|db| / max|b| = %.3e   |da2sum| / a2sum = %.3e"
                 % (np.abs(s32[0] - sW[0]).max() / np.abs(sW[0]).max(), np.abs(s32[1] - sW[1]).max() / np.abs(sW[1]).max(),
                    abs(s32[3] - sW[3]) / sW[3]))
    for nv in (0.09, 1.0):
        lines.append("noise_var = %g, k_var = 1:" % nv)
        m64, S64, _, L64 = R.optimal_q(s64[0], s64[1], nv)
        mu64, v64 = R.predict(xs, z, ell, jit, m64, S64, W=W64)
        bd64 = R.collapsed_bound(*s64, N, nv)
        lines.append("  float64            : min eig(Lambda) = %.6f  max eig = %.4e  bound = %.6f"
                     % (np.linalg.eigvalsh(L64).min(), np.linalg.eigvalsh(L64).max(), bd64))
        for name, st in (("float32 A, f64 sums", s32), ("float32 A, f32 sums", s32b)):
            m, S, _, Lam = R.optimal_q(st[0], st[1], nv)
            ev = np.linalg.eigvalsh(Lam)
            mu, v = R.predict(xs, z32.astype(np.float64), ell, jit, m, S, W=W32.astype(np.float64))
            bd = R.collapsed_bound(st[0], st[1], st[2], st[3], N, nv)
            lines.append("  %s: min eig(Lambda) = %.6f  max|d mean| = %.3e  max|d var| / var = %.3e  |d bound| / |bound| = %.3e"
                         % (name, ev.min(), np.abs(mu - mu64).max(), (np.abs(v - v64) / v64).max(), abs(bd - bd64) / abs(bd64)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
