"""Time the pieces of the multi-class hyper-parameter gradient at fixed q (SparseGP.elbo_and_grad_multi) in ONE process and
write profiles/softmax_grad.txt.

    python tools/bench_softmax_grad.py [--N 1000000] [--M 512] [--classes 3 10] [--nodes 128] [--reps 7] [--iters 3]
                                       [--window-ms 300] [--parts kernels model] [--out profiles/softmax_grad.txt]

d = 2, blobs on a ring, X in float32.  Part `kernels`, per class count C (device events around a window of calls -- as many
as fill `window-ms`, at least `iters` -- sized per form from one probe; `reps` rounds, ALTERNATING between the forms;
median and range of the per-call time):
    sites        hb_lik_softmax_sites_f32                 (lam, beta [C, N] float32, sum l)
    grad         hb_lik_softmax_grad_f32                  (w, r [C, N] float64, sum l): the same node loop plus one fma
    wkgrad_xC    C calls of hb_sgp_wkgrad_f32 and the C - 1 additions of their outputs: the streamed part as
                 elbo_and_grad_multi runs it (reported; a one-pass kernel over all classes measured 1.6 x slower and is
                 not kept)
Before anything is timed lsum of grad is compared bit for bit with that of sites.
Part `model` (wall clock around synchronous calls, after one warm-up call; reported, not bounded): one
SVGPMulticlass.elbo_and_grad() and one outer step of fit_hyper (fit_q(steps=5) + elbo_and_grad()) in a float32 session."""
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


def ring(N, M, C):
    rng = np.random.RandomState(C)
    ang = 2.0 * np.pi * np.arange(C) / C
    cent = 3.0 * np.stack([np.cos(ang), np.sin(ang)], 1)
    y = rng.randint(0, C, N)
    X = cent[y] + 0.5 * rng.randn(N, 2)
    return rng, X, y, X[rng.choice(N, M, replace=False)]


def bench_kernels(N, M, C, S, reps, iters, window_ms):
    rng, Xh, yh, Zh = ring(N, M, C)
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    X, y = f32(Xh), f32(yh)
    z, ell = f64(Zh.astype(np.float32)), f64(np.ones(1))
    nodes = f64(rng.randn(S, C))
    mean, var = f32(2.0 * rng.randn(C, N)), f32(rng.uniform(0.02, 1.5, (C, N)))
    lam, beta = (torch.empty((C, N), dtype=torch.float32, device="cuda") for _ in range(2))
    w, r = (torch.empty((C, N), dtype=torch.float64, device="cuda") for _ in range(2))
    Q = f64(rng.randn(C, M, M) / M)
    Q = (Q + Q.transpose(1, 2)).contiguous()
    R = f64(rng.randn(M, C))
    wsk = torch.empty(H.sgp_kgrad_ws_elems(N, M, 2, 1), dtype=torch.float64, device="cuda")
    Qc, Rc = [Q[c].contiguous() for c in range(C)], [R[:, c:c + 1].contiguous() for c in range(C)]

    def sites():
        return H.lik_softmax_sites(y, mean, var, nodes, mscale=2.0, vscale=4.0, out=(lam, beta))

    def grad():
        return H.lik_softmax_grad(y, mean, var, nodes, mscale=2.0, vscale=4.0, out=(w, r))

    def wkgrad_xC():
        zb, eb = H.sgp_wkgrad(X, w[0], r[0], z, ell, Qc[0], Rc[0], ws=wsk)
        for c in range(1, C):
            zc, ec = H.sgp_wkgrad(X, w[c], r[c], z, ell, Qc[c], Rc[c], ws=wsk)
            zb, eb = zb + zc, eb + ec
        return zb, eb

    _, _, ls = sites()
    _, _, lg = grad()
    torch.cuda.synchronize()
    assert torch.equal(ls, lg), "hb_lik_softmax_grad's lsum does not have the bits of hb_lik_softmax_sites's"
    forms = dict(sites=sites, grad=grad, wkgrad_xC=wkgrad_xC)
    for fn in forms.values():              # warm-up: every timed shape, code objects loaded
        fn()
        fn()
    torch.cuda.synchronize()
    calls = {k: max(iters, int(np.ceil(window_ms / max(timed(fn, 2), 1e-3)))) for k, fn in forms.items()}
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():        # alternating: every form sees the same clocks and the same neighbours
            times[k].append(timed(fn, calls[k]))
    row = dict(part="kernels", N=N, M=M, d=2, C=C, nodes=S, calls_per_window=calls, reps=reps, lsum_bits_equal=True,
               negative_w=float((w < 0).double().mean().cpu()))
    for k, v in times.items():
        row[k + "_ms"] = round(float(np.median(v)), 3)
        row[k + "_ms_min_max"] = [round(float(np.min(v)), 3), round(float(np.max(v)), 3)]
    row["grad_over_sites"] = round(row["grad_ms"] / row["sites_ms"], 4)
    row["grad_over_sites_per_round"] = [round(p / q, 4) for p, q in zip(times["grad"], times["sites"])]
    return row


def bench_model(N, M, C, S, reps):
    from henbun_amd.models import SVGPMulticlass

    rng, Xh, yh, Zh = ring(N, M, C)
    m = SVGPMulticlass(X=Xh.astype(np.float32), y=yh, Z=Zh.astype(np.float32), num_classes=C, nodes=rng.randn(S, C),
                       dtype="float32")
    m.k_var = np.ones(1) * 4.0
    m.initialize()
    m.reset_q()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def outer():
        m.fit_q(steps=5, tol=0.0)
        m.elbo_and_grad()

    outer()                                # warm-up, and a q of five steps for the gradient
    te, to = [wall(m.elbo_and_grad) for _ in range(reps)], [wall(outer) for _ in range(reps)]
    row = dict(part="model", N=N, M=M, d=2, C=C, nodes=S, reps=reps, value=m.elbo_and_grad()[0])
    for k, v in (("elbo_and_grad", te), ("outer_step", to)):
        row[k + "_ms"] = round(float(np.median(v)), 1)
        row[k + "_ms_min_max"] = [round(float(np.min(v)), 1), round(float(np.max(v)), 1)]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=1000000)
    ap.add_argument("--M", type=int, default=512)
    ap.add_argument("--classes", type=int, nargs="+", default=[3, 10])
    ap.add_argument("--nodes", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--parts", nargs="+", default=["kernels", "model"], choices=["kernels", "model"])
    ap.add_argument("--out", default=os.path.join("profiles", "softmax_grad.txt"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lines = ["Multi-class hyper-parameter gradient at fixed q (tools/bench_softmax_grad.py) on %s" % H.device_info()[0],
             "N = %d, M = %d, d = 2, %d nodes, X in float32" % (args.N, args.M, args.nodes), ""]
    rows = []
    if "kernels" in args.parts:
        lines.append("kernels: device events around windows of >= %.0f ms, %d alternating rounds, median [min, max] ms per call"
                     % (args.window_ms, args.reps))
        for C in args.classes:
            r = bench_kernels(args.N, args.M, C, args.nodes, args.reps, args.iters, args.window_ms)
            rows.append(r)
            lines.append("C = %d   (lsum bits == sites bits: %s; %.1f %% of w negative; calls per window: %s)"
                         % (C, r["lsum_bits_equal"], 100 * r["negative_w"], r["calls_per_window"]))
            for k in ("sites", "grad", "wkgrad_xC"):
                lines.append("  %-10s %9.3f  [%.3f, %.3f]" % ((k, r[k + "_ms"]) + tuple(r[k + "_ms_min_max"])))
            lines.append("  grad / sites = %.4f (per round %s)" % (r["grad_over_sites"], r["grad_over_sites_per_round"]))
            lines.append("")
    if "model" in args.parts:
        lines.append("model (float32 session): wall clock around synchronous calls, %d calls after a warm-up, median [min, max] ms"
                     % min(args.reps, 3))
        for C in args.classes:
            r = bench_model(args.N, args.M, C, args.nodes, min(args.reps, 3))
            rows.append(r)
            lines.append("C = %d   value %.6f" % (C, r["value"]))
            lines.append("  SVGPMulticlass.elbo_and_grad()             %10.1f  [%.1f, %.1f]"
                         % ((r["elbo_and_grad_ms"],) + tuple(r["elbo_and_grad_ms_min_max"])))
            lines.append("  fit_q(steps=5) + elbo_and_grad() (one step) %9.1f  [%.1f, %.1f]"
                         % ((r["outer_step_ms"],) + tuple(r["outer_step_ms_min_max"])))
            lines.append("")
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines))
        print("\n".join(lines))


if __name__ == "__main__":
    main()
