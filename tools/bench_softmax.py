"""Time the pieces of one natural-gradient step of multi-class classification (SparseGP.natgrad_q with likelihoods.Softmax)
in ONE process and write profiles/softmax_fit.txt.

    python tools/bench_softmax.py [--N 1000000] [--M 512] [--classes 3 10] [--nodes 128] [--reps 7] [--iters 3]
                                  [--window-ms 300] [--out profiles/softmax_fit.txt]

fp32, d = 2, blobs on a ring.  Per class count C (device events around a window of calls -- as many as fill `window-ms`, at least
`iters` -- sized per form from one probe; `reps` rounds, ALTERNATING between the forms; median and range of the per-call time):
    sites       hb_lik_softmax_sites_f32                 (lam, beta [C, N], sum l)
    predict     hb_lik_softmax_predict_f32 with labels   (prob [C, N], logdens [N], their sum)
    mwstats     hb_sgp_mwstats_f32                       (C weight sets from ONE A)
    wstats_xC   C calls of hb_sgp_wstats_f32             (the baseline: what the step cost before hb_sgp_mwstats)
    marginals   C calls of hb_sgp_predict_f32, full-rank S
    step        marginals + sites + mwstats + the C float64 M^3 tails (two Cholesky factors, an inverse, three products each)
The outputs of mwstats and wstats_xC are compared bit for bit at this size before anything is timed.  The operation count
says mwstats / wstats_xC should tend to (1 + C / 2) / (1.5 C): forming A_c is about M^2 nc multiply-adds, the symmetric
update about half that; the file records that figure beside the measured one."""
import argparse
import json
import os
import sys

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


def bench(N, M, C, S, reps, iters, window_ms):
    rng = np.random.RandomState(C)
    ang = 2.0 * np.pi * np.arange(C) / C
    cent = 3.0 * np.stack([np.cos(ang), np.sin(ang)], 1)
    yh = rng.randint(0, C, N)
    Xh = cent[yh] + 0.5 * rng.randn(N, 2)
    Zh = Xh[rng.choice(N, M, replace=False)]
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")
    X, y, z, ell = f32(Xh), f32(yh), f32(Zh), f32(np.ones(1))
    nodes = torch.as_tensor(rng.randn(S, C)).cuda()
    frag = torch.empty(2 * M * M, dtype=torch.float32, device="cuda")
    _, W, info = H.cholesky_inverse(H.gram_fwd(z, z, ell, diag_add=1e-3), frag=frag)
    assert int(info.cpu()[0]) == 0
    ws = torch.empty(H.sgp_mwstats_ws_elems(torch.float32, N, M, 2, C), dtype=torch.float32, device="cuda")
    mean, var, lam, beta = (torch.empty((C, N), dtype=torch.float32, device="cuda") for _ in range(4))
    state = dict(m=torch.zeros((C, M), dtype=torch.float32, device="cuda"),
                 S=torch.eye(M, dtype=torch.float32, device="cuda").repeat(C, 1, 1).contiguous(),
                 Lam=torch.eye(M, **f64).repeat(C, 1, 1).contiguous(), eta=torch.zeros((C, M), **f64))
    fused = H.sgp_predict_fused(torch.float32, 1, N, M, 2, 1, H.SGP_S_TRIL, True)

    def marginals():
        for c in range(C):
            H.sgp_predict(X, z, ell, W, state["m"][c:c + 1], state["S"][c], s_kind=H.SGP_S_TRIL,
                          out=(mean[c:c + 1], var[c:c + 1]), wfrag=frag if fused else None)

    def sites():
        return H.lik_softmax_sites(y, mean, var, nodes, mscale=2.0, vscale=4.0, out=(lam, beta))

    def predict():
        return H.lik_softmax_predict(mean, var, nodes, y=y, mscale=2.0, vscale=4.0)

    def mwstats():
        return H.sgp_mwstats(X, lam, beta, z, ell, W, wfrag=frag, ws=ws)

    def wstats_xC():
        return [H.sgp_wstats(X, lam[c], beta[c], z, ell, W, wfrag=frag, ws=ws) for c in range(C)]

    def step():
        for c in range(C):
            L, _ = H.cholesky(state["Lam"][c].contiguous())
            V = H.trinv(L)
            m = H.matmul(H.matmul(state["eta"][c:c + 1].contiguous(), V, transB=True), V)
            Sc, _ = H.cholesky(H.matmul(V, V, transA=True))
            state["m"][c:c + 1], state["S"][c] = m.to(torch.float32), Sc.to(torch.float32)
        marginals()
        sites()
        mwstats()

    marginals()
    _, _, lsum = sites()
    Phi, b, tr = mwstats()                 # one real step from the prior: the timed forms see the weights of a fit
    ref = wstats_xC()
    torch.cuda.synchronize()
    same = all(torch.equal(Phi[c], ref[c][0]) and torch.equal(b[c], ref[c][1][0]) and torch.equal(tr[c], ref[c][2][0])
               for c in range(C))
    assert same, "hb_sgp_mwstats does not return the bits of hb_sgp_wstats at N=%d M=%d C=%d" % (N, M, C)
    eye = torch.eye(M, **f64)
    state["Lam"], state["eta"] = (0.5 * eye + 0.5 * (4.0 * Phi + eye)).contiguous(), (0.5 * 2.0 * b).contiguous()
    forms = dict(sites=sites, predict=predict, mwstats=mwstats, wstats_xC=wstats_xC, marginals=marginals, step=step)
    for fn in forms.values():              # warm-up: every timed shape, code objects loaded
        fn()
        fn()
    torch.cuda.synchronize()
    # every timed window lasts at least `window_ms`: a form's call count is sized from one probe of it
    calls = {k: max(iters, int(np.ceil(window_ms / max(timed(fn, 2), 1e-3)))) for k, fn in forms.items()}
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():        # alternating: every form sees the same clocks and the same neighbours
            times[k].append(timed(fn, calls[k]))
    row = dict(N=N, M=M, d=2, C=C, nodes=S, calls_per_window=calls, reps=reps, fused_marginals=bool(fused),
               bits_equal=bool(same), lsum=float(lsum.cpu()[0]))
    for k, v in times.items():
        row[k + "_ms"] = round(float(np.median(v)), 3)
        row[k + "_ms_min_max"] = [round(float(np.min(v)), 3), round(float(np.max(v)), 3)]
    row["mwstats_over_wstats_xC"] = round(row["mwstats_ms"] / row["wstats_xC_ms"], 4)
    row["mwstats_over_wstats_xC_per_round"] = [round(a / b, 4) for a, b in zip(times["mwstats"], times["wstats_xC"])]
    row["operation_count_ratio"] = round((1.0 + 0.5 * C) / (1.5 * C), 4)
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
    ap.add_argument("--out", default=os.path.join("profiles", "softmax_fit.txt"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    rows = [bench(args.N, args.M, C, args.nodes, args.reps, args.iters, args.window_ms) for C in args.classes]
    lines = ["Multi-class natural-gradient step (tools/bench_softmax.py) on %s" % H.device_info()[0],
             "fp32, N = %d, M = %d, d = 2, %d nodes; device events around windows of >= %.0f ms, %d alternating rounds, median [min, max] ms per call"
             % (args.N, args.M, args.nodes, args.window_ms, args.reps), ""]
    for r in rows:
        lines.append("C = %d   (fused marginals: %s; mwstats bits == wstats bits: %s; calls per window: %s)"
                     % (r["C"], r["fused_marginals"], r["bits_equal"], r["calls_per_window"]))
        for k in ("sites", "predict", "mwstats", "wstats_xC", "marginals", "step"):
            lines.append("  %-10s %9.3f  [%.3f, %.3f]" % ((k, r[k + "_ms"]) + tuple(r[k + "_ms_min_max"])))
        lines.append("  mwstats / wstats_xC = %.4f measured (per round %s); (1 + C/2) / (1.5 C) = %.4f by operation count"
                     % (r["mwstats_over_wstats_xC"], r["mwstats_over_wstats_xC_per_round"], r["operation_count_ratio"]))
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
