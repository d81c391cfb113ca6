"""Time the hyper-parameter gradient of the ELBO at a fixed q(u) (SparseGP.elbo_and_grad, hb_sgp_wkgrad) in ONE process.

    python tools/bench_sgp_elbo_grad.py [--reps 5] [--out profiles/sgp_elbo_grad.txt]

At N = 1e6, M = 512, d = 1 (float32 storage of X, Y; float64 arithmetic), Bernoulli likelihood:
    kgrad     hb_sgp_kgrad_f32 at P = 1 (repack of Q, the column-strip MFMA kernel, the fold); a timed window holds
              --calls (8) calls back to back and the figure is the window over the calls
    wkgrad    hb_sgp_wkgrad_f32 on the same X, Q, R with drawn weights: the same kernel plus two staged values per column
              and one multiply per accumulator.  The expectation recorded here (not asserted): about the cost of kgrad.
    marginals, sites, wstats   the three float64 chunked passes of elbo_and_grad over all of X (hb_sgp_predict_f64,
              hb_lik_sites_f64, hb_sgp_wstats_f64), each timed on its own over the same chunks
    whole     one SparseGP.elbo_and_grad, read-backs included
Device events around each form, `reps` runs alternating between the forms, the median (min, max).  The FLOP/s quoted
for wkgrad is a whole-call rate (repack + strip kernel + fold over 2 M^2 N), not a kernel rate."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import henbun_amd as hb  # noqa: E402
from henbun_amd import hip_ops as H  # noqa: E402
from henbun_amd.models import SVGPLik  # noqa: E402

CHUNK = 32768


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def timing(N, M, reps, calls, lines):
    import sites_ref as SR

    X, y, Z = SR.problem(SR.BERNOULLI, N=N, M=M)
    lik = hb.likelihoods.Bernoulli()
    m = SVGPLik(X=X, Y=y, Z=Z, likelihood=lik, dtype="float32")
    m.gp.kern.lengthscales = SR.ELL.copy()
    m.k_var = np.ones(1) * SR.K_VAR
    m.initialize()
    g = object.__getattribute__
    gp, sess = g(m, "gp"), m._session
    Xd, Yd = sess.data_buffer(g(m, "X")), sess.data_buffer(g(m, "Y"))
    _, _, _, z, ell, W = gp._grad_inputs(g(m, "X"), g(m, "Y"), "bench")
    up = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    rng = np.random.RandomState(1)
    Q = up(rng.randn(M, M))
    Q = (Q + Q.t()).contiguous()
    R = up(rng.randn(M, 1))
    w = rng.randn(N)
    w[rng.uniform(size=N) < 0.1] = 0.0
    w, r = up(w), up(rng.randn(N))
    ws = torch.empty(H.sgp_kgrad_ws_elems(N, M, 1, 1), dtype=torch.float64, device="cuda")
    qm, qS = up(0.1 * rng.randn(1, M)), up(np.tril(0.01 * rng.randn(M, M), -1) + 0.5 * np.eye(M))
    q = (qm.cpu().numpy(), qS.cpu().numpy())
    chunks = [(Xd[c:c + CHUNK].to(torch.float64).contiguous(), Yd[c:c + CHUNK, 0].to(torch.float64).contiguous())
              for c in range(0, N, CHUNK)]
    mv = [H.sgp_predict(Xc, z, ell, W, qm, qS, s_kind=H.SGP_S_TRIL, mode=H.SGP_DIAGONAL) for Xc, _ in chunks]
    mv = [(a.clone(), b.clone()) for a, b in mv]
    lb = [H.lik_sites(lik.lik_id, yc, a, b, mscale=np.sqrt(SR.K_VAR), vscale=SR.K_VAR)[:2] for (_, yc), (a, b) in zip(chunks, mv)]

    def f_kgrad():
        for _ in range(calls):
            H.sgp_kgrad(Xd, Yd, z, ell, Q, R, ws=ws)

    def f_wkgrad():
        for _ in range(calls):
            H.sgp_wkgrad(Xd, w, r, z, ell, Q, R, ws=ws)

    def f_marginals():
        for Xc, _ in chunks:
            H.sgp_predict(Xc, z, ell, W, qm, qS, s_kind=H.SGP_S_TRIL, mode=H.SGP_DIAGONAL)

    def f_sites():
        for (_, yc), (a, b) in zip(chunks, mv):
            H.lik_sites(lik.lik_id, yc, a, b, mscale=np.sqrt(SR.K_VAR), vscale=SR.K_VAR)

    def f_wstats():
        for (Xc, _), (lc, bc) in zip(chunks, lb):
            H.sgp_wstats(Xc, lc, bc, z, ell, W)

    def f_whole():
        gp.elbo_and_grad(g(m, "X"), g(m, "Y"), lik, q, k_var=SR.K_VAR)

    forms = dict(kgrad=f_kgrad, wkgrad=f_wkgrad, marginals=f_marginals, sites=f_sites, wstats=f_wstats, whole=f_whole)
    for fn in forms.values():
        fn()
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            times[k].append(timed(fn) / (calls if k in ("kgrad", "wkgrad") else 1))
    med = {k: float(np.median(v)) for k, v in times.items()}
    flop = 2.0 * M * M * N
    lines.append("N=%d M=%d d=1 (float32 storage, float64 arithmetic), median of %d (kgrad, wkgrad: per call, %d calls per "
                 "timed window):" % (N, M, reps, calls))
    for k in forms:
        lines.append("   %-9s %10.2f ms  (min %.2f max %.2f)" % (k, med[k], min(times[k]), max(times[k])))
    lines.append("   wkgrad / kgrad = %.3f (expected about 1: two more staged values per column, one multiply per accumulator); "
                 "wkgrad, whole call (repack + strips + fold): %.2f TFLOP/s on 2 M^2 N = %.1f GFLOP" % (med["wkgrad"] / med["kgrad"], flop / med["wkgrad"] / 1e9, flop / 1e9))
    lines.append("   of the whole: marginals %.2f, sites %.2f, wstats %.2f, wkgrad %.2f"
                 % tuple(med[k] / med["whole"] for k in ("marginals", "sites", "wstats", "wkgrad")))
    print("\n".join(lines[-9:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--N", type=int, default=1000000)
    ap.add_argument("--M", type=int, default=512)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lines = ["hyper-parameter gradient of the ELBO at a fixed q(u) (tools/bench_sgp_elbo_grad.py) on %s" % (H.device_info()[0],)]
    timing(args.N, args.M, args.reps, args.calls, lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
