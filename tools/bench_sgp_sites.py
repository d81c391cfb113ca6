"""Time the pieces of one natural-gradient step on q(u) (SparseGP.natgrad_q) in ONE process.

    python tools/bench_sgp_sites.py [--N 1000000] [--M 512] [--reps 7] [--iters 5] [--out profiles/sgp_sites_bench.json]

Forms, fp32 (device events around `iters` calls; `reps` rounds, ALTERNATING between the forms; the median is reported):
    stats      hb_sgp_stats_f32                      (the unweighted pass: the yardstick of the weighted one)
    wstats     hb_sgp_wstats_f32                     (Phi = A diag(lam) A^T, b = A beta)
    marginals  hb_sgp_predict_f32, full-rank S       (mean, var of f at every row of X)
    sites      hb_lik_sites_f32, Bernoulli           (lam, beta, sum l)
    sites_*    hb_lik_sites_f32 for Laplace(0.3), Gamma(4), NegativeBinomial(2), Binomial(12) on labels drawn from each at the
               same latent function; param_grad_negbinomial / logdens_negbinomial: hb_lik_param_grad_f32 / hb_lik_logdens_f32
    iteration  marginals + sites + wstats + the float64 M^3 tail (two Cholesky factors, an inverse, three products)
and, once, a Bernoulli fit to tol = 1e-8 from the prior through models.SVGPLik.fit_q (host clock around a synchronise)."""
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
from henbun_amd.models import SVGPLik  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, M = args.N, args.M
    torch.cuda.set_device(0)
    rng = np.random.RandomState(0)
    Xh = rng.uniform(0, 0.5 * M, (N, 1))
    yh = (rng.uniform(size=(N, 1)) < 1.0 / (1.0 + np.exp(-1.5 * np.sin(Xh)))).astype(np.float64)
    Zh = np.linspace(0, 0.5 * M, M)[:, None]
    f32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    X, Y, z, ell = f32(Xh), f32(yh), f32(Zh), f32(np.ones(1))
    frag = torch.empty(2 * M * M, dtype=torch.float32, device="cuda")
    _, W, info = H.cholesky_inverse(H.gram_fwd(z, z, ell, diag_add=1e-5), frag=frag)
    assert int(info.cpu()[0]) == 0
    ws = torch.empty(H.sgp_stats_ws_elems(torch.float32, N, M, 1, 1), dtype=torch.float32, device="cuda")
    mean, var, lam, beta = (torch.empty((1, N), dtype=torch.float32, device="cuda") for _ in range(4))
    Lam = torch.eye(M, dtype=torch.float64, device="cuda")
    eta = torch.zeros((1, M), dtype=torch.float64, device="cuda")
    state = dict(m=torch.zeros((1, M), dtype=torch.float32, device="cuda"), S=torch.eye(M, dtype=torch.float32, device="cuda"))
    fused = H.sgp_predict_fused(torch.float32, 1, N, M, 1, 1, H.SGP_S_TRIL, True)

    def stats():
        H.sgp_stats(X, Y, z, ell, W, wfrag=frag, ws=ws)

    def marginals():
        H.sgp_predict(X, z, ell, W, state["m"], state["S"], s_kind=H.SGP_S_TRIL, out=(mean, var), wfrag=frag if fused else None)

    def sites():
        H.lik_sites(H.LIK_BERNOULLI, Y, mean, var, out=(lam, beta))

    def wstats():
        return H.sgp_wstats(X, lam, beta, z, ell, W, wfrag=frag, ws=ws)

    latent = 1.5 * np.sin(Xh)
    zoo = dict(laplace=(H.LIK_LAPLACE, 0.3, latent + rng.laplace(0.0, 0.3, latent.shape)),
               gamma=(H.LIK_GAMMA, 4.0, rng.gamma(4.0, np.exp(latent) / 4.0)),
               negbinomial=(H.LIK_NEGBINOMIAL, 2.0, rng.negative_binomial(2.0, 2.0 / (2.0 + np.exp(latent)))),
               binomial=(H.LIK_BINOMIAL, 12.0, rng.binomial(12, 1.0 / (1.0 + np.exp(-latent)))))
    zoo = {k: (lik, p, f32(yk)) for k, (lik, p, yk) in zoo.items()}

    def zoo_sites(name):
        lik, p, yk = zoo[name]
        return lambda: H.lik_sites(lik, yk, mean, var, param=p, out=(lam, beta))

    def param_grad():
        lik, p, yk = zoo["negbinomial"]
        return H.lik_param_grad(lik, yk.reshape(-1), mean.reshape(-1), var.reshape(-1), param=p)

    def logdens():
        lik, p, yk = zoo["negbinomial"]
        return H.lik_logdens(lik, yk.reshape(-1), mean.reshape(-1), var.reshape(-1), param=p)

    def iteration():
        L, _ = H.cholesky(Lam)
        V = H.trinv(L)
        m = H.matmul(H.matmul(eta, V, transB=True), V)
        S, _ = H.cholesky(H.matmul(V, V, transA=True))
        state["m"], state["S"] = m.to(torch.float32), S.to(torch.float32)
        marginals()
        sites()
        wstats()

    forms = dict(stats=stats, wstats=wstats, marginals=marginals, sites=sites, iteration=iteration)
    forms.update({"sites_" + k: zoo_sites(k) for k in zoo})
    forms.update(param_grad_negbinomial=param_grad, logdens_negbinomial=logdens)
    marginals()
    sites()
    Phi, b, _ = wstats()                   # one real step from the prior: the timed forms see the weights of a fit
    Lam, eta = (Phi + torch.eye(M, dtype=torch.float64, device="cuda")).contiguous(), b.contiguous()
    for fn in forms.values():              # warm-up: every timed shape, code objects loaded
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(args.reps):
        for k, fn in forms.items():        # alternating: every form sees the same clocks and the same neighbours
            times[k].append(timed(fn, args.iters))
    row = dict(N=N, M=M, iters=args.iters, reps=args.reps, fused_marginals=bool(fused))
    for k, v in times.items():
        row[k + "_ms"] = round(float(np.median(v)), 4)
        row[k + "_ms_min_max"] = [round(float(np.min(v)), 4), round(float(np.max(v)), 4)]
    row["wstats_over_stats"] = round(row["wstats_ms"] / row["stats_ms"], 4)
    row["wstats_over_stats_per_round"] = [round(a / b, 4) for a, b in zip(times["wstats"], times["stats"])]
    print(json.dumps(row), flush=True)

    model = SVGPLik(X=Xh, Y=yh, Z=Zh, likelihood=hb.likelihoods.Bernoulli(), dtype="float32")
    model.initialize()
    model.fit_q(steps=1)                   # warm-up
    sess = model._session
    q = object.__getattribute__(model, "u")
    sess.write_raw(object.__getattribute__(q, "q_mu"), np.zeros(M))
    S0 = np.eye(M)
    sess.write_raw(object.__getattribute__(q, "q_sqrt"), hb.param.tri_pack(S0) if q.packed else S0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, _, info = model.fit_q(steps=50, tol=1e-8)
    torch.cuda.synchronize()
    fit = dict(likelihood="bernoulli", tol=1e-8, steps=int(info["steps"]), wall_ms=round(1e3 * (time.perf_counter() - t0), 2),
               elbo=[round(float(e), 3) for e in info["elbo"]], residual=[float("%.3e" % r) for r in info["residual"]])
    print(json.dumps(fit), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=H.device_info()[0], results=[row], fit=fit), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
