"""Time the input gradients of the closed-form predictive and the closed-form acquisition (hb_sgp_predict_grad, hb_sgp_acq)
in ONE process, beside hb_sgp_predict at the same shape.

    python tools/bench_sgp_acq.py [--reps 5] [--iters 3] [--quick] [--out profiles/sgp_acq.txt]

Shape: n = 10^6 candidates, M = 512, float32 (the fused forms), d = 1, 2, 4; q(u) mean-field and full-rank.  Forms (device
events around `iters` calls; `reps` rounds, ALTERNATING between the forms so that each sees the same clocks and neighbours;
median and (min .. max) of the rounds):
  predict   hb_sgp_predict: mean and variance                    -- the baseline
  grad      hb_sgp_predict_grad: mean, var, dmean, dvar
  acq       hb_sgp_acq: EI values and gradient
  argmax    hb_sgp_acq: EI arg-max only (nothing of size n written; both launches)
By operation count the gradient adds about one half (mean-field) to one and a half (full-rank) M^2 n products to predict's
one to one and a half.  No target is set: the measured ratio to predict is reported."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="a hundredth of the points: checks the tool, measures nothing")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    n, M, dtype = (10000 if args.quick else 1000000), 512, torch.float32
    lines = ["device %s; n = %d, M = %d, float32; median of %d rounds of %d calls (min .. max), ms"
             % (H.device_info()[0], n, M, args.reps, args.iters)]
    rows = []
    for d in (1, 2, 4):
        rng = np.random.default_rng(d)
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()
        dom = 0.5 * M if d == 1 else 8.0
        x = up(rng.uniform(0, dom, (n, d)))
        z = up(np.linspace(0, dom, M)[:, None] if d == 1 else rng.uniform(0, dom, (M, d)))
        ell = up(np.ones(1))
        frag = torch.empty(2 * M * M, dtype=dtype, device="cuda")
        _, W, info = H.cholesky_inverse(H.gram_fwd(z, z, ell, diag_add=1e-3), frag=frag)
        assert int(info.cpu()[0]) == 0
        m = up(rng.standard_normal(M))
        for s_name, s, s_kind in (("mean-field", up(0.2 + 0.6 * rng.uniform(size=M)), H.SGP_S_DIAG),
                                  ("full-rank", up(np.tril(rng.standard_normal((M, M))) * (0.4 / np.sqrt(M)) + 0.3 * np.eye(M)),
                                   H.SGP_S_TRIL)):
            kw = dict(s_kind=s_kind, mode=H.SGP_DIAGONAL, jitter=1e-3, wfrag=frag)
            pout = (torch.empty((1, n), dtype=dtype, device="cuda"), torch.empty((1, n), dtype=dtype, device="cuda"))
            gout = tuple(torch.empty(sh, dtype=dtype, device="cuda") for sh in ((n,), (n,), (n, d), (n, d)))
            akw = dict(best=0.5, param=0.01, scale=1.0, var_floor=1e-6)
            res = {}

            def f_acq():
                res["acq"] = H.sgp_acq(x, z, ell, W, m, s, "ei", grad=True, **akw, **kw)

            def f_argmax():
                res["argmax"] = H.sgp_acq(x, z, ell, W, m, s, "ei", value=False, argmax=True, **akw, **kw)

            forms = dict(predict=lambda: H.sgp_predict(x, z, ell, W, m.reshape(1, -1), s, out=pout, **kw),
                         grad=lambda: H.sgp_predict_grad(x, z, ell, W, m, s, out=gout, **kw), acq=f_acq, argmax=f_argmax)
            for fn in forms.values():          # warm-up: every timed shape, code objects loaded
                fn()
                fn()
            torch.cuda.synchronize()
            val = res["acq"][0]
            same = bool(torch.equal(pout[0].reshape(-1), gout[0]) and torch.equal(pout[1].reshape(-1), gout[1])
                        and int(res["argmax"][3][0]) == int(torch.argmax(val)) and bool(res["argmax"][2][0] == val.max()))
            times = {k: [] for k in forms}
            for _ in range(args.reps):
                for k, fn in forms.items():
                    times[k].append(timed(fn, args.iters))
            st = {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in times.items()}
            base = st["predict"][0]
            rows.append(dict(n=n, M=M, d=d, q=s_name, same_result=same, **{k: [round(t, 4) for t in v] for k, v in st.items()}))
            lines.append("d=%d %-10s: predict %7.3f (%.3f .. %.3f) | grad %7.3f (%.3f .. %.3f) = x %.2f | acq value + gradient "
                         "%7.3f (%.3f .. %.3f) = x %.2f | arg-max only %7.3f (%.3f .. %.3f) = x %.2f of predict%s"
                         % ((d, s_name) + st["predict"] + st["grad"] + (st["grad"][0] / base,) + st["acq"] + (st["acq"][0] / base,)
                            + st["argmax"] + (st["argmax"][0] / base, "" if same else "  RESULTS DIFFER")))
            print(lines[-1], flush=True)
            del pout, gout
    print(json.dumps(dict(rows=rows)), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
