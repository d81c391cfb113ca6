"""Time hb_sgp_select_f32 (greedy conditional-variance selection of inducing points) in ONE process.

    python tools/bench_sgp_select.py [--N 100000 1000000] [--M 256 512 1024] [--reps 3] [--out profiles/sgp_select_bench.json]

Per (N, M), fp32, d = 1, X ~ U(0, M) (one lengthscale of domain per point asked for: no early stop), threshold 0, after a
warm-up run of every timed form:
    select  hb_sgp_select_f32: device events around the whole sequence of M + 1 launches, `reps` runs, the median and the
            min / max.  Model traffic: row j reads j rows of the history, N M^2 / 2 elements of 4 bytes; the achieved rate
            is that over the time.
    copy    the yardstick of the same run: a device-to-device copy of 1 GiB (read + write = 2 GiB moved), events around
            10 of them, between the select runs.
    torch   the same algorithm composed from torch device ops, one launch sequence and ONE READ-BACK (the pivot index)
            per point: what a user could do without the kernel.  Timed once per case (host clock around a synchronise:
            the read-backs are part of it); skipped above --torch-max-elems history elements.
One JSON line per case; --out collects them in a file.  The working set M N 4 bytes against the 256 MiB last-level cache
is recorded per row: the small cases fit, the large ones do not."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from henbun_amd import hip_ops as H  # noqa: E402


def events(fn, iters=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def torch_greedy(X, M):
    """The semantics of hb_sgp_select composed from torch ops (ell = 1, threshold 0); returns idx as a list."""
    N = X.shape[0]
    C = torch.zeros((M, N), dtype=X.dtype, device=X.device)
    dvar = torch.ones(N, dtype=X.dtype, device=X.device)
    idx = []
    for j in range(M):
        i = int(torch.argmax(dvar))                      # the read-back
        p = dvar[i]
        k = torch.exp(-0.5 * ((X - X[i]) ** 2).sum(1))
        c = (k - C[:j, i] @ C[:j]) / torch.sqrt(p)
        C[j] = c
        dvar = torch.clamp(dvar - c * c, min=0)
        dvar[i] = 0
        idx.append(i)
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--M", type=int, nargs="+", default=[256, 512, 1024])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-max-elems", type=float, default=1.1e9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    copy = lambda: dst.copy_(src)
    copy()
    results = []
    for N in args.N:
        for M in args.M:
            rng = np.random.RandomState(0)
            X = torch.as_tensor(rng.uniform(0, 1.0 * M, (N, 1)).astype(np.float32)).cuda()
            ell = torch.ones(1, dtype=torch.float32, device="cuda")
            ws = torch.empty(H.sgp_select_ws_elems(torch.float32, N, M, 1), dtype=torch.float32, device="cuda")
            out = [None]

            def select():
                out[0] = H.sgp_select(X, ell, M, 0.0, ws=ws)

            select()                                         # warm-up
            torch.cuda.synchronize()
            sel, cp = [], []
            for _ in range(args.reps):
                sel.append(events(select))
                cp.append(events(copy, 10))
            count = int(out[0][2].cpu()[0])
            ms, cms = float(np.median(sel)), float(np.median(cp))
            traffic = 0.5 * N * M * M * 4
            row = dict(N=N, M=M, dtype="float32", d=1, count=count, reps=args.reps,
                       select_ms=round(ms, 3), select_ms_min_max=[round(min(sel), 3), round(max(sel), 3)],
                       us_per_point=round(ms * 1e3 / M, 2),
                       model_traffic_GB=round(traffic / 1e9, 2), achieved_GBps=round(traffic / (ms * 1e-3) / 1e9, 1),
                       copy_GBps=round(2.0 * src.numel() * 4 / (cms * 1e-3) / 1e9, 1),
                       history_MiB=round(M * N * 4 / 2 ** 20, 1), last_level_cache_MiB=256,
                       trace=float(out[0][3].cpu()[0]))
            row["achieved_over_copy"] = round(row["achieved_GBps"] / row["copy_GBps"], 3)
            if float(M) * N <= args.torch_max_elems:
                torch_greedy(X, min(M, 16))                  # warm-up of every op
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tidx = torch_greedy(X, M)
                torch.cuda.synchronize()
                row["torch_composed_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
                row["torch_over_select"] = round(row["torch_composed_ms"] / ms, 2)
                same = int(np.sum(np.asarray(tidx) == out[0][0].cpu().numpy()))
                row["torch_same_choices"] = same             # for the record: nearly tied variances may part the two
            print(json.dumps(row), flush=True)
            results.append(row)
            del ws, X
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(device=H.device_info()[0], results=results), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
