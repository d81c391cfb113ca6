"""Time and measure the gradient of the collapsed bound (SparseGP.collapsed_bound_and_grad, hb_sgp_kgrad) in ONE process.

    python tools/bench_sgp_cbgrad.py [--reps 5] [--out profiles/sgp_cbgrad.txt] [--no-precision]

Timing, at N = 1e6, M = 512, d = 1 and at one d = 3 shape (float32 storage of X, Y; float64 arithmetic):
    stats     the float64 statistics Phi, b, yy: per chunk hb_sgp_A_f64 + three hb_matmul_f64
    streamed  hb_sgp_kgrad_f32 (repack of Q, the column-strip MFMA kernel, the fold)
    plain     the same entry in its plain-loop form (diagnostic switch; only at --plain-N columns, it is slow)
    tail      everything else of collapsed_bound_and_grad: factorisations, the M^3 products, the Gram VJP, read-backs
    matmul    the yardstick: hb_matmul_f64 on an equal M x M x N product, [M, M] x [M, 32768] per call -- the guides give
              no float64 MFMA peak, so the achieved FLOP/s of `streamed` (2 M^2 N) is set against this, measured in the
              same run
Device events around each form, `reps` runs alternating, the median.

Precision (the table of DESIGN.md 3, "Gradient of the collapsed bound"): svgp_data inputs, ell = 1, var = 0.09; float64
torch.autograd on the CPU as truth; relative error = max|dz| / max|z gradient| of
    (a) the streamed part taken in float32 (torch float32 on the device, Q K and the epilogue, chunked), the rest float64
    (b) the float64 tail and gradient passes fed the float32-formed Phi, b of statistics() in a float32 session
    (c) collapsed_bound_and_grad as shipped (float64 end to end) in a float32 session."""
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
from henbun_amd.models import SVGP, svgp_data  # noqa: E402

CHUNK = 32768


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def model(N, M, d, dtype, jitter=None):
    if d == 1:
        X, Y, Z = svgp_data(N, M, 0)
        ell = np.ones(1)
    else:
        rng = np.random.RandomState(0)
        X = rng.uniform(0, 4.0, (N, d))
        Y = np.sin(X.sum(1, keepdims=True)) + 0.3 * rng.randn(N, 1)
        Z = rng.uniform(0, 4.0, (M, d))
        ell = np.ones(1) * 1.1          # SVGP's kernel has one shared lengthscale
    m = SVGP(X=X, Y=Y, Z=Z, q_shape="diagonal", dtype=dtype)
    m.gp.kern.lengthscales = ell
    m.k_var = np.ones(1)
    m.var = np.ones(1) * 0.09
    m.initialize()
    return m, X, Y, Z, ell


def timing(N, M, d, reps, plain_N, lines):
    m, X, Y, Z, ell = model(N, M, d, "float32")
    g = object.__getattribute__
    gp, sess = g(m, "gp"), m._session
    Xd, Yd = sess.data_buffer(g(m, "X")), sess.data_buffer(g(m, "Y"))
    up = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.float32).astype(np.float64))).cuda()
    z, elld = up(Z), up(ell)
    L, _ = H.cholesky(H.gram_fwd(z, z, elld, diag_add=1e-5))
    W = H.trinv(L)
    rng = np.random.RandomState(1)
    Q = up(rng.randn(M, M))
    Q = (Q + Q.t()).contiguous()
    R = up(rng.randn(M, 1))
    ws = torch.empty(H.sgp_kgrad_ws_elems(N, M, d, 1), dtype=torch.float64, device="cuda")
    B = torch.randn(M, CHUNK, dtype=torch.float64, device="cuda")
    C = torch.empty(M, CHUNK, dtype=torch.float64, device="cuda")
    stats = [None]

    def f_stats():
        stats[0] = gp._statistics_f64(sess, Xd, Yd, z, elld, W)

    def f_streamed():
        H.sgp_kgrad(Xd, Yd, z, elld, Q, R, ws=ws)

    def f_matmul():
        for _ in range((N + CHUNK - 1) // CHUNK):
            H.matmul(Q, B, out=C)

    def f_tail():
        gp.collapsed_bound_and_grad(Xd[:64].contiguous(), Yd[:64].contiguous(), 0.09, 1.0)   # 64 rows: the data passes vanish

    def f_whole():
        gp.collapsed_bound_and_grad(g(m, "X"), g(m, "Y"), 0.09, 1.0)

    forms = dict(stats=f_stats, streamed=f_streamed, matmul=f_matmul, tail=f_tail, whole=f_whole)
    for fn in forms.values():
        fn()
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            times[k].append(timed(fn))
    med = {k: float(np.median(v)) for k, v in times.items()}
    flop = 2.0 * M * M * N
    lines.append("N=%d M=%d d=%d (float32 storage, float64 arithmetic), median of %d:" % (N, M, d, reps))
    for k in forms:
        lines.append("   %-9s %10.2f ms  (min %.2f max %.2f)" % (k, med[k], min(times[k]), max(times[k])))
    lines.append("   streamed: %.2f TFLOP/s on 2 M^2 N = %.1f GFLOP; hb_matmul_f64 on the equal product: %.2f TFLOP/s (ratio %.2f)"
                 % (flop / med["streamed"] / 1e9, flop / 1e9, flop / med["matmul"] / 1e9, med["matmul"] / med["streamed"]))
    lines.append("   stats / whole = %.2f, streamed / whole = %.2f, tail / whole = %.2f"
                 % (med["stats"] / med["whole"], med["streamed"] / med["whole"], med["tail"] / med["whole"]))
    if plain_N:
        n = min(plain_N, N)
        Xs, Ys = Xd[:n].contiguous(), Yd[:n].contiguous()
        H.debug_set("sgp_kgrad_plain", 1)
        try:
            H.sgp_kgrad(Xs, Ys, z, elld, Q, R, ws=ws)
            tp = timed(lambda: H.sgp_kgrad(Xs, Ys, z, elld, Q, R, ws=ws))
        finally:
            H.debug_clear()
        tf_ = timed(lambda: H.sgp_kgrad(Xs, Ys, z, elld, Q, R, ws=ws))
        lines.append("   plain-loop form at N=%d: %.2f ms against %.2f ms for the strips" % (n, tp, tf_))
    print("\n".join(lines[-(8 + (1 if plain_N else 0)):]), flush=True)


def streamed_fp32(Xd, Yd, z, ell, Q, R):
    """The streamed part in float32 torch ops on the device (what a float32 kernel would compute), chunked."""
    f = torch.float32
    z, ell, Q, R = z.to(f), ell.to(f), Q.to(f), R.to(f)
    zbar = torch.zeros_like(z)
    ellbar = torch.zeros(z.shape[1], dtype=f, device=z.device)
    for c0 in range(0, Xd.shape[0], CHUNK):
        Xc, Yc = Xd[c0:c0 + CHUNK].to(f), Yd[c0:c0 + CHUNK].to(f)
        diff = z[:, None, :] - Xc[None, :, :]                          # [M, n, d]
        K = torch.exp(-0.5 * ((diff / ell) ** 2).sum(-1))
        E = (Q @ K + R @ Yc.t()) * K
        zbar -= (E[:, :, None] * diff).sum(1) / ell ** 2
        ellbar += (E[:, :, None] * diff * diff).sum((0, 1)) / ell ** 3
    return zbar.double(), ellbar.double()


def precision(lines):
    import collapsed_grad_ref as C

    lines.append("")
    lines.append("precision of the z gradient on the device, float32 session, svgp_data, ell = 1, var = 0.09 (truth: float64 autograd, CPU)")
    lines.append("   N, M, jitter | max|z-gradient| | max|streamed part| | (a) streamed part in fp32 | (b) fp64 pass, Phi, b of the fp32 "
                 "statistics() | (c) everything fp64 (shipped)")
    for N, M, jit in [(20000, 64, 1e-6), (20000, 64, 1e-4), (100000, 128, 1e-5)]:
        cfg = hb.settings.get_settings()
        cfg.numerics.jitter_level = jit
        with hb.settings.temp_settings(cfg):
            m, X, Y, Z, ell = model(N, M, 1, "float32")
            g = object.__getattribute__
            gp, sess = g(m, "gp"), m._session
            X32, Y32, Z32 = (np.asarray(a, np.float32).astype(np.float64) for a in (X, Y, Z))
            a = C.bound_autograd(X32, Y32, Z32, ell, jit, 0.09, 1.0)
            r = C.bound_and_grad(X32, Y32, Z32, ell, jit, 0.09, 1.0)
            zmax = np.abs(a["z"]).max()
            _, gc = gp.collapsed_bound_and_grad(g(m, "X"), g(m, "Y"), 0.09, 1.0)
            try:
                st = gp.statistics(g(m, "X"), g(m, "Y"))
                inp = gp._grad_inputs(g(m, "X"), g(m, "Y"))
                ss, Xd_, Yd_, z_, l_, W_ = inp
                _, gb = gp._grad_from_statistics(ss, z_, l_, W_, (st[0], st[1], st[2]), 0.09, 1.0, "diagonal",
                                                 lambda Q, R: ss.H.sgp_kgrad(Xd_, Yd_, z_, l_, Q, R), Xd_.shape[0], Yd_.shape[1])
                eb = "%.2g" % (np.abs(gb["z"] - a["z"]).max() / zmax)
            except hb.graph.CholeskyError as e:
                eb = "fp32 factorisation failed"
            dev = lambda v: torch.as_tensor(np.ascontiguousarray(v)).cuda()
            zs32, _ = streamed_fp32(sess.data_buffer(g(m, "X")), sess.data_buffer(g(m, "Y")), dev(Z32), dev(ell), dev(r["Q"]),
                                    dev(r["R"]))
            ea = np.abs(zs32.cpu().numpy() + r["z_kmm"] - a["z"]).max() / zmax
            ec = np.abs(gc["z"] - a["z"]).max() / zmax
        lines.append("   %d, %d, %g | %.2g | %.3g | %.2g | %s | %.2g"
                     % (N, M, jit, zmax, np.abs(r["z_streamed"]).max(), ea, eb, ec))
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--plain-N", type=int, default=65536)
    ap.add_argument("--no-precision", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    lines = ["gradient of the collapsed bound (tools/bench_sgp_cbgrad.py) on %s" % (H.device_info()[0],)]
    timing(1000000, 512, 1, args.reps, args.plain_N, lines)
    timing(1000000, 256, 3, args.reps, 0, lines)
    if not args.no_precision:
        precision(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
