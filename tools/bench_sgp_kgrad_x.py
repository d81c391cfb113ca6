"""Time the input gradient of the sparse-GP gradient pass (hb_sgp_kgrad_x / hb_sgp_wkgrad_x) against the entries without
it, and one step of models.DeepKernelSVGP, in ONE process.

    python tools/bench_sgp_kgrad_x.py [--reps 9] [--out profiles/sgp_kgrad_x.txt] [--other-lib PATH]

Kernel pairs at N = 1e6, M = 512, d = 1, 2, 4 (float32 storage of X, Y; float64 arithmetic), the whole entry each (repack
of Q, the column-strip MFMA kernel, the fold):
    kgrad    hb_sgp_kgrad_f32          kgrad_x   hb_sgp_kgrad_x_f32   (+ xbar [N, d])
    wkgrad   hb_sgp_wkgrad_f32         wkgrad_x  hb_sgp_wkgrad_x_f32
    other    hb_sgp_kgrad_f32 of ANOTHER build of the library (--other-lib: a libhenbun_hip.so, e.g. of the parent commit),
             called through ctypes on the same buffers in the same alternation -- is the entry without xbar unchanged?
Device events around each call, `reps` rounds alternating the forms, the median, minimum and maximum (the spread).

One DeepKernelSVGP.bound_and_grad() at N = 1e5, M = 128, net [8, 64, 64, 2] (float32 session), broken into
    forward     the plan that leaves H = net(X) on the device
    statistics  the float64 statistics Phi, b, yy of the features
    gradient    hb_sgp_kgrad_x_f32 on the features (zbar, ellbar, Hbar)
    backward    Hbar into the Data buffer and the plan that returns J^T Hbar for the network's variables
    whole       bound_and_grad() (also the M^3 tail, the Gram VJP of K(z, z) and the read-backs)."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from henbun_amd import hip_ops as H  # noqa: E402
from henbun_amd.models import DeepKernelSVGP, _part  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(forms, reps):
    for fn in forms.values():
        fn()
    times = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            times[k].append(timed(fn))
    return times


def report(lines, times, pairs):
    med = {k: float(np.median(v)) for k, v in times.items()}
    for k, v in times.items():
        lines.append("   %-9s %9.3f ms  (min %.3f max %.3f)" % (k, med[k], min(v), max(v)))
    for a, b in pairs:
        if a in med and b in med:
            lines.append("   %s / %s = %.3f" % (a, b, med[a] / med[b]))


def other_kgrad(path):
    """hb_sgp_kgrad_f32 of another build of the library, bound by hand (the signature of include/henbun_hip.h)."""
    lib = ctypes.CDLL(os.path.abspath(path))
    f = lib.hb_sgp_kgrad_f32
    p, l = ctypes.c_void_p, ctypes.c_long
    f.argtypes = [ctypes.c_int, p, p, p, p, l, p, p, p, p, l, l, l, l, p, p]
    f.restype = ctypes.c_int
    return f


def kernels(N, M, d, reps, other, lines):
    rng = np.random.RandomState(d)
    f32, f64 = dict(dtype=torch.float32, device="cuda"), dict(dtype=torch.float64, device="cuda")
    X = torch.as_tensor(rng.uniform(0, 0.5 * M if d == 1 else 4.0, (N, d)), **f32)
    Y = torch.as_tensor(rng.randn(N, 1), **f32)
    w, r = torch.as_tensor(rng.rand(N), **f64), torch.as_tensor(rng.randn(N), **f64)
    z = torch.as_tensor(np.linspace(0, 0.5 * M, M)[:, None] if d == 1 else rng.uniform(0, 4.0, (M, d)), **f64)
    ell = torch.ones(1 if d == 1 else d, **f64)
    Q = torch.as_tensor(rng.randn(M, M), **f64)
    Q = (Q + Q.t()).contiguous()
    R = torch.as_tensor(rng.randn(M, 1), **f64)
    ws = torch.empty(H.sgp_kgrad_ws_elems(N, M, d, 1), **f64)
    forms = dict(kgrad=lambda: H.sgp_kgrad(X, Y, z, ell, Q, R, ws=ws),
                 kgrad_x=lambda: H.sgp_kgrad(X, Y, z, ell, Q, R, ws=ws, x_grad=True),
                 wkgrad=lambda: H.sgp_wkgrad(X, w, r, z, ell, Q, R, ws=ws),
                 wkgrad_x=lambda: H.sgp_wkgrad(X, w, r, z, ell, Q, R, ws=ws, x_grad=True))
    if other is not None:
        zb, eb = torch.empty(M, d, **f64), torch.empty(ell.numel(), **f64)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr())

        def f_other():
            rc = other(H.KERN_RBF, ptr(X), ptr(Y), ptr(z), ptr(ell), ell.numel(), ptr(Q), ptr(R), ptr(zb), ptr(eb), N, M, d, 1,
                       ptr(ws), ctypes.c_void_p(H.stream()))
            assert rc == 0

        forms["other"] = f_other
    times = alternate(forms, reps)
    if other is not None:       # the same entry of the two builds returns the same bits
        z0, e0 = H.sgp_kgrad(X, Y, z, ell, Q, R, ws=ws)
        forms["other"]()
        torch.cuda.synchronize()
        assert torch.equal(z0, zb) and torch.equal(e0, eb)
    lines.append("N=%d M=%d d=%d (float32 storage, float64 arithmetic), median of %d alternating rounds:" % (N, M, d, reps))
    report(lines, times, [("kgrad_x", "kgrad"), ("wkgrad_x", "wkgrad"), ("kgrad", "other")])
    if other is not None:
        lines.append("   zbar, ellbar of kgrad and other: the same bits")


def deep_kernel(N, M, reps, lines):
    rng = np.random.RandomState(0)
    np.random.seed(0)
    X = rng.uniform(-2, 2, (N, 8))
    Y = np.sin(X[:, :1] + X[:, 1:2]) * np.cos(X[:, 2:3]) + 0.1 * rng.randn(N, 1)
    m = DeepKernelSVGP(X=X, Y=Y, M=M, hidden=[64, 64], feature_dim=2, activation="tanh", dtype="float32")
    m.gp.kern.lengthscales = np.ones(2) * 0.3
    m.var = np.ones(1) * 0.1
    m.initialize()
    m.bound_and_grad()
    gp, sess = _part(m, "gp"), m._session
    fwd, fouts = m._plan("forward")
    bwd, _ = m._plan("backward")
    Hd = m._features().clone()
    _, Xd, Yd, z, ell, W = gp._grad_inputs(Hd, _part(m, "Y"))
    Q = torch.randn(M, M, dtype=torch.float64, device="cuda")
    Q = (Q + Q.t()).contiguous()
    R = torch.randn(M, 1, dtype=torch.float64, device="cuda")
    out = [None]

    def f_forward():
        fwd.run()
        fwd.check()

    def f_gradient():
        out[0] = H.sgp_kgrad(Xd, Yd, z, ell, Q, R, x_grad=True)[2]

    def f_backward():
        sess.data_buffer(_part(m, "Hbar")).copy_(out[0])
        torch.cuda.synchronize()
        bwd.run()
        bwd.check()

    forms = dict(forward=f_forward, statistics=lambda: gp._statistics_f64(sess, Xd, Yd, z, ell, W), gradient=f_gradient,
                 backward=f_backward, whole=m.bound_and_grad)
    times = alternate(forms, reps)
    lines.append("DeepKernelSVGP.bound_and_grad() at N=%d M=%d, net [8, 64, 64, 2] tanh, float32 session, median of %d:"
                 % (N, M, reps))
    report(lines, times, [(k, "whole") for k in ("forward", "statistics", "gradient", "backward")])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--N", type=int, default=1000000)
    ap.add_argument("--M", type=int, default=512)
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    other = other_kgrad(args.other_lib) if args.other_lib else None
    lines = ["input gradient of the sparse-GP gradient pass (tools/bench_sgp_kgrad_x.py) on %s" % (H.device_info()[0],)]
    for d in (1, 2, 4):
        n0 = len(lines)
        kernels(args.N, args.M, d, args.reps, other, lines)
        print("\n".join(lines[n0:]), flush=True)
    n0 = len(lines)
    deep_kernel(100000, 128, args.reps, lines)
    print("\n".join(lines[n0:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
