"""Digest of everything the two K-loops compute (gmv_tiles of csrc/gram_matvec.cuh; pw_value_tiles of
csrc/sgp_pathwise.cuh and its copy in sgp_pathwise_grad_kernel), for comparing two trees bit by bit.

    python tools/kloop_digest.py > digest.txt

Fixed-seed problems, the PUBLIC hip_ops entries only (so the script runs unchanged on an older tree), one line
`name sha256` per returned tensor, taken over its float64 bytes, as tools/closed_form_digest.py does.  Two runs of one tree
must agree first (the kernels fold in fixed order); then two trees whose kernels differ only in where the loop lives must
agree line by line.

Gram entries (gram_matvec, gram_predict without a tail and with an EI tail and arg-max, gram_predict_grad), both dtypes,
d in 1 .. 5 (5: the any-d form, the dimensions in two groups), (n, N, S) =
    (1, 1, 1)            a single point
    (130, 2047, 17)      one chunk; ragged strip, K-step and row tile
    (257, 2049, 33)      two chunks; crosses the gradient kernel's 32 right-hand sides
    (130, 34817, 65)     17 full chunks plus one row: the running double sum between groups; crosses the value kernel's 64
and gram_matvec's symmetric form with a non-zero shift at n = N = 130, S = 3.
Pathwise entries (sgp_pathwise, _grad, _argmax, _acq): the shapes of tests/test_pathwise_grad_gpu.py with both lengthscale
layouts, both dtypes."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from henbun_amd import hip_ops as H  # noqa: E402

TORCH = {"float32": torch.float32, "float64": torch.float64}
GRAM = [(1, 1, 1), (130, 2047, 17), (257, 2049, 33), (130, 34817, 65)]
# (n, L, M, d, S)
PATHWISE = [(1, 1, 0, 1, 1), (70, 33, 0, 1, 3), (257, 64, 96, 2, 5), (1000, 130, 160, 3, 17), (300, 16, 40, 5, 2), (130, 8, 8, 1, 65)]


def digest(name, v):
    if isinstance(v, (tuple, list)):
        for i, a in enumerate(v):
            digest("%s.%d" % (name, i), a)
    elif v is not None:
        a = np.ascontiguousarray(v.cpu().numpy(), dtype=np.float64)
        print("%s %s" % (name, hashlib.sha256(a.tobytes()).hexdigest()), flush=True)


def dev(a, dtype):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=TORCH[dtype]).cuda().contiguous()


def gram_routes(dtype, d, n, N, S):
    tag = "%s.gram.d%d.n%d.N%d.S%d." % (dtype, d, n, N, S)
    rng = np.random.default_rng(1000 * d + n + N + S)
    x, x2 = rng.uniform(0.0, 4.0, (n, d)), rng.uniform(0.0, 4.0, (N, d))
    ell = 0.7 + 0.2 * np.arange(d)
    V = rng.standard_normal((S, N)) / np.sqrt(N * S)   # sum of squares of the cache rows' products below 1: prior 2 never clamps
    x, x2, ell, V = (dev(a, dtype) for a in (x, x2, ell, V))
    tail = dict(P=1, scale=1.3, prior=2.0, acq="ei", best=0.01, param=0.01, var_floor=1e-6)
    digest(tag + "gram_matvec", H.gram_matvec(x, x2, ell, V, scale=1.3))
    digest(tag + "gram_predict", H.gram_predict(x, x2, ell, V, P=min(2, S), scale=1.3, prior=2.0))
    digest(tag + "gram_predict.ei", H.gram_predict(x, x2, ell, V, value=True, argmax=True, **tail))
    digest(tag + "gram_predict_grad", H.gram_predict_grad(x, x2, ell, V, P=min(2, S), scale=1.3, prior=2.0))
    digest(tag + "gram_predict_grad.ei", H.gram_predict_grad(x, x2, ell, V, **tail))


def symmetric_route(dtype, d):
    rng = np.random.default_rng(77 + d)
    x, V = rng.uniform(0.0, 4.0, (130, d)), rng.standard_normal((3, 130))
    x, ell, V = dev(x, dtype), dev(0.7 + 0.2 * np.arange(d), dtype), dev(V, dtype)
    digest("%s.gram.d%d.symmetric.shift" % (dtype, d), H.gram_matvec(x, None, ell, V, scale=1.3, shift=0.4))


def pathwise_routes(dtype, n, L, M, d, S, dl):
    tag = "%s.pathwise.n%d.L%d.M%d.d%d.S%d.dl%d." % (dtype, n, L, M, d, S, dl)
    rng = np.random.default_rng(n + L + M + d + S + dl)
    x, omega = rng.uniform(0.0, 8.0, (n, d)), rng.standard_normal((L, d))
    z = rng.uniform(0.0, 8.0, (M, d)) if M else None
    ell = np.array([0.8]) if dl == 1 else 0.7 + 0.2 * np.arange(d)
    coef = rng.standard_normal((S, 2 * L + M))
    coef[:, 2 * L:] *= 1e3
    inc = rng.standard_normal(S)
    x, omega, z, ell, coef, inc = (dev(a, dtype) for a in (x, omega, z, ell, coef, inc))
    digest(tag + "sgp_pathwise", H.sgp_pathwise(x, omega, z, ell, coef, scale=1.7))
    digest(tag + "sgp_pathwise_grad", H.sgp_pathwise_grad(x, omega, z, ell, coef, scale=1.7))
    for largest in (True, False):
        digest(tag + "sgp_pathwise_argmax.%d" % largest, H.sgp_pathwise_argmax(x, omega, z, ell, coef, scale=1.7, largest=largest))
        for acq in ("ei", "pi"):
            digest(tag + "sgp_pathwise_acq.%s.%d" % (acq, largest),
                   H.sgp_pathwise_acq(x, omega, z, ell, coef, inc, scale=1.7, acq=acq, largest=largest))


def main():
    for dtype in ("float32", "float64"):
        for d in (1, 2, 3, 4, 5):
            for n, N, S in GRAM:
                gram_routes(dtype, d, n, N, S)
            symmetric_route(dtype, d)
        for shape in PATHWISE:
            for dl in sorted({1, shape[3]}):
                pathwise_routes(dtype, *shape, dl)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
