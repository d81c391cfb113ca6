"""Plain float64 numpy references of the kernels that carry the optimiser step and the amortised / full-rank posteriors:
the fused encoder (hb_mlp2_sample_fwd / _bwd), the full-rank sampler (hb_fullrank_sample_kl_fwd / _fwd1 / _bwd), one Adam
step (hb_adam_step) and the middle-axis reductions (hb_reduce).  Written from include/henbun_hip.h and the file-head
comments of csrc/mlp.hip, csrc/variational.hip, csrc/adam.hip -- the formulas, not the kernel bodies.

The second half restates the LAUNCHERS' arithmetic (which kernel form, how many row chunks, how many grid-stride trips) so
that tests/test_step_kernels_cpu.py can assert that the shapes of tests/test_step_kernels_gpu.py still reach the paths they
were chosen for; if a launcher's thresholds move, that file fails and says which shape lost its purpose."""
import numpy as np

L = 16            # latent dimensions of the fused encoder (32 outputs = [mu | log-std])


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------ encoder
def act(name, v):
    v = _f64(v)
    if name == "sigmoid":
        e = np.exp(-np.abs(v))                      # no overflow at |v| = 40 and beyond
        return np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    if name == "relu":
        return np.where(v > 0, v, 0.0)
    if name == "tanh":
        return np.tanh(v)
    raise ValueError(name)


def act_grad_from_output(name, h):
    """The activation's derivative written through its OUTPUT h."""
    if name == "sigmoid":
        return h * (1.0 - h)
    if name == "relu":
        return (h > 0).astype(np.float64)
    if name == "tanh":
        return 1.0 - h * h
    raise ValueError(name)


def encoder_fwd(y, w0, b0, w1, b1, name, u):
    """o = act(y w0 + b0) w1 + b1, x = mu + exp(s) u, kl = -0.5 sum(2 s + u^2 - x^2).
    Returns a dict: pre (pre-activations), h, o, x, kl and the natural scales of the sums (o_scale = |h| |w1| + |b1|,
    kl_scale = 0.5 sum(|2 s| + u^2 + x^2))."""
    y, w0, b0, w1, b1, u = (_f64(a) for a in (y, w0, b0, w1, b1, u))
    pre = y @ w0 + b0.reshape(1, -1)
    h = act(name, pre)
    o = h @ w1 + b1.reshape(1, -1)
    mu, s = o[:, :L], o[:, L:]
    x = mu + np.exp(s) * u
    kl = -0.5 * np.sum(2.0 * s + u * u - x * x)
    return dict(pre=pre, h=h, o=o, x=x, kl=kl,
                pre_scale=np.abs(y) @ np.abs(w0) + np.abs(b0).reshape(1, -1),
                o_scale=np.abs(h) @ np.abs(w1) + np.abs(b1).reshape(1, -1),
                x_scale=np.abs(mu) + np.exp(s) * np.abs(u),
                kl_scale=0.5 * np.sum(np.abs(2.0 * s) + u * u + x * x))


def encoder_vjp(y, w0, b0, w1, name, s, u, x, xbar, klbar):
    """Closed-form VJP of sum(xbar * x) + klbar * kl with respect to (w0, b0, w1, b1), from the operands the C entry takes:
    the log-std half s of o, the noise u and the sample x of the forward.  xbar / klbar None = 0.
        mubar = xbar + klbar x ;  sbar = mubar exp(s) u - klbar ;  do = [mubar | sbar]
        dw1 = h^T do ; db1 = colsum(do) ; dh = do w1^T ; dpre = dh o act'(h) ; dw0 = y^T dpre ; db0 = colsum(dpre)."""
    y, w0, b0, w1, s, u, x = (_f64(a) for a in (y, w0, b0, w1, s, u, x))
    kb = 0.0 if klbar is None else float(np.asarray(klbar).reshape(-1)[0])
    xb = np.zeros_like(x) if xbar is None else _f64(xbar)
    h = act(name, y @ w0 + b0.reshape(1, -1))
    mubar = xb + kb * x
    sbar = mubar * np.exp(s) * u - kb
    do = np.concatenate([mubar, sbar], axis=1)
    dpre = (do @ w1.T) * act_grad_from_output(name, h)
    return y.T @ dpre, dpre.sum(0), h.T @ do, do.sum(0)


# ---------------------------------------------------------------------------------------------------- full-rank sampler
def tri_pack(S):
    """[rows, size, size] -> [rows, size (size + 1) / 2], numpy tril_indices (row-major) order."""
    i, j = np.tril_indices(S.shape[-1])
    return np.ascontiguousarray(S[:, i, j])


def tri_unpack(Sp, size):
    i, j = np.tril_indices(size)
    S = np.zeros((Sp.shape[0], size, size), dtype=Sp.dtype)
    S[:, i, j] = Sp
    return S


def fullrank_fwd(mu, S, u, packed=False):
    """x_r = mu_r + tril(S_r) u_r ;  kl = -0.5 sum(log S_kk^2 + u^2 - x^2).  S dense [rows, size, size] (whatever sits above the
    diagonal is not read: only the entries j <= k are indexed) or packed.  Returns (x, kl, x_scale, kl_scale)."""
    mu, u = _f64(mu), _f64(u)
    rows, size = mu.shape
    Sp = _f64(S) if packed else tri_pack(_f64(S))
    i, j = np.tril_indices(size)
    x, xs = mu.copy(), np.abs(mu)
    terms = Sp * u[:, j]                             # S_kj u_j, j <= k
    np.add.at(x, (slice(None), i), terms)
    np.add.at(xs, (slice(None), i), np.abs(terms))
    d = Sp[:, i == j]                                # the diagonal, in order of k
    ld = np.log(d * d)
    kl = -0.5 * np.sum(ld) - 0.5 * np.sum(u * u - x * x)
    return x, kl, xs, 0.5 * (np.sum(np.abs(ld)) + np.sum(u * u + x * x))


def fullrank_vjp(S, u, x, xbar, klbar, packed=False):
    """mubar = xbar + klbar x ;  Sbar[k][j < k] = mubar_k u_j ;  Sbar[k][k] = mubar_k u_k - klbar / S_kk ;  dense: zero above the
    diagonal; packed: S's layout.  x is the forward's sample (an operand of the C entry)."""
    u, x = _f64(u), _f64(x)
    rows, size = u.shape
    kb = 0.0 if klbar is None else float(np.asarray(klbar).reshape(-1)[0])
    mubar = (np.zeros_like(x) if xbar is None else _f64(xbar)) + kb * x
    i, j = np.tril_indices(size)
    Sp = _f64(S) if packed else _f64(S)[:, i, j]
    Sb = mubar[:, i] * u[:, j]
    dg = i == j
    Sb[:, dg] -= kb / Sp[:, dg]
    return mubar, (Sb if packed else tri_unpack(Sb, size))


# ------------------------------------------------------------------------------------------------------------------ Adam
def adam_step(theta, g, m, v, t, lr, b1, b2, eps, gscale):
    """One TensorFlow-1 Adam step: epsilon is added to the sqrt(v') that is NOT bias-corrected.  Returns (theta', m', v', t')."""
    theta, g, m, v = (_f64(a) for a in (theta, g, m, v))
    t1 = int(t) + 1
    gs = gscale * g
    m1 = b1 * m + (1.0 - b1) * gs
    v1 = b2 * v + (1.0 - b2) * gs * gs
    lr_t = lr * np.sqrt(1.0 - b2 ** t1) / (1.0 - b1 ** t1)
    return theta - lr_t * m1 / (np.sqrt(v1) + eps), m1, v1, t1


# ------------------------------------------------------------------------------------------------------------ reductions
def reduce_mid(x, op):
    """Sum or max over the middle axis of [K1, R, K2]; the sum of an empty axis is 0."""
    x = _f64(x)
    return x.sum(1) if op == "sum" else x.max(1)


# =================================================================================================== launcher arithmetic
def mlp2_fwd_trips(n):
    """(grid, trips of the first wave) of hb_mlp2_sample_fwd_f32: workgroups of four 32-row tiles, at most 1024 of them."""
    ntiles = n // 32
    grid = min((ntiles + 3) // 4, 1024)
    return grid, len(range(0, ntiles, grid * 4))


def mlp2_bwd_partition(n, hid):
    """The row chunks of hb_mlp2_sample_bwd_f32: a list with one [tiles of wave 0, .., tiles of wave 3] per chunk."""
    ntiles = n // 32
    want = min(256 // (hid // 64), ntiles // 4)
    chunks = max(1, min(128, want))
    per = -(-ntiles // chunks)
    out = []
    for c in range(chunks):
        t0, t1 = c * per, min(c * per + per, ntiles)
        out.append([list(range(t0 + w, t1, 4)) for w in range(4)])
    return out


def fullrank_fwd_form(rows, size):
    """(kernel, launches, trips) of hb_fullrank_sample_kl_fwd1 with a sync word: 'thread' (size <= 64) or 'wave', one launch
    or three, and the trips of the capped grid's stride loop in the three-launch form."""
    n = rows * size
    if size <= 64:
        return "thread", 3, 1
    one = size <= 1024 and n <= 8192 and rows * ((size + 1) // 2) <= 4 * 2048
    grid = max(1, min((n + 3) // 4, 2048))
    return "wave", (1 if one else 3), -(-n // (grid * 4))


def adam_form(n, elem_bytes, base_offset_bytes):
    """(kernel, vector tail) of hb_adam_step: 'block' (n <= 2048, one workgroup, tick inside), 'vec' (16-byte lanes; the
    n % (16 / elem_bytes) tail one by one) or 'scalar' (several workgroups, a base that is not 16-byte aligned)."""
    if n <= 2048:
        return "block", 0
    if base_offset_bytes % 16 == 0:
        return "vec", n % (16 // elem_bytes)
    return "scalar", 0


def reduce_split(K1, R, K2, ws_elems=1 << 16):
    """(kernel, S) of hb_reduce: 'rows' (K2 == 1) or 'cols', and the number of R-splits of its first pass."""
    S = 1
    if K2 == 1:
        if K1 < 64 and R > 16384:
            S = min(R // 4096, max(256 // K1, 1))
            if S * K1 > ws_elems:
                S = 1
        return "rows", S
    blocks = -(-K2 // 64) * K1
    if blocks < 128 and R > 2048:
        S = min(R // 512, max(512 // blocks, 1))
        if S * K1 * K2 > ws_elems:
            S = 1
    return "cols", S
