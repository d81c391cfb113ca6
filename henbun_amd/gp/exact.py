"""Exact GP regression by conjugate gradients (not in the reference; Gardner et al. 2018, Wang et al. 2019).

K^ = k_var K(X, X) + noise_var I is never formed: every product K^ V is one hb_gram_matvec, which synthesises the kernel
values in LDS and contracts them on the MFMA for up to 64 right-hand sides at a time.  Memory is O(N (S + R)) for S
right-hand sides and a rank-R preconditioner -- five vectors [S, N], the factor [R, N] and the product's workspace, at
most (16 sizeof(T) + 8) S N bytes (hb_gram_matvec_ws_elems); time is N^2 d kernel evaluations per iteration.  The vector
updates, the dot products and every scalar of the iteration run in the library's own kernels (hb_pcg_*: the scalars in
double); torch allocates, copies and converts dtypes, nothing else.

The log marginal likelihood and its gradient (log_marginal_likelihood below; GP.log_marginal_likelihood_and_grad,
ExactGPR.fit_hyper) come from the same machinery: one lockstep solve over the rows [Y columns; probes] (per block of 64
rows) whose recurrence
coefficients, logged by hb_pcg_*_coef, give the log-determinant by stochastic Lanczos quadrature at no extra product, then
ONE hb_gram_bilinear_grad -- a pass over the N^2 kernel entries that contracts K and dK/d ell against all the pairs of
vectors of the gradient's traces -- and a host tail in float64.

The predictive variance costs a solve per 64 test points; VarianceCache below replaces it, where an upper bound will do,
by the Galerkin restriction of K^^-1 to the span of the preconditioner's basis: predict_f(var='cache'), acquisition and
argmax are then ONE hb_gram_predict pass over any number of points.

Out of scope: kernels other than UnitRBF, non-Gaussian likelihoods, variance reduction of the trace estimators beyond
the preconditioner.
"""
from __future__ import annotations

import numpy as np

from .._settings import settings
from . import _host
from .sparse import PathwiseDraws


class NotConverged(RuntimeError):
    """pcg_solve did not reach its tolerance within max_iter; `info` is the dict a converged solve returns."""

    def __init__(self, message, info):
        RuntimeError.__init__(self, message)
        self.info = info


class Preconditioner:
    """P = k_var C^T C + noise_var I with C [R, N] the pivoted incomplete Cholesky factor of K(X, X) that hb_sgp_select
    leaves at the start of its workspace (threshold 0; R = the rows it produced, at most `rank`), in the dtype of X.
    apply() forms w = C^T (noise_var I + k_var C C^T)^-1 C r, so that by Woodbury P^-1 r = (r - k_var w) / noise_var;
    the R x R Cholesky and the two triangular products are float64, the two N-sized products run in the dtype of X."""

    def __init__(self, sess, Xd, ell, k_var, noise_var, rank):
        torch, H = sess.torch, sess.H
        N, d = Xd.shape
        self._H, self._torch = H, torch
        self.k_var, self.noise_var = float(k_var), float(noise_var)
        want = min(int(rank), N, 8192)
        self.N, self.ld = N, (N + 63) // 64 * 64
        self.C = torch.empty(H.sgp_select_ws_elems(Xd.dtype, N, want, d), dtype=Xd.dtype, device=Xd.device)
        _, _, count, _ = H.sgp_select(Xd, ell, want, 0.0, ws=self.C)
        self.rank = R = int(count.cpu()[0])       # the selection stops early when no conditional variance is left
        G = H.matmul_ld(self.C, self.ld, self.C, self.ld, torch.empty((R, R), dtype=Xd.dtype, device=Xd.device), R, R, N,
                        transB=True, alpha=self.k_var)
        G = H.matutil(G.to(torch.float64), H.MATUTIL_ADD_EYE, alpha=self.noise_var)
        self.Linv = H.trinv(_host.factor(H, G, "Preconditioner", "noise_var I + k_var C C^T (rank %d)" % R, RuntimeError))

    def apply(self, r, out):
        """out [S, N] = C^T (noise_var I + k_var C C^T)^-1 C r for the rows of r [S, N]."""
        torch, H = self._torch, self._H
        S, R, N = r.shape[0], self.rank, self.N
        t = H.matmul_ld(r, N, self.C, self.ld, torch.empty((S, R), dtype=r.dtype, device=r.device), S, R, N, transB=True)
        u = H.matmul(H.matmul(t.to(torch.float64), self.Linv, transB=True), self.Linv)
        return H.matmul_ld(u.to(r.dtype).contiguous(), R, self.C, self.ld, out, S, N, R)


_COEF_BLOCK = 256   # iterations per block of the coefficient log (record=True)


class _CoefLog:
    """The coefficient log of a recorded solve: blocks [2 _COEF_BLOCK, S] of NaN that `new_block()` allocates as the
    iteration reaches them (device tensors in pcg_solve; anything numpy converts elsewhere), handed to the recording steps
    by slot(i) while the log is open.  stop() closes it (the first restart): later iterations get no slot and no block.
    assemble(iterations, rows) turns the ONE read-back of the blocks into [iterations, 2, S] whatever was allocated -- iterations past
    the last block (everything after a stop) are NaN rows, i.e. 'no coefficient'."""

    def __init__(self, S, new_block, block=_COEF_BLOCK):
        self.S, self.block, self._new, self.blocks, self.open = int(S), int(block), new_block, [], True

    def slot(self, i):
        """(the block iteration i writes to, i's index in it), or (None, 0) once the log is closed"""
        if not self.open:
            return None, 0
        while i // self.block >= len(self.blocks):
            self.blocks.append(self._new())
        return self.blocks[i // self.block], i % self.block

    def stop(self):
        self.open = False

    def assemble(self, iterations, rows):
        """rows: the blocks concatenated, as numpy [2 block len(blocks), S] (None without blocks)"""
        coef = np.full((iterations, 2, self.S), np.nan)
        if rows is not None:
            got = np.asarray(rows, dtype=np.float64).reshape(-1, 2, self.S)
            n = min(iterations, got.shape[0])
            coef[:n] = got[:n]
        return coef


def pcg_solve(sess, Xd, ell, k_var, noise_var, B, precond=None, tol=None, max_iter=1000, record=False):
    """Solve (k_var K(X, X) + noise_var I) x_s = b_s for the S rows of B [S, N] by S preconditioned conjugate-gradient
    iterations run in lockstep, each with its own alpha_s, beta_s: ONE hb_gram_matvec per iteration for all of them.
    Xd [N, d], ell [1] or [d] and B are device tensors of one dtype.  precond: a Preconditioner of the same X and
    hyper-parameters, or None for plain CG.  Stops when |r_s| <= tol |b_s| for every s (tol=None: 1e-6 in float64, 1e-3 in
    float32); a row that has converged stops moving.  One host read-back per iteration (the S residual norms).  When the
    recurrence reports convergence the residual b - K^ x is formed with one more product; should it be above the
    tolerance (the recurrence drifts in float32) the iteration restarts from it.  Returns (x [S, N], info) with info =
    dict(iterations, restarts, residual [S] = |b - K^ x| / |b| from that last product, converged, precond_rank):
    `iterations` counts the products with a search direction, `restarts` the times the iteration was restarted (each
    costs one product more, as does the final check); raises NotConverged, carrying the same info, after max_iter
    iterations.
    record=True logs the recurrence (hb_pcg_update_coef / hb_pcg_direction_coef; x is the same bits) and adds to info
    coef [iterations, 2, S] float64 -- alpha_j, beta_j per row, NaN from where a row had converged -- read back ONCE after
    the loop, rz0 [S] = r . P^-1 r of the first direction, and lanczos_steps [S], the leading steps of each row that form
    one three-term recurrence.  A restart breaks the recurrence: recording stops at the first one."""
    torch, H = sess.torch, sess.H
    S, N = B.shape
    dt, dev = B.dtype, B.device
    if tol is None:
        tol = 1e-6 if dt == torch.float64 else 1e-3
    tol, k_var, noise_var = float(tol), float(k_var), float(noise_var)
    if not (tol > 0.0 and k_var > 0.0 and noise_var > 0.0):
        raise ValueError("pcg_solve: tol, k_var and noise_var must be positive (got %r, %r, %r)" % (tol, k_var, noise_var))
    if precond is not None and precond.rank == 0:
        precond = None
    new = lambda: torch.empty((S, N), dtype=dt, device=dev)
    x, r, p, Ap = H.fill(new(), 0.0), H.ewise("COPY", [B]), new(), new()
    w = new() if precond is not None else None
    gws = torch.empty(max(H.gram_matvec_ws_elems(dt, N, N, S), 1), dtype=dt, device=dev)
    product = lambda V: H.gram_matvec(Xd, None, ell, V, scale=k_var, shift=noise_var, out=Ap, ws=gws)

    bb = H.pcg_dot(B, B)
    rr, rz = H.ewise("COPY", [bb]), torch.empty_like(bb)
    bb_h = bb.cpu().numpy()
    thr_h = tol * tol * bb_h
    thr = torch.as_tensor(thr_h).to(dev)

    log = _CoefLog(S, lambda: H.fill(torch.empty((2 * _COEF_BLOCK, S), dtype=torch.float64, device=dev), float("nan")))
    if not record:
        log.stop()
    log_of = log.slot

    def direction(first, i=None):
        if precond is not None:
            precond.apply(r, w)
        coef, at = (None, 0) if i is None else log_of(i)
        H.pcg_direction(r, w, p, rz, rr, thr, wscale=k_var, zscale=1.0 / noise_var if precond is not None else 1.0, first=first,
                        coef=coef, it=at)

    def true_residual():
        product(x)
        H.ewise("SUB", [B, Ap], out=r)
        H.pcg_dot(r, r, out=rr)
        return rr.cpu().numpy()

    rr_h, it, restarts, converged = bb_h, 0, 0, False
    direction(True)
    rz0 = H.ewise("COPY", [rz]) if record else None
    while True:
        if np.all(rr_h <= thr_h):
            rr_h = true_residual()           # r and rr now hold the residual itself
            if np.all(rr_h <= thr_h):
                converged = True
                break
            if it >= max_iter:
                break
            direction(True)                  # the recurrence had drifted: restart from the residual
            restarts += 1
            log.stop()
        elif it >= max_iter:
            rr_h = true_residual()
            break
        product(p)
        coef, at = log_of(it)
        H.pcg_update(x, r, p, Ap, rz, rr, thr, coef=coef, it=at)
        rr_h = rr.cpu().numpy()
        it += 1
        if not np.all(rr_h <= thr_h):
            direction(False, it - 1)
    residual = np.sqrt(rr_h / np.where(bb_h > 0.0, bb_h, 1.0))
    info = dict(iterations=it, restarts=restarts, residual=residual, converged=converged,
                precond_rank=0 if precond is None else precond.rank)
    if record:
        coef = log.assemble(it, torch.cat(log.blocks).cpu().numpy() if log.blocks else None)   # the one read-back
        rz0_h = rz0.cpu().numpy()
        rz0_h[~(bb_h > thr_h)] = 0.0          # a row that never started (b = 0) was never written
        info.update(coef=coef, rz0=rz0_h, lanczos_steps=_lanczos_steps(coef))
    if not converged:
        raise NotConverged("pcg_solve: %d iterations did not reach |r| <= %g |b| (largest residual %g)"
                           % (it, tol, float(residual.max())), info)
    return x, info


def _lanczos_steps(coef):
    """[S]: the leading alpha_j of each row of coef [iterations, 2, S] that are positive (NaN: the row had stopped)."""
    ok = coef[:, 0, :] > 0.0
    return np.where(ok.all(0), coef.shape[0], np.argmin(ok, axis=0)).astype(np.int64) if coef.shape[0] else np.zeros(coef.shape[2], np.int64)


def lanczos_logquad(alpha, beta):
    """e_1^T log(T) e_1 for the Lanczos tridiagonal T [m, m] of a CG recurrence with coefficients alpha [m], beta [>= m - 1]:
    diagonal 1 / alpha_0, then 1 / alpha_j + beta_{j-1} / alpha_{j-1}; off-diagonal sqrt(beta_{j-1}) / alpha_{j-1}.  numpy
    float64 on the host (m is at most the iteration count); m = 0 gives 0."""
    alpha = np.asarray(alpha, dtype=np.float64)
    m = alpha.shape[0]
    if m == 0:
        return 0.0
    beta = np.asarray(beta, dtype=np.float64)[:m - 1]
    T = np.diag(1.0 / alpha)
    if m > 1:
        T[np.arange(1, m), np.arange(1, m)] += beta / alpha[:-1]
        off = np.sqrt(beta) / alpha[:-1]
        T[np.arange(1, m), np.arange(m - 1)] = off
        T[np.arange(m - 1), np.arange(1, m)] = off
    lam, V = np.linalg.eigh(T)
    return float(np.sum(V[0] ** 2 * np.log(lam)))


def log_marginal_likelihood(sess, Xd, Yt, ell, k_var, noise_var, precond, tol, max_iter, num_probes=16, seed=0, probes=None,
                            grad=True):
    """The log marginal likelihood of Y = f(X) + N(0, noise_var), f ~ GP(0, k_var k), and its gradient, without the [N, N]
    matrix (Gardner et al. 2018).  With K^ = k_var K(X, X) + noise_var I, alpha_c = K^^-1 y_c, P_ the preconditioner (I
    without one) and T probes z_t with E[z z^T] = P_, u_t = K^^-1 z_t:
        L = -1/2 sum_c y_c . alpha_c - P/2 logdet K^ - N P / 2 log 2 pi
        dL/dtheta = sum_c 1/2 alpha_c^T (dK^/dtheta) alpha_c - P / (2 T) sum_t u_t^T (dK^/dtheta) P_^-1 z_t
        logdet K^ ~ logdet P_ + 1/T sum_t (z_t^T P_^-1 z_t) e_1^T log(T_t) e_1
    T_t being the Lanczos tridiagonal of probe t's own CG recurrence (lanczos_logquad).  The rows [Y columns; probes] are
    solved in lockstep by pcg_solve(record=True) -- ONE solve for P + T <= 64, otherwise one per block of 64 rows, each with
    its own iteration count --, then ONE hb_gram_bilinear_grad over all P + T pairs and one hb_pcg_dot;
    the N^2 work in the session's dtype, every scalar double.  Xd [N, d], Yt [P, N], ell device tensors of the session's
    dtype; precond a Preconditioner of the same hyper-parameters or None.  Default probes: z_t = sqrt(k_var) eps1 C +
    sqrt(noise_var) eps2 with eps1 [T, R], eps2 [T, N] from hip_ops.Rng(seed) in that order (no preconditioner: z_t = eps2);
    probes= injects Z [T, N] as given.  Returns (value, grad, info): grad = dict(lengthscales [dl], k_var, noise_var)
    float64 with respect to the constrained values (None with grad=False); info = the solve's info -- with several blocks
    `iterations` and `restarts` are SUMS over the blocks' solves, residual / rz0 / coef concatenated over the rows, coef
    NaN-padded to the longest block -- plus
    logdet, logdet_precond, num_probes and lanczos_steps [T] (the probes' rows).  The estimate is a deterministic function
    of (seed or probes); its distance from the exact value is the estimator's variance."""
    torch, H = sess.torch, sess.H
    P, N = Yt.shape
    dt, dev = Yt.dtype, Yt.device
    k_var, noise_var = float(k_var), float(noise_var)
    if precond is not None and precond.rank == 0:
        precond = None
    if probes is None:
        T = int(num_probes)
        if T < 1:
            raise ValueError("log_marginal_likelihood: num_probes >= 1 expected (got %r)" % (num_probes,))
        rng = H.Rng(seed, device=dev)
        if precond is None:
            Z = rng.normal((T, N), dtype=dt)
        else:
            R = precond.rank
            e1, e2 = rng.normal((T, R), dtype=dt), rng.normal((T, N), dtype=dt)
            Z = H.matmul_ld(e1, R, precond.C, precond.ld, torch.empty((T, N), dtype=dt, device=dev), T, N, R,
                            alpha=np.sqrt(k_var))
            Z = H.ewise("ADD", [Z, H.ewise("AFFINE", [e2], params=(np.sqrt(noise_var), 0.0))])
    else:
        if np.ndim(probes) != 2 or np.shape(probes)[1] != N or np.shape(probes)[0] < 1:
            raise ValueError("log_marginal_likelihood: probes must be [T, %d] (got %s)" % (N, np.shape(probes)))
        Z = _host.upload(sess, probes)
        T = Z.shape[0]
    rows = torch.cat([Yt, Z]).contiguous()
    S = P + T
    sol = torch.empty((S, N), dtype=dt, device=dev)
    infos = []
    for a in range(0, S, 64):
        x, inf = pcg_solve(sess, Xd, ell, k_var, noise_var, rows[a:a + 64].contiguous(), precond, tol, max_iter, record=True)
        H.ewise("COPY", [x], out=sol[a:a + 64])
        infos.append(inf)
    iters = max(i["iterations"] for i in infos)
    coef = np.full((iters, 2, S), np.nan)
    for a, i in zip(range(0, S, 64), infos):
        coef[:i["coef"].shape[0], :, a:a + 64] = i["coef"]
    cat = lambda k: np.concatenate([i[k] for i in infos])
    info = dict(iterations=sum(i["iterations"] for i in infos), restarts=sum(i["restarts"] for i in infos),
                residual=cat("residual"), converged=all(i["converged"] for i in infos), precond_rank=infos[0]["precond_rank"],
                coef=coef, rz0=cat("rz0"))
    steps = cat("lanczos_steps")

    if precond is None:
        PinvZ, logdet_p = Z, 0.0
    else:
        PinvZ = H.ewise("AFFINE", [H.ewise("SUB", [Z, H.ewise("AFFINE", [precond.apply(Z, torch.empty_like(Z))],
                                                           params=(k_var, 0.0))])], params=(1.0 / noise_var, 0.0))
        # logdet(noise_var I + k_var C C^T) = 2 sum log diag L = -2 sum log diag L^-1
        logdet_p = (N - precond.rank) * np.log(noise_var) - 2.0 * float(np.log(torch.diagonal(precond.Linv).cpu().numpy()).sum())
    quad = [info["rz0"][P + t] * lanczos_logquad(coef[:steps[P + t], 0, P + t], coef[:steps[P + t], 1, P + t]) for t in range(T)]
    logdet = logdet_p + float(np.sum(quad)) / T
    fit = float(H.pcg_dot(Yt, sol[:P].contiguous()).cpu().numpy().sum())
    value = -0.5 * fit - 0.5 * P * logdet - 0.5 * N * P * np.log(2.0 * np.pi)
    info.update(logdet=logdet, logdet_precond=logdet_p, num_probes=T, lanczos_steps=steps[P:])
    if not grad:
        return value, None, info
    Bm = torch.cat([sol[:P], PinvZ]).contiguous()
    wts = np.concatenate([np.full(P, 0.5), np.full(T, -0.5 * P / T)])
    g = H.gram_bilinear_grad(Xd, ell, sol, Bm, wts).cpu().numpy()
    dots = H.pcg_dot(sol, Bm).cpu().numpy()
    return value, dict(lengthscales=k_var * g[1:], k_var=float(g[0]), noise_var=float(wts @ dots)), info


_CACHE_JITTER = 1e-13        # VarianceCache: T + eps tr(T) / r I is factorised, eps from here ...
_CACHE_JITTER_TRIES = 3      # ... multiplied by 100 after a failed factorisation, at most this many times
_CACHE_PRODUCT_BYTES = 1 << 30   # workspace of the product K^ C above which the rows of C are taken in blocks


class VarianceCache:
    """A cached upper bound of the exact GP's predictive variance (ExactPosterior.build_cache).  For a full-row-rank
    basis C [r, N], the Galerkin restriction of K^ = k_var K(X, X) + noise_var I to span(C^T) gives
        G = C^T (C K^ C^T)^-1 C  <=  K^^-1     (positive semi-definite order),
    so that v_cache(x) = k_var - k*^T G k* = k_var - |R_c k*|^2, R_c = L_T^-1 C, T = C K^ C^T = L_T L_T^T, is
      - an UPPER bound of the exact variance k_var - k*^T K^^-1 k* at every x (conservative error bars),
      - non-increasing as rows are appended to C, and the exact variance once C spans the numerical range of K,
      - one kernel product per point, with no Krylov iteration and no random numbers.
    C is the pivoted incomplete Cholesky factor hb_sgp_select leaves in its workspace (the preconditioner's basis), its
    rows scaled to unit norm; T, its Cholesky factor and R_c are float64 whatever the session's dtype, R_c is rounded
    ONCE to the session's dtype.  The jitter added to T replaces (C K^ C^T)^-1 by something smaller: it can only loosen
    the bound, never break it.  HONEST LIMIT: the bound is tight once r reaches the number of eigenvalues of K that
    matter -- roughly the volume of the data in lengthscale units; on a domain of hundreds of lengthscales a small r
    leaves it loose (still an upper bound).  predict_f(var=True) stays the exact route.
    Building needs 2 r N 8 bytes transiently (C and K^ C, then C and R_c, in float64) beside the selection's own
    workspace; the cache keeps Rc and the basis C, [r, N] each, in the session's dtype."""

    def __init__(self, sess, Xd, ell, k_var, noise_var, rank, threshold, precond=None):
        torch, H = sess.torch, sess.H
        N, d = Xd.shape
        dt, dev, f64 = Xd.dtype, Xd.device, torch.float64
        want = min(int(rank), N, 8192)
        ld = (N + 63) // 64 * 64
        if precond is not None and float(threshold) == 0.0 and precond.rank == want and precond.N == N:
            hist, r = precond.C, precond.rank     # the same selection: its first `want` rows
        else:
            hist = torch.empty(H.sgp_select_ws_elems(dt, N, want, d), dtype=dt, device=dev)
            _, _, count, _ = H.sgp_select(Xd, ell, want, float(threshold), ws=hist)
            r = int(count.cpu()[0])
        if r < 1:
            raise ValueError("build_cache: the selection produced no row (threshold %r)" % (threshold,))
        self.basis = hist[:r * ld].view(r, ld)[:, :N].contiguous()     # C as the selection left it
        C = self.basis.to(f64)
        del hist
        C = H.ewise("MUL", [C, H.ewise("RSQRT", [H.pcg_dot(C, C)]).reshape(r, 1)])      # unit rows
        X64, ell64 = Xd.to(f64), ell.to(f64)
        KC = torch.empty((r, N), dtype=f64, device=dev)
        rows = r
        while rows > 64 and H.gram_matvec_ws_elems(f64, N, N, rows) * 8 > _CACHE_PRODUCT_BYTES:
            rows = (rows // 2 + 63) // 64 * 64    # (a row of the product does not depend on the others: the same bits)
        gws = torch.empty(max(H.gram_matvec_ws_elems(f64, N, N, rows), 1), dtype=f64, device=dev)
        for a in range(0, r, rows):
            H.gram_matvec(X64, None, ell64, C[a:a + rows], scale=float(k_var), shift=float(noise_var), out=KC[a:a + rows], ws=gws)
        del gws
        T = H.matutil(H.matmul(KC, C, transB=True), H.MATUTIL_SYM)
        del KC
        trace = float(torch.diagonal(T).cpu().numpy().sum())
        eps = _CACHE_JITTER
        for attempt in range(_CACHE_JITTER_TRIES + 1):
            try:
                L = _host.factor(H, H.matutil(T, H.MATUTIL_ADD_EYE, alpha=eps * trace / r), "build_cache",
                                 "C K^ C^T + %g tr / r I (rank %d)" % (eps, r), RuntimeError)
                break
            except RuntimeError:
                if attempt == _CACHE_JITTER_TRIES:
                    raise
                eps *= 100.0
        self.Rc = H.matmul(H.trinv(L), C).to(dt).contiguous()            # rounded once
        self.rank = r
        self.info = dict(rank=r, asked=int(rank), jitter=eps, trace=trace)


class ExactPosterior:
    """The exact GP posterior given (X, Y) at fixed hyper-parameters (GP.condition): a snapshot, like PathwiseDraws, of X
    [N, d], the lengthscales, k_var, noise_var, alpha = K^^-1 Y [P, N], the preconditioner and the solve's `info`, on the
    device in the session's dtype.  Later changes to the model do not move it.  build_cache() adds a VarianceCache:
    predict_f(var='cache'), acquisition and argmax then cost ONE kernel product over the candidates, however many, and
    predict_grad, acquisition(grad=True) and maximise add their exact input gradients at 1 + d times that product."""

    KINDS = ("ei", "pi", "ucb")

    def __init__(self, sess, X, Y, ell, k_var, noise_var, alpha, precond, info, tol, max_iter):
        self._sess = sess
        self._X, self._Y, self._ell, self._alpha, self._precond = X, Y, ell, alpha, precond
        self.k_var, self.noise_var, self.info = float(k_var), float(noise_var), info
        self.tol, self.max_iter = tol, int(max_iter)
        self._cache, self._V, self.cache_info = None, None, None

    alpha = property(lambda self: self._alpha.cpu().numpy(), doc="K^^-1 Y as numpy [P, N]")

    def _solve(self, B):
        return pcg_solve(self._sess, self._X, self._ell, self.k_var, self.noise_var, B, self._precond, self.tol, self.max_iter)

    def _new_points(self, Xnew):
        Xn = _host.device_data(self._sess, Xnew, "Xnew")
        if Xn.shape[1] != self._X.shape[1]:
            raise ValueError("ExactPosterior: Xnew %s does not match X %s" % (tuple(Xn.shape), tuple(self._X.shape)))
        return Xn

    def build_cache(self, rank=256, threshold=None):
        """Build the VarianceCache of this posterior (see there for what it bounds and where it is loose) and return
        self.  rank: rows of the pivoted incomplete Cholesky basis asked for (at most N and 8192); the selection stops
        earlier once no conditional variance exceeds `threshold` (None: settings.numerics.jitter_level, the convention
        of greedy_inducing).  The preconditioner's basis is reused when its rank and threshold (0) match.  cache_info =
        dict(rank = rows produced, asked, jitter = the eps of T + eps tr(T) / r I that factorised, trace = tr T).
        Needs 2 r N 8 bytes transiently whatever the session's dtype."""
        thr = float(settings.numerics.jitter_level if threshold is None else threshold)
        if not (int(rank) >= 1 and thr >= 0.0):
            raise ValueError("build_cache: rank >= 1 and threshold >= 0 expected (got %r, %r)" % (rank, threshold))
        self._cache = VarianceCache(self._sess, self._X, self._ell, self.k_var, self.noise_var, rank, thr, self._precond)
        self._V = self._sess.torch.cat([self._alpha, self._cache.Rc]).contiguous()     # [P + r, N]: mean rows, cache rows
        self.cache_info = dict(self._cache.info)
        return self

    cache_basis = property(lambda self: self._need_cache("cache_basis").basis.cpu().numpy(),
                           doc="the basis C [r, N] of the cache as the selection produced it (numpy)")

    def _need_cache(self, who):
        if self._cache is None:
            raise ValueError("%s: no variance cache, call build_cache() first" % who)
        return self._cache

    def _cached(self, Xn, **kw):
        P = self._alpha.shape[0]
        return self._sess.H.gram_predict(Xn, self._X, self._ell, self._V, P=P, scale=self.k_var, prior=self.k_var, **kw)

    def predict_f(self, Xnew, var=True):
        """(mean [P, n], var [n]) of the latent f at the rows of Xnew, as numpy.  The mean is ONE hb_gram_matvec,
        k_var alpha K(X, Xnew).  var = k_var - k*^T K^^-1 k* costs ONE LOCKSTEP SOLVE PER 64 TEST POINTS, each as expensive
        as the conditioning itself (right-hand sides k_var K(X, Xnew_block) from hb_gram_fwd); var=False skips it and
        returns (mean, None).  var='cache': (mean, var_upper) from ONE hb_gram_predict pass over Xnew -- the same mean
        bits and the VarianceCache's upper bound of the variance (build_cache() first, else ValueError)."""
        if isinstance(var, str):
            if var != "cache":
                raise ValueError("predict_f: var must be True, False or 'cache' (got %r)" % (var,))
            self._need_cache("predict_f(var='cache')")
            mean, v, _, _, _ = self._cached(self._new_points(Xnew))
            return mean.cpu().numpy(), v.cpu().numpy()
        torch, H = self._sess.torch, self._sess.H
        Xn = self._new_points(Xnew)
        n = Xn.shape[0]
        mean = H.gram_matvec(Xn, self._X, self._ell, self._alpha, scale=self.k_var).cpu().numpy()
        if not var:
            return mean, None
        out = np.empty(n, dtype=mean.dtype)
        for a in range(0, n, 64):
            blk = Xn[a:a + 64].contiguous()
            rhs = H.ewise("AFFINE", [H.gram_fwd(blk, self._X, self._ell)], params=(self.k_var, 0.0))   # [nb, N]
            sol, _ = self._solve(rhs)
            q = H.ewise("AFFINE", [H.pcg_dot(rhs, sol)], params=(-1.0, self.k_var))                    # float64 [nb]
            out[a:a + 64] = q.cpu().numpy()
        return mean, out

    def predict_y(self, Xnew, var=True):
        """predict_f plus the noise variance: the predictive of a new observation (var='cache': of the upper bound)."""
        mean, v = self.predict_f(Xnew, var=var)
        return mean, None if v is None else v + np.asarray(self.noise_var, dtype=v.dtype)

    def _acq_args(self, who, kind, best, param, var_floor):
        if kind not in self.KINDS:
            raise ValueError("%s: kind must be one of %s, got %r" % (who, self.KINDS, kind))
        if self._alpha.shape[0] != 1:
            raise NotImplementedError("%s: one latent function only (Y has %d columns)" % (who, self._alpha.shape[0]))
        if kind != "ucb" and best is None:
            raise ValueError("%s: the acquisition %r needs `best`, the incumbent value" % (who, kind))
        self._need_cache(who)
        var_floor = self.k_var * float(settings.numerics.jitter_level) if var_floor is None else float(var_floor)
        if not var_floor >= 0.0:
            raise ValueError("%s: var_floor >= 0 expected (got %r)" % (who, var_floor))
        return dict(acq=kind, best=0.0 if best is None else float(best), param=float(param), var_floor=var_floor)

    def _cached_grad(self, Xn, **kw):
        P = self._alpha.shape[0]
        return self._sess.H.gram_predict_grad(Xn, self._X, self._ell, self._V, P=P, scale=self.k_var, prior=self.k_var, **kw)

    def predict_grad(self, X):
        """(mean [P, n], var_upper [n], dmean [P, n, d], dvar [n, d]) as numpy: the moments of predict_f(X, var='cache'),
        bit for bit, and their exact input gradients dmean[p, j, k] = d mean[p, j] / d x_jk from ONE hb_gram_predict_grad
        pass (build_cache() first, else ValueError).  dvar is exactly 0 where the bound was clamped to 0."""
        self._need_cache("predict_grad")
        mean, v, _, dmean, dvar, _ = self._cached_grad(self._new_points(X))
        return mean.cpu().numpy(), v.cpu().numpy(), dmean.cpu().numpy(), dvar.cpu().numpy()

    def acquisition(self, X, kind, best=None, param=0.0, largest=True, var_floor=None, grad=False):
        """The closed-form acquisition `kind` ('ei', 'pi': param = xi, improvement over `best`; 'ucb': param = beta) at
        the rows of X, as numpy [n], from the exact mean and the CACHED variance bound (build_cache() first): ONE
        hb_gram_predict pass, the tail of SparsePosterior.acquisition per point in double.  For maximising f (largest) or
        minimising it; sigma^2 = max(var_upper, var_floor), var_floor=None: k_var * jitter_level as there.  The bound
        makes sigma conservative: exploration is never under-weighted.  One latent function only.  grad=True: (values
        [n], gradient [n, d]), the exact input gradient from ONE hb_gram_predict_grad pass (the same value bits); where
        the variance was clamped the gradient does not pass through it."""
        args = self._acq_args("acquisition", kind, best, param, var_floor)
        if grad:
            _, _, val, _, _, g = self._cached_grad(self._new_points(X), largest=bool(largest), mean=False, var=False, dmean=False,
                                                   dvar=False, **args)
            return val.cpu().numpy(), g.cpu().numpy()
        _, _, val, _, _ = self._cached(self._new_points(X), largest=bool(largest), mean=False, var=False, value=True, **args)
        return val.cpu().numpy()

    def argmax(self, X, kind, best=None, param=0.0, largest=True, var_floor=None):
        """(index, value): the row of X at which acquisition(X, ...) is largest (ties: the first row; a NaN is never
        chosen) and its value there, without writing anything of size n, so X can be millions of candidates.  No
        comparable value: (-1, -inf)."""
        args = self._acq_args("argmax", kind, best, param, var_floor)
        Xd = self._new_points(X)
        if Xd.shape[0] < 1:
            raise ValueError("argmax: at least one candidate expected")
        _, _, _, bv, bi = self._cached(Xd, largest=bool(largest), mean=False, var=False, value=False, argmax=True, **args)
        return int(bi.cpu().numpy()[0]), self._sess.np_dtype(bv.cpu().numpy()[0])

    def maximise(self, X, kind, best=None, param=0.0, largest=True, var_floor=None, steps=50, lr=0.05, bounds=None, starts=None):
        """(x_best [R, d], a_best [R], info): the acquisition maximised over the box `bounds` by `steps` steps of projected
        Adam ascent on its exact input gradient, from its best candidate among the rows of X (R = 1, found by argmax), or
        from every row of starts [R, d].  The contract of SparsePosterior.maximise: the optimiser runs on the host in
        float64, in lengthscale units so that lr is a fraction of a lengthscale, each evaluation ONE
        hb_gram_predict_grad pass at the R current points rounded to the session's dtype; bounds = (lo [d], hi [d]),
        default the per-column minimum and maximum of X.  The best (value, point) seen is kept, the start included:
        a_best is never below the start's value and is the bits of acquisition(x_best).  info = dict(start_idx (None
        with starts), start_value [R], steps).  steps < 0, lr <= 0, malformed bounds or starts and X of another width
        raise ValueError."""
        sess = self._sess
        args = self._acq_args("maximise", kind, best, param, var_floor)
        Xd = self._new_points(X)
        d, dt = int(Xd.shape[1]), np.dtype(sess.np_dtype).type
        steps = int(steps)
        if steps < 0 or not float(lr) > 0.0:
            raise ValueError("maximise: steps >= 0 and lr > 0 expected (got %r, %r)" % (steps, lr))
        if Xd.shape[0] < 1:
            raise ValueError("maximise: at least one candidate expected")
        box = _host.ascent_box("maximise", Xd, bounds, d, dt)
        ell = np.broadcast_to(np.asarray(self._ell.cpu().numpy(), np.float64), (d,))

        def evaluate(xc):
            _, _, val, _, _, g = self._cached_grad(_host.upload(sess, xc), largest=bool(largest), mean=False, var=False,
                                                   dmean=False, dvar=False, **args)
            return val.cpu().numpy(), g.cpu().numpy().astype(np.float64)

        if starts is None:
            _, _, _, bv, bi = self._cached(Xd, largest=bool(largest), mean=False, var=False, value=False, argmax=True, **args)
            idx, f0 = bi.cpu().numpy(), bv.cpu().numpy().astype(dt)   # (best_val is the value's bits, widened)
            if idx[0] < 0:
                raise ValueError("maximise: the acquisition has no comparable value among the candidates")
            x = Xd[bi].cpu().numpy()
        else:
            x = np.ascontiguousarray(np.asarray(starts, dtype=dt))
            if x.ndim != 2 or x.shape[1] != d or x.shape[0] < 1:
                raise ValueError("maximise: starts [R, %d] expected, got %s" % (d, x.shape))
            idx, f0 = None, evaluate(x)[0]
        info = dict(start_idx=idx, start_value=f0.copy(), steps=steps)
        x_best, a_best = _host.adam_ascent(evaluate, x, f0, ell, box, 1.0, steps, float(lr), dt)
        return x_best, a_best, info

    def sample_functions(self, num_samples, num_features=1024, seed=0, noise=None):
        """num_samples posterior FUNCTION draws as a PathwiseDraws with z = X, M = N (pathwise conditioning on the data
        themselves, Wilson et al. 2021).  With L = num_features, omega_l ~ N(0, I_d), w_s ~ N(0, I_2L), eps_s ~ N(0, I_N):
            g_s(x) = L^-1/2 sum_l [ w_s,2l cos(omega_l . x~) + w_s,2l+1 sin(omega_l . x~) ]       (prior path, unit RBF)
            v_s = sqrt(k_var) K^^-1 (y - sqrt(k_var) g_s(X) - sqrt(noise_var) eps_s)
            f_s(x) = sqrt(k_var) ( g_s(x) + v_s K(X, x) ),
        i.e. coefficient rows [w_s / sqrt(L) | v_s] under scale = sqrt(k_var), the conventions of SparseGP.pathwise_draws.
        g_s(X) is hb_sgp_pathwise with M = 0; the v_s come from lockstep solves in blocks of 64 draws; evaluation is the
        unchanged hb_sgp_pathwise, O((N + L) n) per draw.  noise=None draws omega [L, d], w [S, 2L], eps [S, N] from
        hip_ops.Rng(seed), in that order; noise=dict(omega=, w=, eps=) injects them.  One output column (P = 1) only.  The object's
        grad, argmax and maximise (PathwiseDraws) run unchanged on it: z = X is all the kernels see."""
        sess = self._sess
        torch, H = sess.torch, sess.H
        S, L = int(num_samples), int(num_features)
        if not (S >= 1 and L >= 1):
            raise ValueError("sample_functions: num_samples >= 1 and num_features >= 1 expected (got %r, %r)"
                             % (num_samples, num_features))
        if self._Y.shape[0] != 1:
            raise NotImplementedError("sample_functions: one latent function only (Y has %d columns)" % self._Y.shape[0])
        N, d = self._X.shape
        dt = sess.torch_dtype
        omega, w, eps = _host.pathwise_noise(sess, "sample_functions", noise, seed, ((L, d), (S, 2 * L), (S, N)))
        cw = H.ewise("AFFINE", [w], params=(1.0 / np.sqrt(L), 0.0))
        sk = float(np.sqrt(self.k_var))
        prior = H.sgp_pathwise(self._X, omega, None, self._ell, cw, scale=sk)                           # [S, N]
        rhs = H.ewise("SUB", [H.ewise("SUB", [self._Y, prior]), H.ewise("AFFINE", [eps], params=(np.sqrt(self.noise_var), 0.0))])
        V = torch.empty((S, N), dtype=dt, device=sess.device)
        for a in range(0, S, 64):
            sol, _ = self._solve(rhs[a:a + 64].contiguous())
            H.ewise("AFFINE", [sol], params=(sk, 0.0), out=V[a:a + 64])
        coef = torch.cat([cw, V], dim=1).contiguous()
        return PathwiseDraws(sess, omega, coef, self._X, self._ell, sk)
