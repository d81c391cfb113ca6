"""The identity behind hb_sgp_bwd_phi (numpy float64, no GPU):

    Phisym(L^T tril(-W^T Abar A^T)) == Phisym(-Abar A^T),      W = L^-1,  Abar = u^T fbar + A diag(c)

Phisym (matutil mode 4) reads the lower triangle only, L^T is upper triangular, so the tril in between drops out, and
L^T W^T = I cancels the two triangular factors.  Phisym itself is taken from tests/graph_oracle.py (the evaluator the
CPU suite checks the traced graph with), so the mirror / half-diagonal convention the kernel must reproduce is pinned
here: Phisym(Q)_ij = Q_{max(i,j), min(i,j)} / 2, the diagonal included."""
import numpy as np

import graph_oracle as GO
from henbun_amd import graph as G


def phisym_oracle(Q):
    x = G.leaf("data", Q.shape, var=None)
    y = G.matutil(x, 4)
    return GO.evaluate([y], {x: Q})[y].numpy()


def phisym_explicit(Q):
    i, j = np.indices(Q.shape)
    return 0.5 * Q[np.maximum(i, j), np.minimum(i, j)]


def problem(M=96, n=70, P=3, diag_add=1e-3, seed=0):
    rng = np.random.RandomState(seed)
    z = np.sort(rng.uniform(0.0, 0.25 * M, (M, 1)), axis=0)
    x = rng.uniform(0.0, 0.25 * M, (n, 1))
    Kmm = np.exp(-0.5 * (z - z.T) ** 2) + diag_add * np.eye(M)
    L = np.linalg.cholesky(Kmm)
    W = np.linalg.inv(L)
    A = W @ np.exp(-0.5 * (z - x.T) ** 2)
    u, fbar, c = rng.randn(P, M), rng.randn(P, n), rng.randn(n)
    Abar = u.T @ fbar + A * c[None, :]
    return Kmm, L, W, A, Abar


def test_mode4_of_the_graph_oracle_is_half_of_the_lower_triangle_mirrored():
    Q = np.random.RandomState(1).randn(7, 7)
    got = phisym_oracle(Q)
    assert np.array_equal(got, phisym_explicit(Q))
    assert np.array_equal(got, got.T) and np.array_equal(np.diag(got), 0.5 * np.diag(Q))
    # ... and it is the symmetrised Phi of Murray's Cholesky VJP: (Phi(Q) + Phi(Q)^T) / 2
    phi = np.tril(Q, -1) + 0.5 * np.diag(np.diag(Q))
    assert np.allclose(got, 0.5 * (phi + phi.T), rtol=0, atol=1e-15)


def test_phisym_of_the_vjp_product_is_phisym_of_minus_abar_at():
    Kmm, L, W, A, Abar = problem()
    assert np.linalg.cond(Kmm) > 1e3       # the two routes differ in conditioning, not in value
    Lbar = -np.tril(W.T @ Abar @ A.T)      # what hb_sgp_bwd returns
    via_product = phisym_oracle(L.T @ np.tril(Lbar))
    direct = phisym_oracle(-Abar @ A.T)
    err = np.abs(via_product - direct).max() / np.abs(direct).max()
    assert err <= 1e-10, err
    # the tril is not what makes them equal: without it the lower triangle of the product is the same
    assert np.abs(np.tril(L.T @ Lbar) - np.tril(L.T @ (-W.T @ Abar @ A.T))).max() <= 1e-10 * np.abs(direct).max()
