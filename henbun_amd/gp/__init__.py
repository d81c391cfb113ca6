from . import kernels
from .exact import ExactPosterior, NotConverged, Preconditioner, VarianceCache, log_marginal_likelihood, pcg_solve
from .gp import GP, SparseGP
from .sparse import PathwiseDraws, SparsePosterior, greedy_inducing
