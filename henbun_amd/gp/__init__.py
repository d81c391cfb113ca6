from . import kernels
from .exact import ExactPosterior, NotConverged, Preconditioner, pcg_solve
from .gp import GP, PathwiseDraws, SparseGP, greedy_inducing
