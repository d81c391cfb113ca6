from . import kernels
from .gp import GP, PathwiseDraws, SparseGP, greedy_inducing
