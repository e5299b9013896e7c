"""gsum_amd — MI355X-native GP hot path of buqeye/gsum (kernel build, jittered Cholesky,
multivariate-normal log-likelihood) behind gsum's ConjugateGaussianProcess / ConjugateStudentProcess / TruncationGP / TruncationTP surface.

Compute runs in libgsum_hip.so (hand-written HIP for gfx950, bound with ctypes); the variogram (``VariogramFourthRoot``,
``Diagnostic.variogram``) runs in its own libgsum_vario.so, and the reference distributions of ``GraphicalDiagnostic`` (``refdist``: column
sort, percentile bands, interval coverage) in their own libgsum_refdist.so; the uncorrelated model ``TruncationPointwise`` (grid
likelihood, credible-interval coverage) has its own libgsum_pointwise.so, the leave-one-out and leave-group-out diagnostics
(``loo_from_factor``, ``kfold_from_factor``, ``Diagnostic.loo`` / ``.kfold``, ``ConjugateGaussianProcess.loo`` / ``.kfold``) their own libgsum_loo.so, the Toeplitz likelihood path for stationary kernels on uniform one-dimensional grids
(``structure="toeplitz"``, ``toeplitz_column``, ``toeplitz_gram``, ``uniform_grid_step``) its own libgsum_toep.so, the banded likelihood path for short-range kernels on sorted one-dimensional points
(``structure="banded"``, ``sorted_points``, ``banded_halfwidth``, ``banded_matrix``, ``banded_gram``, ``banded_forward``) its own libgsum_band.so, and ``hpd``, ``hpd_pdf``, ``median_pdf`` and ``cartesian`` are
the reference's host helpers.  matplotlib is imported by ``GraphicalDiagnostic``'s plot
methods when they are called, never by importing this package.  There is no CPU path except where a class takes ``backend='cpu'``.
"""
from .series import coefficients, partials, geometric_sum
from .conjugate import (ConjugateGaussianProcess, ConjugateStudentProcess, posterior_from_gram, lml_from_gram,
                        lml_from_gram_batch, student_lml_from_gram, cov_factor)
from .truncation import TruncationGP, TruncationTP
from .kernels import describe_kernel, describe_thetas
from .datasets import (make_gaussian_partial_sums, make_gaussian_partial_sums_uniform,
                       make_gaussian_partial_sums_on_grid, sample_mvn_cholesky)
from .diagnostics import Diagnostic, pivoted_cholesky
from .variogram import VariogramFourthRoot
from . import refdist
from .graphical import GraphicalDiagnostic
from .pointwise import TruncationPointwise
from .loo import FoldResult, LooResult, kfold_from_factor, loo_from_factor, make_folds
from .toeplitz import (toeplitz_column, toeplitz_grad, toeplitz_gradient_columns, toeplitz_gram, toeplitz_inverse_column, toeplitz_solve,
                       uniform_grid_step, toeplitz_predict, toeplitz_inverse_diagonal, toeplitz_loo, toeplitz_panel_width)
from .banded import banded_forward, banded_gram, banded_halfwidth, banded_matrix, banded_max_halfwidth, sorted_points
from .stats import hpd, hpd_pdf, median_pdf, cartesian
from .grid import shard_range, gather_flat, lml_grid_distributed, predict_distributed
from ._lib import HipContext, HipGroup, KernelDesc, default_context, default_group, device_count, lab_context, load_library

__version__ = "0.1.0"
__all__ = [
    "coefficients", "partials", "geometric_sum", "ConjugateGaussianProcess", "ConjugateStudentProcess",
    "TruncationGP", "TruncationTP", "posterior_from_gram", "lml_from_gram", "lml_from_gram_batch", "student_lml_from_gram", "cov_factor", "describe_kernel", "describe_thetas", "make_gaussian_partial_sums",
    "make_gaussian_partial_sums_uniform", "make_gaussian_partial_sums_on_grid", "sample_mvn_cholesky", "shard_range", "gather_flat",
    "lml_grid_distributed", "Diagnostic", "pivoted_cholesky", "VariogramFourthRoot", "GraphicalDiagnostic", "refdist",
    "TruncationPointwise", "LooResult", "loo_from_factor", "FoldResult", "kfold_from_factor", "make_folds", "toeplitz_column", "toeplitz_gram", "uniform_grid_step", "toeplitz_inverse_column", "toeplitz_solve", "toeplitz_grad",
    "toeplitz_gradient_columns", "toeplitz_predict", "toeplitz_inverse_diagonal", "toeplitz_loo", "toeplitz_panel_width", "sorted_points", "banded_halfwidth", "banded_matrix",
    "banded_gram", "banded_forward", "banded_max_halfwidth", "hpd", "hpd_pdf", "median_pdf", "cartesian", "predict_distributed", "HipContext", "HipGroup", "KernelDesc", "default_context", "default_group", "device_count", "lab_context", "load_library",
]
