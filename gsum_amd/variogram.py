R"""The empirical semivariogram with fourth-root-transform uncertainties: gsum.helpers.VariogramFourthRoot (helpers.py:525-730).

``backend='hip'`` (the default; $GSUM_BACKEND) runs the pair stage and ``cov`` / ``compute`` in libgsum_vario.so (DESIGN.md section
12): distances bit-identical to numpy's, per-bin counts exact, per-bin sums and cov sums in a fixed device order (bitwise
reproducible, not numpy's order).  ``backend='cpu'`` is the same class on numpy / scipy: its per-bin averages are the reference's
own (bit-identical), and ``cov`` is the reference's arithmetic in blocks, so that memory stays O(block) instead of O(pairs of a
bin ^ 2); only its summation order differs.

The reference's O(P) / O(N^2) attributes (P = N (N - 1) / 2 pairs) are lazy properties built on the host on first access,
bit-identical to the reference: ``inputs`` (32 P bytes), ``data`` (24 P n_curves bytes), ``bin_idx`` (8 P bytes), ``bin_mask``
(Nb P bytes: 8 GB at N = 2000 with 4000 bins) and ``gamma_tilde_grid`` (8 N^2 n_curves bytes); building ``inputs`` / ``data``
passes through the reference's full N x N arrays (N / 2 times as much).  ``rho_ijkl``, ``corr_ijkl``, ``cov_ijkl`` and ``var_ij``
are the reference's host numpy / scipy code on ``gamma_tilde_grid``.
"""
from __future__ import annotations

from math import gamma

import numpy as np
from scipy.special import hyp2f1

from ._backend import resolve_backend, resolve_device

__all__ = ["VariogramFourthRoot"]

_CHUNK = 1 << 20            # cpu backend: array elements per block


class VariogramFourthRoot:
    R"""Computes the empirical semivariogram and uncertainties via the fourth root transformation (Bowman & Crujeiras 2013,
    Cressie & Hawkins 1980), as gsum.helpers.VariogramFourthRoot.

    Parameters
    ----------
    X : array, shape = (N, n_features)
    z : array, shape = (N,) or (n_curves, N)
        The function values, one curve per row (the reference's code reads them so; its docstring says otherwise).
    bin_bounds : array, shape = (n_bins - 1,)
        Non-decreasing, finite bin boundaries; a distance h is in bin #{bounds <= h} (numpy.digitize).
    device, backend : as for the model classes ('hip' or 'cpu').

    Limits (ValueError): N <= 65535, n_features <= 64, n_bins <= 32767, finite X, finite non-decreasing bounds.
    ``close()`` frees the device object (``__del__`` does too).
    """

    mean_factor = np.sqrt(2 / np.pi) * gamma(0.75)
    var_factor = 2. / np.pi * (np.sqrt(np.pi) - gamma(0.75)**2)
    corr_factor = gamma(0.75)**2 / (np.sqrt(np.pi) - gamma(0.75)**2)

    def __init__(self, X, z, bin_bounds, device=None, backend=None):
        self._dev = None
        self.backend, self.device = resolve_backend(backend), resolve_device(device)
        X = np.asarray(X, dtype=float)
        if X.ndim != 2:
            raise ValueError("X must have shape (n_samples, n_features)")
        N, d = X.shape
        z = np.atleast_2d(np.asarray(z, dtype=float))
        if z.ndim != 2 or z.shape[-1] != N:
            raise ValueError(f"z must have shape (N,) or (n_curves, N) with N = len(X) = {N}, got {np.shape(z)}")
        bin_bounds = np.asarray(bin_bounds, dtype=float)
        if bin_bounds.ndim != 1 or bin_bounds.shape[0] < 1:
            raise ValueError("bin_bounds must be a non-empty 1-D array")
        if not (1 <= N <= 65535):
            raise ValueError(f"N must be in [1, 65535], got {N}")
        if not (1 <= d <= 64):
            raise ValueError(f"X must have 1 to 64 features, got {d}")
        if bin_bounds.shape[0] + 1 > 32767:
            raise ValueError("at most 32767 bins (32766 bounds)")
        if z.shape[0] < 1:
            raise ValueError("z holds no curve")
        if not np.all(np.isfinite(X)):
            raise ValueError("X must be finite")
        if not np.all(np.isfinite(bin_bounds)):
            raise ValueError("bin_bounds must be finite")
        if np.any(np.diff(bin_bounds) < 0):
            raise ValueError("bin_bounds must be non-decreasing (numpy.digitize's decreasing order is not supported)")
        self._X, self._z, self._bounds = X, z, bin_bounds
        self._lazy = {}
        Ncurves = z.shape[0]
        Nb = len(bin_bounds) + 1

        if self.backend == "hip":
            from ._vario_lib import DeviceVariogram
            self._dev = DeviceVariogram(self.device, X, z, bin_bounds)
            counts = self._dev.counts
            full = counts > 0
            mean_h, mean_dij = np.zeros(Nb), np.zeros((Nb, Ncurves))
            mean_h[full] = self._dev.h_sum[full] / counts[full]
            mean_dij[full] = self._dev.dij_sum[full] / counts[full][:, None]
        else:
            counts, mean_h, mean_dij = self._cpu_pair_stage()

        bin_labels = np.arange(Nb)
        gamma_star_hat = np.full((Nb, Ncurves), np.nan)
        # midpoints of the bounds; the overflow bins' moved one bin length out (helpers.py:584-588)
        bin_locations = np.zeros(Nb)
        bin_locations[1:-1] = (bin_bounds[1:] + bin_bounds[:-1]) / 2
        bin_locations[0] = 2 * bin_bounds[0] - bin_locations[1]
        bin_locations[-1] = 2 * bin_bounds[-1] - bin_locations[-2]
        full = counts > 0                                   # non-empty bins: the in-bin averages
        bin_locations[full] = mean_h[full]
        gamma_star_hat[full] = mean_dij[full]
        gamma_tilde = self.variogram_scale(gamma_star_hat)
        gamma_star_mean = self.mean_factor * gamma_star_hat

        self.N = N
        self.Nb = Nb
        self.Ncurves = Ncurves
        self.bin_labels = bin_labels
        self.bin_counts = counts
        self.bin_locations = bin_locations
        self.gamma_star_hat = gamma_star_hat
        self.gamma_star_mean = gamma_star_mean
        self.gamma_tilde = gamma_tilde

    # ---- device object ---------------------------------------------------------------------------------------------------------
    def close(self):
        if self._dev is not None:
            self._dev.free()
            self._dev = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- cpu backend -----------------------------------------------------------------------------------------------------------
    def _cpu_grid(self):
        """(N x N bins, h and bin of each tril pair, tril rows, tril columns), built in row blocks with the reference's
        expressions (the same bits as its full N x N arrays)."""
        if "_grid" not in self._lazy:
            X, N = self._X, self._X.shape[0]
            grid = np.empty((N, N), dtype=np.int16)
            ti, tj = np.tril_indices(N, -1)
            h_tril = np.empty(len(ti))
            rows = max(1, _CHUNK // max(1, N * X.shape[1]))
            for a in range(0, N, rows):
                h = np.linalg.norm(X[a:a + rows, None, :] - X, axis=-1)
                grid[a:a + rows] = np.digitize(h, self._bounds)
                sel = (ti >= a) & (ti < a + rows)
                h_tril[sel] = h[ti[sel] - a, tj[sel]]
            self._lazy["_grid"] = (grid, h_tril, grid[ti, tj].astype(np.intp), ti, tj)
        return self._lazy["_grid"]

    def _cpu_pair_stage(self):
        """Counts and the reference's per-bin averages (np.average of the bin's values in tril order: the same bits)."""
        zT = self._z.T
        Nb = len(self._bounds) + 1
        _, h_tril, bins, ti, tj = self._cpu_grid()
        counts = np.bincount(bins, minlength=Nb).astype(np.int64)
        order = np.argsort(bins, kind="stable")
        starts = np.concatenate([[0], np.cumsum(counts)])
        mean_h, mean_dij = np.zeros(Nb), np.zeros((Nb, zT.shape[1]))
        for b in np.flatnonzero(counts):
            p = order[starts[b]:starts[b + 1]]
            mean_h[b] = np.average(h_tril[p], axis=0)
            mean_dij[b] = np.average(np.sqrt(np.abs(zT[ti[p]] - zT[tj[p]])), axis=0)
        return counts, mean_h, mean_dij

    def _cpu_cov_sum(self, b1, b2):
        """The reference's cov_ijkl summed over the pairs of b1 x b2, in blocks of rows of the Cartesian product."""
        grid, _, bins, ti, tj = self._cpu_grid()
        gt = self.gamma_tilde
        p = np.flatnonzero(bins == b1)
        q = p if b2 == b1 else np.flatnonzero(bins == b2)
        i_all, j_all, k, ell = ti[p], tj[p], ti[q], tj[q]
        var1 = self.var_factor * np.sqrt(gt[b1])
        var2 = self.var_factor * np.sqrt(gt[b2])
        total = 0.
        rows = max(1, _CHUNK // max(1, len(q) * self.Ncurves))
        for s in range(0, len(p), rows):
            i, j = i_all[s:s + rows, None], j_all[s:s + rows, None]
            gam_jk, gam_il, gam_ik, gam_jl = gt[grid[j, k]], gt[grid[i, ell]], gt[grid[i, k]], gt[grid[j, ell]]
            rho = (gam_jk + gam_il - gam_ik - gam_jl) / (2 * np.sqrt(gt[b1] * gt[b2]))
            corr = (1 - rho**2) * hyp2f1(0.75, 0.75, 0.5, rho**2) - 1
            corr *= self.corr_factor
            corr[rho >= 1.] = 1.
            corr[rho <= -1.] = -1.
            corr = np.where(((i == k) & (j == ell))[..., None], 1., corr)
            total += np.sum(corr * np.sqrt(var1 * var2), axis=(0, 1))
        return total

    # ---- lazy reference attributes ---------------------------------------------------------------------------------------------
    def _host_full(self):
        if "inputs" not in self._lazy:
            X, z, N = self._X, self._z, self._X.shape[0]
            hij = np.linalg.norm(X[:, None, :] - X, axis=-1)
            bin_grid = np.digitize(hij, self._bounds)
            inputs = np.recarray((N, N), dtype=[('hij', float), ('bin_idxs', int), ('i', int), ('j', int)])
            inputs.hij = hij
            inputs.i = np.arange(N)[:, None]
            inputs.j = np.arange(N)
            inputs.bin_idxs = bin_grid
            data = np.recarray((N, N, z.shape[0]), dtype=[('dij', float), ('zi', float), ('zj', float)])
            data.zi = zi = z.T[:, None, :]
            data.zj = zj = z.T[None, :, :]
            data.dij = np.sqrt(np.abs(zi - zj))
            tri_idx = np.tril_indices(N, -1)
            self._lazy["inputs"] = inputs[tri_idx]
            self._lazy["data"] = data[tri_idx]
            self._lazy["bin_grid"] = bin_grid
        return self._lazy

    @property
    def inputs(self):
        return self._host_full()["inputs"]

    @property
    def data(self):
        return self._host_full()["data"]

    @property
    def bin_idx(self):
        if "bin_idx" not in self._lazy:
            self._lazy["bin_idx"] = np.digitize(self.inputs.hij, self._bounds)
        return self._lazy["bin_idx"]

    @property
    def bin_mask(self):
        if "bin_mask" not in self._lazy:
            self._lazy["bin_mask"] = self.bin_labels[:, None] == self.bin_idx
        return self._lazy["bin_mask"]

    @property
    def gamma_tilde_grid(self):
        if "gamma_tilde_grid" not in self._lazy:
            self._lazy["gamma_tilde_grid"] = self.gamma_tilde[self._host_full()["bin_grid"]]
        return self._lazy["gamma_tilde_grid"]

    # ---- the reference's host methods ------------------------------------------------------------------------------------------
    def rho_ijkl(self, i, j, k, l):  # noqa: E741
        R"""The correlation between :math:`(Z_i - Z_j)` and :math:`(Z_k - Z_l)`, estimated by gamma tilde"""
        gam = self.gamma_tilde_grid
        gam_jk = gam[j, k]
        gam_il = gam[i, l]
        gam_ik = gam[i, k]
        gam_jl = gam[j, l]
        gam_ij = gam[i, j]
        gam_kl = gam[k, l]
        rho = (gam_jk + gam_il - gam_ik - gam_jl) / (2 * np.sqrt(gam_ij * gam_kl))
        return rho

    def corr_ijkl(self, i, j, k, l):  # noqa: E741
        R"""The correlation between sqrt|Z_i - Z_j| and sqrt|Z_k - Z_l|, set to +/-1 where rho leaves (-1, 1)."""
        rho = self.rho_ijkl(i, j, k, l)
        corr = (1 - rho**2) * hyp2f1(0.75, 0.75, 0.5, rho**2) - 1
        corr *= self.corr_factor
        corr[rho >= 1.] = 1.
        corr[rho <= -1.] = -1.
        return corr

    def cov_ijkl(self, i, j, k, l):  # noqa: E741
        R"""The covariance between sqrt|Z_i - Z_j| and sqrt|Z_k - Z_l|; the correlation is 1 when (i, j) == (k, l)."""
        i, j, k, l = np.atleast_1d(i, j, k, l)  # noqa: E741
        if not (i.shape == j.shape == k.shape == l.shape):
            raise ValueError(i.shape == j.shape == k.shape == l.shape, 'i, j, k, l must have the same shape')
        n = i.shape[0], self.Ncurves
        corr = np.where((i == k) & (j == l), np.ones(n).T, self.corr_ijkl(i, j, k, l).T).T
        return corr * np.sqrt(self.var_ij(i, j) * self.var_ij(k, l))

    def var_ij(self, i, j):
        R"""The variance of sqrt(|Z_i - Z_j|), estimated by gamma tilde"""
        return self.var_factor * np.sqrt(self.gamma_tilde_grid[i, j])

    # ---- cov / compute ---------------------------------------------------------------------------------------------------------
    def _bin(self, b):
        b = int(b)
        if not -self.Nb <= b < self.Nb:
            raise IndexError(f"bin {b} is out of bounds for {self.Nb} bins")
        return b % self.Nb

    def _cov_sums(self, b1, b2):
        """Undivided sums of cov_ijkl for the bin pairs b1[r] x b2[r], shape (len(b1), n_curves); 0 for an empty bin."""
        if self.backend == "hip":
            if self._dev is None:
                raise ValueError("VariogramFourthRoot is closed")
            return self._dev.cov_sums(self.gamma_tilde, self.var_factor, self.corr_factor, b1, b2)
        out = np.zeros((len(b1), self.Ncurves))
        for r, (x, y) in enumerate(zip(b1, b2)):
            if self.bin_counts[x] * self.bin_counts[y]:
                out[r] = self._cpu_cov_sum(x, y)
        return out

    def cov(self, bin1, bin2=None):
        R"""The covariance of the binned means of sqrt|Z_i - Z_j| of two bins, shape (n_curves,); 0. when either bin is empty."""
        b1 = self._bin(bin1)
        b2 = b1 if bin2 is None else self._bin(bin2)
        nb1, nb2 = self.bin_counts[b1], self.bin_counts[b2]
        if (nb1 * nb2) == 0:
            return 0.
        cov = 0.
        cov += self._cov_sums(np.array([b1]), np.array([b2]))[0]
        cov /= nb1 * nb2
        return cov

    def variogram_scale(self, x):
        return (x / self.mean_factor) ** 4

    def fourth_root_scale(self, x):
        return self.mean_factor * x ** 0.25

    def compute(self, rt_scale=False):
        R"""The mean semivariogram and approximate 68% bands (gamma, lower, upper), each (Nb, n_curves), on the variogram scale
        (default) or the fourth-root scale (``rt_scale=True``).  The covariances of all bins are one device call."""
        gam = self.gamma_star_mean if rt_scale else self.gamma_tilde
        labels = self.bin_labels.astype(np.int32)
        sums = self._cov_sums(labels, labels)
        counts = self.bin_counts
        cov = np.zeros((self.Nb, self.Ncurves))
        full = counts > 0
        cov[full] = sums[full] / (counts[full] * counts[full])[:, None]
        sd = np.sqrt(cov)
        lower = self.gamma_star_mean - sd
        upper = self.gamma_star_mean + sd
        if not rt_scale:
            lower = self.variogram_scale(lower)
            upper = self.variogram_scale(upper)
        return gam, lower, upper
