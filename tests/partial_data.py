"""The host statement of ``connectome_gnn_amd.ingest.partial_correlation`` in float64, its condition number, the
same statement carried out in float32 by the host's LAPACK, and the seeded cohorts its tests share.

Statement, per unit with a symmetric matrix ``R`` ``[n, n]`` (fp32 inputs, read from the upper triangle ``i <= j``,
everything below in fp64): ROI ``i`` is *excluded* iff ``R_ii == 0``; over the others ``C = (1 - a) R + a I`` with
``a = shrinkage``; ``P = C^-1``; ``out_ij = -P_ij / sqrt(P_ii P_jj)`` clamped to ``[-1, 1]`` for ``i != j`` and
``out_ii = 1``; the rows and columns of the excluded ROIs, diagonal included, are 0; ``absolute`` takes ``|out|``.
A unit whose ``C`` is not positive definite, or holds a NaN, is all NaN.

Cohorts: the time-series recipes of ``tests/timeseries_data.py`` passed through its ``host_corr`` and rounded to
fp32 (the diagonal is exactly 1, or 0 for a constant column), and one white-noise subject for the largest ``n``.
"""
import functools

import numpy as np
import torch

from tests import timeseries_data as TS

EPS = 2.0 ** -24                                  # the unit roundoff of fp32
KAPPA_CAP = 4096.0                                # every parity case of the device tests stays below it


def _upper(R):
    """The symmetric fp64 matrix whose upper triangle is R's."""
    R = R.double()
    up = torch.triu(R)
    return up + torch.triu(R, 1).t()


def covariance(R, shrinkage=0.0):
    """(C [n, n] fp64, kept [n] bool): the shrunk matrix with the identity on the excluded ROIs, and who is not."""
    R = _upper(R)
    n = R.shape[0]
    kept = R.diagonal() != 0
    C = (1.0 - shrinkage) * R + shrinkage * torch.eye(n, dtype=torch.float64)
    both = kept[:, None] & kept[None, :]
    C = torch.where(both, C, torch.zeros_like(C))
    C[~kept, ~kept] = 1.0
    return C, kept


def host_unit(R, shrinkage=0.0, absolute=False):
    """[n, n] float64: the statement for one unit."""
    C, kept = covariance(R, shrinkage)
    n = C.shape[0]
    if bool(torch.isnan(C).any()) or torch.linalg.cholesky_ex(C).info.item() != 0:
        return torch.full((n, n), float("nan"), dtype=torch.float64)
    P = torch.linalg.inv(C)
    d = 1.0 / torch.sqrt(P.diagonal())
    out = (-P * d[:, None] * d[None, :]).clamp(-1.0, 1.0)
    out = torch.where(kept[:, None] & kept[None, :], out, torch.zeros_like(out))
    out = torch.triu(out, 1)
    out = out + out.t() + torch.diag(kept.double())       # (symmetric to the bit, as the device's is)
    return out.abs() if absolute else out


def host_partial(R, shrinkage=0.0, absolute=False):
    """[U, n, n] float64 for R [U, n, n] (or [n, n] for one unit)."""
    if R.dim() == 2:
        return host_unit(R, shrinkage, absolute)
    return torch.stack([host_unit(r, shrinkage, absolute) for r in R])


def kappa2(C):
    """The fp64 2-norm condition number of C [n, n] over the ROIs that are not excluded (an excluded ROI is an
    isolated unit eigenvalue of ``covariance``'s C: it is left out); the largest over the units of [U, n, n]."""
    if C.dim() == 3:
        return max(kappa2(c) for c in C)
    C = C.double()
    off = C - torch.diag(C.diagonal())
    kept = ~((off == 0).all(1) & (C.diagonal() == 1))
    if not bool(kept.any()):
        return 1.0
    ev = torch.linalg.eigvalsh(C[kept][:, kept])
    return float(ev[-1] / ev[0]) if float(ev[0]) > 0 else float("inf")


def kappa_of(R, shrinkage=0.0):
    """kappa2 of the shrunk matrices of R [U, n, n]."""
    return max(kappa2(covariance(r, shrinkage)[0]) for r in R)


def host32(R, shrinkage=0.0):
    """The statement in float32 with the host's LAPACK: ``cholesky``, the triangular inverse ``M = L^-1``, ``M^T M``,
    the normalisation.  [U, n, n] float32; what an fp32 solver library gives, the yardstick of the tolerance."""
    out = []
    for r in R:
        C, kept = covariance(r, shrinkage)
        C = C.float()
        n = C.shape[0]
        L = torch.linalg.cholesky(C)
        M = torch.linalg.solve_triangular(L, torch.eye(n, dtype=torch.float32), upper=False)
        P = M.t() @ M
        d = 1.0 / torch.sqrt(P.diagonal())
        o = (-P * d[:, None] * d[None, :]).clamp(-1.0, 1.0)
        o = torch.where(kept[:, None] & kept[None, :], o, torch.zeros_like(o))
        o.fill_diagonal_(0.0)
        out.append(o + torch.diag(kept.float()))
    return torch.stack(out)


def tol(kappa, c):
    """``c kappa 2^-24 + 4 2^-24``: the error of an fp32 factorisation grows with kappa; the second term covers the
    normalisation, the clamp and the rounding of the result."""
    return c * kappa * EPS + 4.0 * EPS


def _rounded(r):
    return r.float().contiguous()                 # (host_corr's diagonal is exactly 1 or 0: it survives the rounding)


@functools.lru_cache(maxsize=None)
def cohort(S, T, n, seed=0):
    """[S, n, n] fp32 (host, shared between tests: do not modify): the correlations of ``timeseries_data.recipe``."""
    return _rounded(TS.host_corr(TS.recipe(S, T, n, seed)))


@functools.lru_cache(maxsize=None)
def planted(S, T, n, seed=0):
    """The same of ``timeseries_data.planted``: in the last unit and for n >= 5, ROIs 1 and n - 2 are excluded."""
    return _rounded(TS.host_corr(TS.planted(S, T, n, seed)))


@functools.lru_cache(maxsize=None)
def white_frames(T, n, seed=7):
    """[1, T, n] fp32: one subject of white noise."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, T, n, generator=g, dtype=torch.float64).float().contiguous()


@functools.lru_cache(maxsize=None)
def white(T, n, seed=7):
    """[1, n, n] fp32: the correlations of ``white_frames``."""
    return _rounded(TS.host_corr(white_frames(T, n, seed)))


def block_diagonal(sizes, T=300, seed=11):
    """[1, n, n] fp32, n = sum(sizes): the recipe's correlations inside each block, exact zeros across."""
    n = sum(sizes)
    R = torch.zeros(n, n, dtype=torch.float32)
    lo = 0
    for k, m in enumerate(sizes):
        R[lo:lo + m, lo:lo + m] = cohort(1, T, m, seed + k)[0]
        lo += m
    return R[None].contiguous()


def residual_partial(x):
    """[n, n] float64, the definition: the Pearson correlation of the residuals of columns i and j of x [T, n] after
    regressing both (with an intercept) on all the other columns."""
    x = x.double().numpy()
    T, n = x.shape
    out = np.eye(n)
    for i in range(n):
        for j in range(i + 1, n):
            rest = [k for k in range(n) if k not in (i, j)]
            A = np.concatenate([np.ones((T, 1)), x[:, rest]], axis=1)
            ri = x[:, i] - A @ np.linalg.lstsq(A, x[:, i], rcond=None)[0]
            rj = x[:, j] - A @ np.linalg.lstsq(A, x[:, j], rcond=None)[0]
            out[i, j] = out[j, i] = float(ri @ rj / np.sqrt((ri @ ri) * (rj @ rj)))
    return torch.from_numpy(out)
