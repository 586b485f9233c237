"""Restatement of clip_dplm_amd.distribution and of ops.kernel_sums in plain torch, the M x N matrix materialised.

    d2_ij = |x_i - y_j|^2,  K_ij = sum_b w_b exp(-gamma_b d2_ij),  ksum_i = sum_j K_ij,  kbary_i = sum_j K_ij y_j
    diag_offset d >= 0: row i leaves out key i + d (where that key exists)
    MMD^2 unbiased: sum_{i != i'} K(x_i, x_i') / (M (M - 1)) + sum_{j != j'} K(y_j, y_j') / (N (N - 1)) - 2 sum K(x_i, y_j) / (M N)
    MMD^2 biased:   the same sums with their diagonals and the denominators M^2, N^2
    Frechet:        |mu_x - mu_y|^2 + tr(C_x + C_y - 2 (C_x C_y)^(1/2)),  covariances over n - 1

It runs where its inputs are: on the CPU, except that the GPU tests hand it device tensors for their largest shapes
(4097 keys), where torch's own f64 / f32 kernels take seconds off a case.  In float64 d2 comes from the coordinate
differences and is the reference; in float32 it comes from the norm expansion nx_i + ny_j - 2 <x_i, y_j> clamped at 0, the
form the kernel uses: the yardstick for tolerances (what plain f32 arithmetic in another summation order makes of the
same formulae).  Everything is differentiable torch, so autograd through it checks the gradients.
"""
import math

import torch


def sq_dists(x, y):
    """[M, N] squared distances: float64 from coordinate differences (row chunks of at most 2^24 differences), other
    dtypes from the norm expansion clamped at 0."""
    if x.dtype == torch.float64:
        rows = max(1, (1 << 24) // max(1, y.shape[0] * y.shape[1]))
        return torch.cat([((x[i:i + rows, None, :] - y[None, :, :]) ** 2).sum(-1) for i in range(0, len(x), rows)])
    return ((x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2.0 * x @ y.T).clamp_min(0)


def mixture(d2, gammas, weights):
    """K = sum_b w_b exp(-gamma_b d2) in d2's dtype."""
    k = torch.zeros_like(d2)
    for g, w in zip(gammas, weights):
        k = k + float(w) * torch.exp(-torch.as_tensor(g, dtype=d2.dtype, device=d2.device) * d2)
    return k


def skip_mask(M, N, diag_offset, device=None):
    """bool [M, N]: True where row i keeps key j (False at j == i + diag_offset; all True for diag_offset < 0)."""
    keep = torch.ones(M, N, dtype=torch.bool, device=device)
    if diag_offset >= 0:
        i = torch.arange(M, device=device)
        j = i + diag_offset
        ok = j < N
        keep[i[ok], j[ok]] = False
    return keep


def kernel_sums_from(d2, y, gammas, weights, diag_offset=-1):
    """(ksum, kbary) from a given distance matrix (the GPU test computes it once per shape)."""
    k = mixture(d2, gammas, weights) * skip_mask(d2.shape[0], d2.shape[1], diag_offset, d2.device)
    return k.sum(1), k @ y


def kernel_sums(x, y, gammas, weights, diag_offset=-1):
    return kernel_sums_from(sq_dists(x, y), y, gammas, weights, diag_offset)


def mean_cost(x, y):
    """mean_ij |x_i - y_j|^2 in closed form (what ot.mean_cost computes), in the inputs' dtype."""
    return (x * x).sum(1).mean() + (y * y).sum(1).mean() - 2.0 * (x.mean(0) * y.mean(0)).sum()


def default_gammas(x, y, multipliers=(0.25, 0.5, 1.0, 2.0, 4.0)):
    c = mean_cost(x.detach(), y.detach())
    return [1.0 / (m * c) for m in multipliers]


def mmd2(x, y, gammas, weights=None, unbiased=True, dtype=torch.float64):
    """MMD^2 as a differentiable 0-d tensor in `dtype`; gammas are constants (numbers or 0-d tensors)."""
    x, y = x.to(dtype), y.to(dtype)
    B = len(gammas)
    weights = [1.0 / B] * B if weights is None else weights
    M, N = len(x), len(y)
    d = 0 if unbiased else -1
    kxx = mixture(sq_dists(x, x), gammas, weights) * skip_mask(M, M, d, x.device)
    kyy = mixture(sq_dists(y, y), gammas, weights) * skip_mask(N, N, d, x.device)
    kxy = mixture(sq_dists(x, y), gammas, weights)
    cxx, cyy = (M * (M - 1), N * (N - 1)) if unbiased else (M * M, N * N)
    return kxx.sum() / cxx + kyy.sum() / cyy - 2.0 * kxy.sum() / (M * N)


def frechet(x, y, dtype=torch.float64):
    """The Frechet distance with tr (C_x C_y)^(1/2) from the eigenvalues of the (non-symmetric) product C_x C_y itself:
    they are those of C_x^(1/2) C_y C_x^(1/2), real and >= 0 up to rounding."""
    x, y = x.detach().to(dtype).cpu(), y.detach().to(dtype).cpu()
    mx, my = x.mean(0), y.mean(0)
    cx, cy = torch.cov(x.T), torch.cov(y.T)
    lam = torch.linalg.eigvals(cx @ cy).real.clamp_min(0)
    return float(((mx - my) ** 2).sum() + torch.trace(cx) + torch.trace(cy) - 2.0 * lam.sqrt().sum())


def unit_clouds(M, N, P, seed, shift=0.3):
    """Seeded unit-norm rows in f32, the keys shifted by shift * sqrt(P) along the first axis before normalising."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, P, generator=g, dtype=torch.float64)
    y = torch.randn(N, P, generator=g, dtype=torch.float64)
    y[:, 0] += shift * math.sqrt(P)
    n = torch.nn.functional.normalize
    return n(x, dim=1).float(), n(y, dim=1).float()
