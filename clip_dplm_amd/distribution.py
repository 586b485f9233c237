"""Distances between two embedding clouds as distributions: multi-bandwidth MMD on the fused kernel of
csrc/kernel_sums.hip, the Fréchet distance, and the three metric names of the reference's evaluation config.

The reference's config asks for `metrics: ['wasserstein', 'mmd', 'fid']` (tong/configs/default.yaml:74) from a
utils.metrics.FlowEvaluator that tong/experiments/evaluate.py:5,24,40 imports and the reference never defines.
'wasserstein' is ot.sinkhorn_divergence; this module adds the other two and evaluate_distributions, which takes the names.

MMD with a mixture of Gaussian bandwidths, clouds x [M, P], y [N, P] (f32, device):

    k(a, b) = sum_b w_b exp(-gamma_b |a - b|^2)
    unbiased:  sum_{i != i'} k(x_i, x_i') / (M (M - 1)) + sum_{j != j'} k(y_j, y_j') / (N (N - 1)) - 2 sum_ij k(x_i, y_j) / (M N)
    biased:    the V-statistic, the diagonals included and the denominators M^2, N^2

Each of the three blocks is one ops.kernel_sums call (include/clipk.h: clipk_kernel_sums): one tile walk for all B
bandwidths, the M x N matrix never written, the diagonal of a self block dropped as a term.  The backward pass is the
same entry with the weights w_b gamma_b and the key-weighted sums: with K' that mixture, g_i = sum_j K'_ij and
m_i = sum_j K'_ij y_j,  d/dx_i sum_j k(x_i, y_j) = -2 (g_i x_i - m_i);  a self block enters twice by symmetry.  What is
left to ATen is O((M + N) P) glue: squared norms, the closed-form mean cost, the sums over rows.
"""
from __future__ import annotations

import math

import torch

from . import ops, ot

__all__ = ["mmd2", "frechet_distance", "evaluate_distributions"]

DEFAULT_MULTIPLIERS = (0.25, 0.5, 1.0, 2.0, 4.0)


def _vector_arg(name, v):
    """Length of a bandwidth / weight argument (a sequence of numbers or a 1-D tensor), with its own errors."""
    if isinstance(v, torch.Tensor):
        if v.dim() != 1:
            raise ValueError(f"{name} must be 1-D, got shape {tuple(v.shape)}")
        if not v.is_floating_point():
            raise TypeError(f"{name} must be a floating-point tensor, got {v.dtype}")
        return v.shape[0]
    try:
        vals = [float(t) for t in v]
    except TypeError:
        raise TypeError(f"{name} must be a sequence of numbers or a 1-D tensor") from None
    if not all(math.isfinite(t) for t in vals):
        raise ValueError(f"{name} must be finite, got {vals}")
    return len(vals)


def _check_args(x, y, gammas, multipliers, weights, unbiased):
    """Every argument error of mmd2(), raised before anything is launched.  Returns B."""
    for name, t in (("x", x), ("y", y)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
        if t.dim() != 2 or t.shape[0] == 0:
            raise ValueError(f"{name} must be a non-empty 2-D tensor, got shape {tuple(t.shape)}")
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"x has {x.shape[1]} columns, y {y.shape[1]}")
    P = x.shape[1]
    if P == 0 or P % 4 or P > ops.KERNEL_SUMS_MAX_P:
        raise ValueError(f"the width must be a multiple of 4 and at most {ops.KERNEL_SUMS_MAX_P}, got {P}")
    bands = ("multipliers", multipliers) if gammas is None else ("gammas", gammas)
    B = _vector_arg(*bands)
    if not 1 <= B <= ops.KERNEL_SUMS_MAX_B:
        raise ValueError(f"{bands[0]} must have 1 to {ops.KERNEL_SUMS_MAX_B} entries, got {B}")
    if not isinstance(bands[1], torch.Tensor) and not all(float(t) > 0 for t in bands[1]):
        raise ValueError(f"{bands[0]} must be positive, got {list(bands[1])}")
    if weights is not None and _vector_arg("weights", weights) != B:
        raise ValueError(f"weights must have one entry per bandwidth ({B})")
    if unbiased and (x.shape[0] < 2 or y.shape[0] < 2):
        raise ValueError(f"the unbiased estimator needs at least 2 rows per cloud, got {x.shape[0]} and {y.shape[0]}")
    if not x.is_cuda or not y.is_cuda:
        raise ValueError("mmd2 needs device tensors (there is no CPU fallback)")
    return B


def _device_vector(v, dev):
    if isinstance(v, torch.Tensor):
        return v.detach().to(device=dev, dtype=torch.float32).contiguous()
    return torch.tensor([float(t) for t in v], dtype=torch.float32, device=dev)


def _row_sums(x, y, gammas, weights, nx, ny, diag_offset):
    """sum_ij K_ij of one block in f64 (0-d): the kernel's f32 row sums, added up in f64."""
    ksum, _ = ops.kernel_sums(x, y, gammas, weights, nx, ny, diag_offset=diag_offset)
    return ksum.sum(dtype=torch.float64)


def _row_gradient(x, y, gw, weights_g, nx, ny, diag_offset):
    """d/dx_i sum_j K_ij = -2 (g_i x_i - m_i) with the weights w_b gamma_b."""
    g, m = ops.kernel_sums(x, y, gw, weights_g, nx, ny, diag_offset=diag_offset, want_bary=True)
    return -2.0 * (g[:, None] * x - m)


class _MMD2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, gammas, weights, unbiased, same):
        xd = x.detach().contiguous()
        yd = xd if same else y.detach().contiguous()             # a cloud with itself: one set of norms, two launches
        M, N = xd.shape[0], yd.shape[0]
        nx = (xd * xd).sum(1)
        ny = nx if yd is xd else (yd * yd).sum(1)
        diag = 0 if unbiased else -1
        cxx = M * (M - 1) if unbiased else M * M
        cyy = N * (N - 1) if unbiased else N * N
        sxx = _row_sums(xd, xd, gammas, weights, nx, nx, diag)
        syy = sxx if yd is xd else _row_sums(yd, yd, gammas, weights, ny, ny, diag)
        sxy = _row_sums(xd, yd, gammas, weights, nx, ny, -1)
        ctx.save_for_backward(xd, yd, gammas, weights, nx, ny)
        ctx.norm = (cxx, cyy, M * N)
        # the three terms are of the size of the kernel, their combination can be orders smaller: combined in f64
        return (sxx / cxx + syy / cyy - 2.0 * sxy / (M * N)).float()

    @staticmethod
    @torch.no_grad()
    def backward(ctx, grad):
        xd, yd, gammas, weights, nx, ny = ctx.saved_tensors
        cxx, cyy, cxy = ctx.norm
        wg = weights * gammas
        gx = gy = None
        # a self block depends on its cloud through both arguments (factor 2); its diagonal has no gradient and is
        # skipped under either estimator
        if ctx.needs_input_grad[0]:
            gx = (_row_gradient(xd, xd, gammas, wg, nx, nx, 0) * (2.0 / cxx)
                  - _row_gradient(xd, yd, gammas, wg, nx, ny, -1) * (2.0 / cxy)) * grad
        if ctx.needs_input_grad[1]:
            gy = (_row_gradient(yd, yd, gammas, wg, ny, ny, 0) * (2.0 / cyy)
                  - _row_gradient(yd, xd, gammas, wg, ny, nx, -1) * (2.0 / cxy)) * grad
        return gx, gy, None, None, None, None


def mmd2(x, y, gammas=None, multipliers=DEFAULT_MULTIPLIERS, weights=None, unbiased: bool = True):
    """Squared maximum mean discrepancy between the clouds x [M, P] and y [N, P] (f32, device; P % 4 == 0, P <= 512)
    under the kernel sum_b weights[b] exp(-gammas[b] |a - b|^2), as a differentiable 0-d tensor.

    gammas: B <= 8 positive bandwidths, a sequence of numbers or a tensor (a device tensor is read by the kernel: nothing
    is read back, so the call can be captured in a graph).  None: gammas[b] = 1 / (multipliers[b] * ot.mean_cost(x, y)),
    from the closed form on the detached clouds, on the device.  weights: B mixture weights, 1 / B each by default.
    unbiased=True: the U-statistic, the pairs of a point with itself left out (M, N >= 2); False: the V-statistic, which
    is never negative and 0 for equal clouds.  Gradients flow to x and y only: the bandwidths are constants, also when
    they are derived from the clouds."""
    B = _check_args(x, y, gammas, multipliers, weights, unbiased)
    dev = x.device
    if gammas is None:
        mult = _device_vector(multipliers, dev)
        gammas_t = 1.0 / (mult * ot.mean_cost(x.detach(), y.detach()))
    else:
        gammas_t = _device_vector(gammas, dev)
    weights_t = torch.full((B,), 1.0 / B, dtype=torch.float32, device=dev) if weights is None else _device_vector(weights, dev)
    return _MMD2Fn.apply(x, y, gammas_t, weights_t, bool(unbiased), y is x)


def _sqrt_psd(c):
    """Symmetric square root of a positive semi-definite matrix (negative eigenvalues of rounding clipped to 0)."""
    lam, vec = torch.linalg.eigh(c)
    return (vec * lam.clamp_min(0).sqrt()) @ vec.T


@torch.no_grad()
def frechet_distance(x, y) -> float:
    """|mu_x - mu_y|^2 + tr(C_x + C_y - 2 (C_x C_y)^(1/2)) between the Gaussians fitted to the clouds x [M, P], y [N, P]
    (any float dtype, device or host; the FID formula), as a Python float.  Covariances with denominator n - 1; means
    and covariances are accumulated in f64 on the inputs' device, the two P x P eigen-decompositions run in f64 on the
    host:  tr (C_x C_y)^(1/2) = sum_k sqrt(max(lambda_k, 0)) over the eigenvalues of C_x^(1/2) C_y C_x^(1/2).  Not
    differentiable."""
    for name, t in (("x", x), ("y", y)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise TypeError(f"{name} must be a floating-point tensor")
        if t.dim() != 2 or t.shape[0] < 2 or t.shape[1] == 0:
            raise ValueError(f"{name} must be 2-D with at least 2 rows, got shape {tuple(t.shape)}")
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"x has {x.shape[1]} columns, y {y.shape[1]}")

    def moments(t):
        t = t.detach().double()
        mu = t.mean(0)
        c = t - mu
        return mu.cpu(), ((c.T @ c) / (t.shape[0] - 1)).cpu()

    (mx, cx), (my, cy) = moments(x), moments(y)
    rx = _sqrt_psd(cx)
    inner = rx @ cy @ rx
    lam = torch.linalg.eigvalsh(0.5 * (inner + inner.T))
    cross = lam.clamp_min(0).sqrt().sum()
    d = mx - my
    return float(d @ d + torch.trace(cx) + torch.trace(cy) - 2.0 * cross)


_MMD_KW = ("gammas", "multipliers", "weights", "unbiased")
_SINKHORN_KW = ("eps", "eps_rel", "a", "b", "n_iters", "tol", "check_every")


@torch.no_grad()
def evaluate_distributions(x, y, metrics=("wasserstein", "mmd", "fid"), **kw) -> dict:
    """The reference's three distribution metrics (tong/configs/default.yaml:74) between the clouds x and y, a dict of
    Python floats by name: 'wasserstein' = ot.sinkhorn_divergence, 'mmd' = mmd2, 'fid' = frechet_distance.  Keyword
    arguments go to the call that takes them: gammas / multipliers / weights / unbiased to mmd2, eps / eps_rel / a / b /
    n_iters / tol / check_every to the Sinkhorn divergence."""
    calls = {
        "wasserstein": lambda: ot.sinkhorn_divergence(x, y, **{k: v for k, v in kw.items() if k in _SINKHORN_KW}),
        "mmd": lambda: mmd2(x, y, **{k: v for k, v in kw.items() if k in _MMD_KW}),
        "fid": lambda: frechet_distance(x, y),
    }
    metrics = list(metrics)
    for name in metrics:
        if name not in calls:
            raise ValueError(f"unknown metric {name!r}: the names are {sorted(calls)}")
    for k in kw:
        if k not in _MMD_KW + _SINKHORN_KW:
            raise TypeError(f"unexpected keyword argument {k!r}")
    return {name: float(calls[name]()) for name in metrics}
