"""Conditional flow matching along a Schrodinger bridge: what the reference's SchrodingerBridgeFlow
(tong/models/flows/ot_flow.py:87-99) asks of a third-party library that works on the materialised squared-distance
matrix, `SchrodingerBridgeConditionalFlowMatcher(sigma, ot_method="sinkhorn", reg=2 sigma^2)`, on ot.py's solver.

One training batch: solve the entropic plan between the source batch x0 and the target batch x1 (ot.sinkhorn,
eps = reg), draw index pairs (i, j) ~ P (SinkhornResult.sample_pairs: one ops.sim_sample launch, the M x N matrix is
never written), re-pair the rows and build the bridge's location and conditional target field:

    mu = t x1 + (1 - t) x0,   xt = mu + sigma sqrt(t (1 - t)) noise,   ut = (1 - 2 t) / (2 t (1 - t) + 1e-8) (xt - mu) + x1 - x0

flow_matching_loss (tong/utils/losses.py:30-32) trains a field against ut.  The arithmetic on [n, P] is plain torch on
any device - it is not a hot path; the solve and the draw need the device.  The reference's OTFlow network, which feeds
ut into its own input, is not part of this module.

The reference's other coupling, flow_type == 'exact_ot' (ExactOTFlow, ot_flow.py:58-68, on the library's
ExactOptimalTransportConditionalFlowMatcher), re-pairs the batches with the optimal permutation and moves along straight
lines: ExactOptimalTransportConditionalFlowMatcher below, on ot.exact_assignment, with

    xt = t x1 + (1 - t) x0 + sigma noise,   ut = x1 - x0                                      (linear_conditional_flow)

The library is not a dependency: these formulae are what this module commits to.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import ops, ot

__all__ = ["conditional_flow", "SchrodingerBridgeConditionalFlowMatcher", "flow_matching_loss", "linear_conditional_flow",
           "ExactOptimalTransportConditionalFlowMatcher"]


def _flow_args(x0, x1, t, noise):
    for name, v in (("x0", x0), ("x1", x1), ("noise", noise)):
        if not isinstance(v, torch.Tensor):
            raise TypeError(f"{name} must be a tensor")
    if x0.shape != x1.shape or noise.shape != x0.shape:
        raise ValueError(f"x0, x1 and noise must have one shape, got {tuple(x0.shape)}, {tuple(x1.shape)}, {tuple(noise.shape)}")
    t = torch.as_tensor(t, dtype=x0.dtype, device=x0.device)
    if t.dim() > 1 or (t.dim() == 1 and t.shape[0] != x0.shape[0]):
        raise ValueError(f"t must be a scalar or have one entry per row, got shape {tuple(t.shape)}")
    return t.reshape(-1, *([1] * (x0.dim() - 1))) if t.dim() == 1 else t


def conditional_flow(x0, x1, t, noise, sigma):
    """(xt, ut) of the bridge between the paired rows x0, x1 [n, P] at times t [n] (or a 0-d tensor / number) under the
    standard-normal `noise` [n, P]; the formulae are in the module's docstring."""
    t = _flow_args(x0, x1, t, noise)
    mu = t * x1 + (1.0 - t) * x0
    xt = mu + sigma * torch.sqrt(t * (1.0 - t)) * noise
    ut = (1.0 - 2.0 * t) / (2.0 * t * (1.0 - t) + 1e-8) * (xt - mu) + x1 - x0
    return xt, ut


def linear_conditional_flow(x0, x1, t, noise, sigma):
    """(xt, ut) of the straight path between the paired rows x0, x1 [n, P] at times t [n] (or a 0-d tensor / number):
    xt = t x1 + (1 - t) x0 + sigma noise, ut = x1 - x0."""
    t = _flow_args(x0, x1, t, noise)
    return t * x1 + (1.0 - t) * x0 + sigma * noise, x1 - x0


def flow_matching_loss(v, target_v):
    """Mean squared error between the predicted and the target field (tong/utils/losses.py:30-32)."""
    return torch.nn.functional.mse_loss(v, target_v)


class SchrodingerBridgeConditionalFlowMatcher:
    """sigma: the bridge's noise scale.  reg: the entropic regularisation handed to ot.sinkhorn as eps, None = 2 sigma^2
    (the reference's setting).  n_iters, tol: the solver's; tol=None runs exactly n_iters iterations and reads nothing
    back from the device.  precision: ot.sinkhorn's ("f32" or "bf16x3"; the draws always use the exact f32 kernel)."""

    def __init__(self, sigma: float, reg: Optional[float] = None, n_iters: int = 50, tol: Optional[float] = None,
                 precision: str = "f32"):
        sigma = float(sigma)
        if not (sigma > 0 and math.isfinite(sigma)):
            raise ValueError(f"sigma must be positive and finite, got {sigma}")
        reg = 2.0 * sigma * sigma if reg is None else float(reg)
        if not (reg > 0 and math.isfinite(reg)):
            raise ValueError(f"reg must be positive and finite, got {reg}")
        if int(n_iters) < 1:
            raise ValueError("n_iters must be at least 1")
        if tol is not None and not float(tol) > 0:
            raise ValueError(f"tol must be positive or None, got {tol}")
        if precision not in ot.PRECISIONS:
            raise ValueError(f"precision must be one of {ot.PRECISIONS}, got {precision!r}")
        self.sigma, self.reg, self.n_iters, self.tol, self.precision = sigma, reg, int(n_iters), tol, precision

    @torch.no_grad()
    def sample_location_and_conditional_flow(self, x0, x1, t=None, return_noise=False, return_indices=False, seed=0,
                                             generator=None):
        """(t, xt, ut[, noise][, (i, j)]) for the batches x0 [M, P], x1 [N, P] (f32, device): n = M pairs (i, j) drawn from
        the entropic plan between them, xt and ut = conditional_flow(x0[i], x1[j], t, noise, sigma).  t [M]: given, or
        uniform on [0, 1) under `generator`, which also drives the noise and the choice of i; `seed` (an int, or an int64
        device tensor {seed, stream_offset}) drives the choice of j.  With tol=None and a seed tensor nothing is read back."""
        if isinstance(x0, torch.Tensor) and isinstance(t, torch.Tensor) and t.shape != (x0.shape[0],):
            raise ValueError(f"t must have shape ({x0.shape[0]},), got {tuple(t.shape)}")
        ops._seed_offset(seed, 0)
        r = ot.sinkhorn(x0, x1, eps=self.reg, n_iters=self.n_iters, tol=self.tol, precision=self.precision)
        n = x0.shape[0]
        i, j = r.sample_pairs(n, seed=seed, generator=generator)
        a, b = r._x.index_select(0, i), r._y.index_select(0, j)
        if t is None:
            t = torch.rand(n, dtype=a.dtype, device=a.device, generator=generator)
        noise = torch.randn(a.shape, dtype=a.dtype, device=a.device, generator=generator)
        xt, ut = conditional_flow(a, b, t, noise, self.sigma)
        out = [t, xt, ut]
        if return_noise:
            out.append(noise)
        if return_indices:
            out.append((i, j))
        return tuple(out)


class ExactOptimalTransportConditionalFlowMatcher:
    """The reference's 'exact_ot' coupling: batches re-paired by the optimal permutation between them
    (ot.exact_assignment; solver_kw are its keyword arguments), straight conditional paths with noise scale sigma
    (0 by default).  replace=True draws the n = N rows i uniformly with replacement under `generator`, as a draw from the
    plan does; replace=False takes every row once, in order."""

    def __init__(self, sigma: float = 0.0, replace: bool = True, **solver_kw):
        sigma = float(sigma)
        if not (sigma >= 0 and math.isfinite(sigma)):
            raise ValueError(f"sigma must be non-negative and finite, got {sigma}")
        unknown = set(solver_kw) - {"eps", "eps_rel", "eps_start_rel", "theta", "check_every", "max_rounds"}
        if unknown:
            raise TypeError(f"unknown solver arguments: {sorted(unknown)}")
        self.sigma, self.replace, self.solver_kw = sigma, bool(replace), dict(solver_kw)

    @torch.no_grad()
    def sample_location_and_conditional_flow(self, x0, x1, t=None, return_noise=False, return_indices=False, generator=None):
        """(t, xt, ut[, noise][, (i, j)]) for the batches x0, x1 [N, P] (f32, device): j = perm[i] under the optimal
        matching, xt and ut = linear_conditional_flow(x0[i], x1[j], t, noise, sigma).  t [N]: given, or uniform on [0, 1)
        under `generator`, which also drives the noise and (replace=True) the choice of i.  Raises RuntimeError when the
        solve left rows unassigned."""
        if isinstance(x0, torch.Tensor) and isinstance(t, torch.Tensor) and t.shape != (x0.shape[0],):
            raise ValueError(f"t must have shape ({x0.shape[0]},), got {tuple(t.shape)}")
        r = ot.exact_assignment(x0, x1, **self.solver_kw)
        if bool((r.perm < 0).any()):
            raise RuntimeError(f"exact_assignment did not converge ({r.reason}): no matching to pair the batches with")
        n, dev = x0.shape[0], r.perm.device
        if self.replace:
            i = torch.randint(n, (n,), dtype=torch.int64, device=dev, generator=generator)
        else:
            i = torch.arange(n, dtype=torch.int64, device=dev)
        j = r.perm.index_select(0, i)
        a, b = r._x.index_select(0, i), r._y.index_select(0, j)
        if t is None:
            t = torch.rand(n, dtype=a.dtype, device=dev, generator=generator)
        noise = torch.randn(a.shape, dtype=a.dtype, device=dev, generator=generator)
        xt, ut = linear_conditional_flow(a, b, t, noise, self.sigma)
        out = [t, xt, ut]
        if return_noise:
            out.append(noise)
        if return_indices:
            out.append((i, j))
        return tuple(out)
