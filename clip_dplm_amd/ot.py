"""Entropic optimal transport (Sinkhorn) between embedding clouds on the fused kernels of csrc/sinkhorn.hip.

The transport maps of icnn.py are judged by the reference with paired distances only (TransportCost's "Wasserstein-2" is
the mean of ||T(x_i) - y_i||, compute_transport_error a paired MSE); whether T pushes the source DISTRIBUTION onto the
target one is what this module measures.  The reference's second generation (tong/models/flows/ot_flow.py,
SchrodingerBridgeFlow) takes an entropic plan with reg = 2 sigma^2 from a library on the materialised squared-distance
matrix; here the M x N matrix is never written (include/clipk.h: clipk_sim_lse_bias, clipk_sinkhorn_apply).

Clouds x [M, P], y [N, P] (f32, device), weights a [M], b [N] (> 0, sum 1; uniform by default), cost C_ij = |x_i - y_j|^2:

    OT_eps = min_P <P, C> + eps KL(P | a (x) b)

With S = (2 / eps) x y^T and scaled log-potentials u, v (the squared norms are absorbed into them):

    u_i = log a_i - LSE_j(S_ij + v_j),  v_j = log b_j - LSE_i(S_ij + u_i)       start v = log b; one iteration = u, then v
    P_ij = exp(S_ij + u_i + v_j);  f_i = eps (u_i - log a_i) + |x_i|^2,  g_j = eps (v_j - log b_j) + |y_j|^2
    OT_eps = <a, f> + <b, g>;   dOT_eps / dx_i = 2 (r_i x_i - sum_j P_ij y_j),  r_i = sum_j P_ij        (envelope theorem)
    symmetric problem (y is x, a = b):  u <- (u + log a - LSE(S + u)) / 2, one potential
    S_eps(x, y) = OT_eps(x, y) - OT_eps(x, x) / 2 - OT_eps(y, y) / 2                                   (debiased divergence)

Every half-iteration is one ops.sim_lse_bias call (ops.sim_lse_bias_x3, the product as a bf16x3 split on the bf16 matrix
pipe, for all but the last iteration of a precision="bf16x3" solve); every plan-weighted sum one ops.sinkhorn_apply
call; every batch of draws from the plan (SinkhornResult.sample_targets / sample_pairs, what flow.py's matcher re-pairs its batches with) one
ops.sim_sample call.  What is left to ATen is O((M + N) P) glue: squared norms, the closed-form mean cost, the duals
from the potentials, the row gather of a draw.

The exact (non-entropic) coupling of two clouds of one size - the reference's flow_type == 'exact_ot' - is the second half
of this module: exact_assignment / wasserstein2_exact on the auction kernels of csrc/auction.hip.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional, Union

import torch

from . import ops

__all__ = ["SinkhornResult", "sinkhorn", "sinkhorn_loss", "sinkhorn_divergence", "mean_cost", "evaluate_transport",
           "AssignmentResult", "exact_assignment", "wasserstein2_exact", "eps_schedule", "PRECISIONS"]


def mean_cost(x, y, a=None, b=None):
    """sum_ij a_i b_j |x_i - y_j|^2 in closed form, sum_i a_i |x_i|^2 + sum_j b_j |y_j|^2 - 2 <sum_i a_i x_i, sum_j b_j y_j>:
    no pass over pairs.  0-d tensor on the inputs' device."""
    nx, ny = (x * x).sum(1), (y * y).sum(1)
    mx = x.mean(0) if a is None else a @ x
    my = y.mean(0) if b is None else b @ y
    sx = nx.mean() if a is None else (a * nx).sum()
    sy = ny.mean() if b is None else (b * ny).sum()
    return sx + sy - 2.0 * (mx * my).sum()


def _check_args(x, y, eps, eps_rel, a, b, n_iters, tol, check_every, symmetric):
    """Every argument error of sinkhorn(), raised before anything is launched."""
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
    if P == 0 or P % 4 or P > ops.SIM_LSE_BIAS_MAX_P:
        raise ValueError(f"the width must be a multiple of 4 and at most {ops.SIM_LSE_BIAS_MAX_P}, got {P}")
    for name, w, t in (("a", a, x), ("b", b, y)):
        if w is None:
            continue
        if not isinstance(w, torch.Tensor) or w.dtype != torch.float32:
            raise TypeError(f"{name} must be a float32 tensor")
        if w.shape != (t.shape[0],):
            raise ValueError(f"{name} must have shape ({t.shape[0]},), got {tuple(w.shape)}")
        if w.device != t.device:
            raise ValueError(f"{name} is on {w.device}, its cloud on {t.device}")
        # (a host read: skipped while a graph is being captured, where the weights were checked by the warm-up call)
        if not (w.is_cuda and torch.cuda.is_current_stream_capturing()) and not bool((w > 0).all()):
            raise ValueError(f"{name} must be positive")
    if eps is not None and not isinstance(eps, torch.Tensor) and not (float(eps) > 0 and math.isfinite(float(eps))):
        raise ValueError(f"eps must be positive and finite, got {eps}")
    if eps is None and not (float(eps_rel) > 0 and math.isfinite(float(eps_rel))):
        raise ValueError(f"eps_rel must be positive and finite, got {eps_rel}")
    if int(n_iters) < 1 or int(check_every) < 1:
        raise ValueError("n_iters and check_every must be at least 1")
    if tol is not None and not float(tol) > 0:
        raise ValueError(f"tol must be positive or None, got {tol}")
    if symmetric and (y is not x or (b is not None and b is not a)):
        raise ValueError("symmetric=True is the problem of a cloud with itself: pass y = x (the same tensor) and b = a or None")
    if not x.is_cuda or not y.is_cuda:
        raise ValueError("sinkhorn needs device tensors (there is no CPU fallback)")


@dataclass
class SinkhornResult:
    """Potentials and value of one solve.  f, g: the dual potentials; u, v: the scaled log-potentials of the plan
    P_ij = exp((2 / eps) <x_i, y_j> + u_i + v_j); eps, value (= <a, f> + <b, g>) and marginal_error (the L1 distance of the
    plan's row marginal from a; the column marginal is exact after a v update) are 0-d device tensors, so that a solve
    with tol=None does not wait for the device once its arguments are checked; n_iters: iterations run.  precision: the
    solve's ("f32" or "bf16x3"); logit_error_bound: 0-d device tensor, the eta no logit of the split iterations was further
    from the exact one than (0 for f32) - DESIGN.md has what it bounds in the result."""
    f: torch.Tensor
    g: torch.Tensor
    u: torch.Tensor
    v: torch.Tensor
    eps: torch.Tensor
    value: torch.Tensor
    n_iters: int
    marginal_error: torch.Tensor
    precision: str = "f32"
    logit_error_bound: Optional[torch.Tensor] = None
    _x: torch.Tensor = field(repr=False, default=None)
    _y: torch.Tensor = field(repr=False, default=None)
    _scale: torch.Tensor = field(repr=False, default=None)
    _nx: torch.Tensor = field(repr=False, default=None)
    _ny: torch.Tensor = field(repr=False, default=None)
    _a: Optional[torch.Tensor] = field(repr=False, default=None)     # the row weights (None = uniform), for sample_pairs

    def marginals(self):
        """(row sums [M], column sums [N]) of the plan."""
        rows, _, _ = ops.sinkhorn_apply(self._x, self._y, self._scale, self.u, self.v, want_bary=False, want_cost=False)
        cols, _, _ = ops.sinkhorn_apply(self._y, self._x, self._scale, self.v, self.u, want_bary=False, want_cost=False)
        return rows, cols

    def cost(self):
        """<P, C>, the transport cost of the plan without the entropy term (0-d tensor)."""
        _, _, c = ops.sinkhorn_apply(self._x, self._y, self._scale, self.u, self.v, self._nx, self._ny, want_mass=False,
                                     want_bary=False)
        return c.sum()

    def barycentric_map(self):
        """[M, P]: sum_j P_ij y_j / sum_j P_ij, where the plan sends x_i on average."""
        mass, bary, _ = ops.sinkhorn_apply(self._x, self._y, self._scale, self.u, self.v, want_cost=False)
        return bary / mass[:, None]

    def sample_targets(self, rows=None, seed=0):
        """int64 [n]: for each entry of `rows` one j ~ P(. | row) = softmax_j(S_row,j + v_j), by one ops.sim_sample call
        (Gumbel arg max; include/clipk.h: clipk_sim_sample has the noise).  rows: int64 index tensor on the clouds' device,
        entries in [0, M), repeats allowed; None = arange(M), which reads x in place - otherwise one row gather, O(n P)
        glue.  Draw k uses stream k of `seed`, so equal (rows, seed) give equal draws and repeated rows independent ones.
        seed: a Python int, or an int64 device tensor {seed, stream_offset} read by the kernel (no host read, capturable)."""
        ops._seed_offset(seed, 0)
        x = self._x
        if rows is not None:
            if not isinstance(rows, torch.Tensor) or rows.dtype != torch.int64 or rows.dim() != 1 or rows.numel() == 0:
                raise TypeError("rows must be a non-empty 1-D int64 index tensor")
            if rows.device != x.device:
                raise ValueError(f"rows is on {rows.device}, the clouds on {x.device}")
            # (a host read: skipped while a graph is being captured, where the rows were checked by the warm-up call)
            if not (rows.is_cuda and torch.cuda.is_current_stream_capturing()) and not bool(((rows >= 0) & (rows < x.shape[0])).all()):
                raise IndexError(f"rows must lie in [0, {x.shape[0]})")
        return self._draw(rows, seed)

    def _draw(self, rows, seed):
        x = self._x if rows is None else self._x.index_select(0, rows)
        return ops.sim_sample(x, self._y, self._scale, bias=self.v, seed=seed)

    def sample_pairs(self, n=None, seed=0, generator=None):
        """(i, j), int64 [n] each (n defaults to M): i from torch.multinomial over the row weights `a` (uniform if none
        were given) with replacement, under `generator`; j = sample_targets(i, seed).  The row marginal of the drawn
        coupling is therefore exactly `a`, and the conditionals are the plan's: this is the joint plan up to the
        result's `marginal_error`, the L1 distance between the plan's own row marginal and `a`."""
        M = self._x.shape[0]
        n = M if n is None else int(n)
        if n < 1:
            raise ValueError(f"n must be at least 1, got {n}")
        ops._seed_offset(seed, 0)
        w = self._a if self._a is not None else torch.ones(M, dtype=torch.float32, device=self._x.device)
        i = torch.multinomial(w, n, replacement=True, generator=generator)
        return i, self._draw(i, seed)                  # (in range by construction: no host read)


PRECISIONS = ("f32", "bf16x3")


def _split_planes(t):
    """(hi, lo, max row norm [1]) of a cloud: the bf16 planes ops.split_bf16 writes, once per solve."""
    pitch = ops.plane_pitch(t.shape[1])
    hi = torch.empty((t.shape[0], pitch), dtype=torch.bfloat16, device=t.device)
    lo = torch.empty_like(hi)
    norm = torch.zeros(1, dtype=torch.float32, device=t.device)
    ops.split_bf16(t, hi, lo, norm)
    return hi, lo, norm


def _logit_error_bound(P, scale, xnorm, ynorm):
    """eta of include/clipk.h (clipk_sim_lse_bias_x3) as a 0-d device tensor: no split logit scale * A_ij is further from
    scale * <x_i, y_j> than |scale| max|x| max|y| eps_rel + eps_abs, in either direction of the half-iteration."""
    from .retrieval import prefilter_eps_rel
    s = scale.abs()
    eta = s * xnorm * ynorm * prefilter_eps_rel(P, "bf16x3") + (s * P * (xnorm + ynorm + 1.0) + 1.0) * 2.0 ** -120
    return eta.reshape(())


@torch.no_grad()
def sinkhorn(x, y, eps: Union[None, float, torch.Tensor] = None, eps_rel: float = 0.05, a=None, b=None, n_iters: int = 100,
             tol: Optional[float] = 1e-5, check_every: int = 10, symmetric: bool = False,
             precision: str = "f32") -> SinkhornResult:
    """Solve OT_eps between the clouds x [M, P] and y [N, P] (f32, device; P % 4 == 0, P <= 768).

    eps: the regularisation in units of the squared distance (a number or a 0-d device tensor); None takes eps_rel x the
    mean cost, from mean_cost's closed form, on the device.  a, b: weights (> 0, summing to 1), None = uniform.
    tol=None runs exactly n_iters iterations without waiting for the device, so the call can be captured in a graph (with
    uniform weights nothing is read back at all; given weights are checked for positivity by one host read before the
    first launch, which is left out while a graph is being captured);
    with a tol the L1 marginal error (a device scalar the update kernel leaves behind) is read every check_every
    iterations and the solve stops once it is below tol.  symmetric=True (y is x, b is a or None): the averaged update with one
    potential; the alternating one leaves the two potentials of a self problem apart for hundreds of iterations.

    precision="bf16x3": the clouds are split once into bf16 hi / lo planes and the iterations run on the bf16 matrix pipe
    (ops.sim_lse_bias_x3), whose logits are within the result's `logit_error_bound` of the exact ones; the LAST
    iteration and the final error pass run on the exact f32 kernel, so the column marginal is exact and marginal_error is
    the exact plan's.  tol=None: n_iters - 1 split iterations and one exact one, no host read.  With a tol: split
    iterations (looked at every check_every) until their error is below tol or n_iters - 1 have run, then exact
    iterations, each looked at, until the exact error is below tol or n_iters is used up; n_iters counts both phases."""
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
    _check_args(x, y, eps, eps_rel, a, b, n_iters, tol, check_every, symmetric)
    x = x.detach().contiguous()
    y = x if symmetric else y.detach().contiguous()
    if symmetric:
        b = a
    dev = x.device
    M, N = x.shape[0], y.shape[0]
    nx = (x * x).sum(1)
    ny = nx if symmetric else (y * y).sum(1)
    loga = torch.full((M,), -math.log(M), dtype=torch.float32, device=dev) if a is None else a.log()
    logb = loga if symmetric else (torch.full((N,), -math.log(N), dtype=torch.float32, device=dev) if b is None else b.log())
    if eps is None:
        eps_t = float(eps_rel) * mean_cost(x, y, a, b)
    elif isinstance(eps, torch.Tensor):
        eps_t = eps.detach().to(device=dev, dtype=torch.float32).reshape(())
    else:
        eps_t = torch.full((), float(eps), dtype=torch.float32, device=dev)
    scale = (2.0 / eps_t).reshape(1)
    err = torch.zeros(1, dtype=torch.float32, device=dev)
    n_iters, check_every = int(n_iters), int(check_every)
    split = precision == "bf16x3"
    if split:
        xh, xl, xnorm = _split_planes(x)
        yh, yl, ynorm = (xh, xl, xnorm) if symmetric else _split_planes(y)
        bound = _logit_error_bound(x.shape[1], scale, xnorm, ynorm)
    else:
        bound = torch.zeros((), dtype=torch.float32, device=dev)

    def update_u(exact, **kw):                      # the half-iteration with x as the queries
        if exact:
            return ops.sim_lse_bias(x, y, scale, **kw)
        return ops.sim_lse_bias_x3(xh, xl, yh, yl, x.shape[1], scale, **kw)

    def update_v(exact, **kw):                      # ... with y as the queries
        if exact:
            return ops.sim_lse_bias(y, x, scale, **kw)
        return ops.sim_lse_bias_x3(yh, yl, xh, xl, x.shape[1], scale, **kw)

    u = loga.clone() if symmetric else torch.empty_like(loga)
    v = u if symmetric else logb.clone()

    def iteration(it, exact, look):
        """Iteration `it` (0-based); with look, whether the error of the plan it replaced is below tol (a host read)."""
        look = look and (symmetric or it > 0)       # the alternating update's first iteration has no u to compare with
        if look:
            err.zero_()
        if symmetric:
            update_u(exact, bias=u, logw=loga, prev=u, average=True, out=u, err=err if look else None)
        else:
            update_u(exact, bias=v, logw=loga, prev=u if look else None, out=u, err=err if look else None)
            update_v(exact, bias=u, logw=logb, out=v)
        return look and err.item() < tol

    done = 0
    n_split = n_iters - 1 if split else 0           # the split phase leaves at least one iteration to the exact kernel
    while done < n_split:
        done += 1
        if iteration(done - 1, False, tol is not None and done % check_every == 0):
            break
    while done < n_iters:
        done += 1
        # exact iterations of a split solve are each looked at; those of an f32 solve every check_every
        if iteration(done - 1, True, tol is not None and (split or done % check_every == 0)):
            break
    # the returned plan's own row error: one more half-iteration's worth of work, its update discarded
    err.zero_()
    ops.sim_lse_bias(x, y, scale, bias=v, logw=loga, prev=u, out=torch.empty_like(u), err=err)
    f = eps_t * (u - loga) + nx
    g = f if symmetric else eps_t * (v - logb) + ny
    va = f.mean() if a is None else (a * f).sum()
    vb = va if symmetric else (g.mean() if b is None else (b * g).sum())
    return SinkhornResult(f=f, g=g, u=u, v=v, eps=eps_t, value=va + vb, n_iters=done, marginal_error=err.reshape(()),
                          precision=precision, logit_error_bound=bound,
                          _x=x, _y=y, _scale=scale, _nx=nx, _ny=ny, _a=a)


def _row_gradient(x, y, scale, u, v):
    """dOT_eps / dx = 2 (r_i x_i - sum_j P_ij y_j) from the potentials."""
    mass, bary, _ = ops.sinkhorn_apply(x, y, scale, u, v, want_cost=False)
    return 2.0 * (mass[:, None] * x - bary)


def _check_apply_width(x):
    if x.shape[1] > ops.SINKHORN_APPLY_MAX_P:
        raise ValueError(f"gradients and plan sums need a width of at most {ops.SINKHORN_APPLY_MAX_P}, got {x.shape[1]}")


class _SinkhornLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, a, b, kw):
        if x.requires_grad or y.requires_grad:
            _check_apply_width(x)
        r = sinkhorn(x, y, a=a, b=b, **kw)
        ctx.save_for_backward(r._x, r._y, r._scale, r.u, r.v)
        return r.value.clone()

    @staticmethod
    @torch.no_grad()
    def backward(ctx, grad):
        x, y, scale, u, v = ctx.saved_tensors
        gx = _row_gradient(x, y, scale, u, v) * grad if ctx.needs_input_grad[0] else None
        gy = _row_gradient(y, x, scale, v, u) * grad if ctx.needs_input_grad[1] else None
        return gx, gy, None, None, None


class _SinkhornDivergenceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, a, b, same, kw):
        if x.requires_grad or y.requires_grad:
            _check_apply_width(x)
        if same:                                     # a cloud with itself: the three terms are one problem, S_eps = 0
            xy = xx = yy = sinkhorn(x, x, a=a, b=a, symmetric=True, **kw)
        else:
            xy = sinkhorn(x, y, a=a, b=b, **kw)
            kw = dict(kw, eps=xy.eps)                # the three terms share the cross problem's eps
            xx = sinkhorn(xy._x, xy._x, a=a, b=a, symmetric=True, **kw)
            yy = sinkhorn(xy._y, xy._y, a=b, b=b, symmetric=True, **kw)
        ctx.save_for_backward(xy._x, xy._y, xy._scale, xy.u, xy.v, xx.u, yy.u)
        return xy.value - 0.5 * xx.value - 0.5 * yy.value

    @staticmethod
    @torch.no_grad()
    def backward(ctx, grad):
        # the self terms enter with factor 1/2 and depend on their cloud through both arguments: the two halves add up to
        # one row gradient
        x, y, scale, u, v, uxx, uyy = ctx.saved_tensors
        gx = gy = None
        if ctx.needs_input_grad[0]:
            gx = (_row_gradient(x, y, scale, u, v) - _row_gradient(x, x, scale, uxx, uxx)) * grad
        if ctx.needs_input_grad[1]:
            gy = (_row_gradient(y, x, scale, v, u) - _row_gradient(y, y, scale, uyy, uyy)) * grad
        return gx, gy, None, None, None, None


def _solver_kw(eps, eps_rel, n_iters, tol, check_every, precision):
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, got {precision!r}")
    return dict(eps=eps, eps_rel=eps_rel, n_iters=n_iters, tol=tol, check_every=check_every, precision=precision)


def sinkhorn_loss(x, y, eps=None, eps_rel: float = 0.05, a=None, b=None, n_iters: int = 100, tol: Optional[float] = 1e-5,
                  check_every: int = 10, precision: str = "f32"):
    """OT_eps(x, y) as a differentiable 0-d tensor.  Gradients flow to x and y only (not to the weights, and eps - also
    when it is derived from the clouds - is a constant); they are the envelope-theorem gradients, exact at convergence:
    nothing is unrolled, so a solve stopped early gives the gradient of its current plan.  Gradients need P <= 512.
    precision: sinkhorn()'s; the plan sums of the gradient are always exact f32."""
    return _SinkhornLossFn.apply(x, y, a, b, _solver_kw(eps, eps_rel, n_iters, tol, check_every, precision))


def sinkhorn_divergence(x, y, eps=None, eps_rel: float = 0.05, a=None, b=None, n_iters: int = 100,
                        tol: Optional[float] = 1e-5, check_every: int = 10, precision: str = "f32"):
    """The debiased divergence S_eps(x, y) = OT_eps(x, y) - OT_eps(x, x) / 2 - OT_eps(y, y) / 2 as a differentiable 0-d
    tensor: zero for equal clouds, positive otherwise.  The self terms use the symmetric update and the cross term's eps.
    Gradients and precision as in sinkhorn_loss."""
    return _SinkhornDivergenceFn.apply(x, y, a, b, y is x and b is a,
                                       _solver_kw(eps, eps_rel, n_iters, tol, check_every, precision))


@torch.no_grad()
def evaluate_transport(transport, source, target, batch_size: int = 128, **sinkhorn_kwargs) -> dict:
    """Judge a transport map on held-out clouds: `mse`, the reference's paired compute_transport_error
    (triple_flow/4_transport_maps.py:284-301); `sinkhorn_divergence` between transport(source) and target, which needs no
    pairing; `identity_divergence` between source and target when their widths match - what the map has to beat."""
    from .icnn import compute_transport_error
    out = {"mse": compute_transport_error(transport, source, target, batch_size)}
    moved = torch.cat([transport(source[i:i + batch_size]) for i in range(0, len(source), batch_size)]).float().contiguous()
    tgt = target.float().contiguous()
    out["sinkhorn_divergence"] = float(sinkhorn_divergence(moved, tgt, **sinkhorn_kwargs))
    if source.shape[1] == target.shape[1]:
        out["identity_divergence"] = float(sinkhorn_divergence(source.float().contiguous(), tgt, **sinkhorn_kwargs))
    return out


# ------------------------------------------------------------------------------------------------ the exact coupling
# For two clouds of one size N with uniform weights the optimal plan of min_P <P, C> is a permutation.  The reference
# selects it with flow_type == 'exact_ot' (tong/models/flows/triple_flow.py:12-17, ot_flow.py:58-68) and takes it from a
# library that copies the squared-distance matrix to the host and runs a network-simplex solver there, once per batch.
# Here it is the auction algorithm (Bertsekas) on the device, the matrix never written: rows bid for keys on the values
#     z_ij = 2 <x_i, y_j> - |y_j|^2 - p_j = 2 <x_i, y_j> + bias_j            (-C_ij - p_j up to the row constant |x_i|^2)
# An unassigned row offers its best key the price rise gap + eps (gap = best - second-best value); the key goes to the
# largest offer.  When every row holds a key, z_{i,perm(i)} >= max_j z_ij - eps on every row (eps-complementary
# slackness), so the matching's mean cost is within eps of the optimum.  eps-scaling runs phases from a coarse eps down
# to the wanted one, keeping the prices and resetting the assignment.  One round is ops.auction_rounds' three launches;
# the host reads the unassigned count every check_every rounds.
def _check_assignment_args(x, y, eps, eps_rel, eps_start_rel, theta, check_every, max_rounds):
    """Every argument error of exact_assignment(), raised before anything is launched."""
    for name, t in (("x", x), ("y", y)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a tensor")
        if t.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {t.dtype}")
        if t.dim() != 2 or t.shape[0] == 0:
            raise ValueError(f"{name} must be a non-empty 2-D tensor, got shape {tuple(t.shape)}")
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"x has {x.shape[1]} columns, y {y.shape[1]}")
    if x.shape[0] != y.shape[0]:
        raise ValueError(f"x has {x.shape[0]} rows, y {y.shape[0]}: clouds of unequal sizes have no permutation plan "
                         "(use ot.sinkhorn for the entropic plan between them)")
    P = x.shape[1]
    if P == 0 or P % 4 or P > ops.SIM_LSE_BIAS_MAX_P:
        raise ValueError(f"the width must be a multiple of 4 and at most {ops.SIM_LSE_BIAS_MAX_P}, got {P}")
    if x.shape[0] > ops.AUCTION_MAX_N:
        raise ValueError(f"at most {ops.AUCTION_MAX_N} rows, got {x.shape[0]}")
    for name, v in (("eps", eps), ("eps_rel", eps_rel), ("eps_start_rel", eps_start_rel)):
        if name == "eps" and v is None:
            continue
        if isinstance(v, (bool, torch.Tensor)) or not (float(v) > 0 and math.isfinite(float(v))):
            raise ValueError(f"{name} must be a positive finite number, got {v!r}")
    if not (float(theta) > 1 and math.isfinite(float(theta))):
        raise ValueError(f"theta must be greater than 1, got {theta}")
    if int(check_every) < 1:
        raise ValueError("check_every must be at least 1")
    if int(max_rounds) < 1:
        raise ValueError("max_rounds must be at least 1")
    if not x.is_cuda or not y.is_cuda:
        raise ValueError("exact_assignment needs device tensors (there is no CPU fallback)")


def eps_schedule(eps_start: float, eps: float, theta: float):
    """The eps of every phase: eps_start, eps_start / theta, ... while above eps, then eps itself."""
    out, e = [], float(eps_start)
    while e > eps:
        out.append(e)
        e /= theta
    out.append(float(eps))
    return out


@dataclass
class AssignmentResult:
    """One exact_assignment() solve.  perm [N] int64 (device): row i of x is matched to row perm[i] of y (-1 on a row left
    unassigned when converged is False); cost: the mean squared distance of the matching; lower_bound, gap = cost -
    lower_bound: the dual certificate in f64 - the optimum lies in [lower_bound, cost] and the auction guarantees gap <=
    eps up to rounding (cost and gap are nan while rows are unassigned); eps: the last phase's, in units of the squared
    distance; n_rounds: rounds enqueued (each phase's count rounded up to check_every), phase_rounds: the same per phase;
    reason: 'converged', 'stalled' (an offer left an f32 price unchanged: eps is below the resolution of the prices) or
    'max_rounds'.  bias [N] f32 = -|y_j|^2 - price_j, assigned / owner [N] int32: the device state the solve ended in."""
    perm: torch.Tensor
    cost: float
    lower_bound: float
    gap: float
    eps: float
    n_rounds: int
    n_phases: int
    converged: bool
    reason: str
    phase_rounds: tuple
    bias: torch.Tensor
    assigned: torch.Tensor
    owner: torch.Tensor
    _best: torch.Tensor = field(repr=False, default=None)
    _x: torch.Tensor = field(repr=False, default=None)
    _y: torch.Tensor = field(repr=False, default=None)

    def duals(self):
        """(f [N], g [N]) in f64: f_i = |x_i|^2 - max_j z_ij, g_j = -price_j = |y_j|^2 + bias_j.  f_i + g_j <= |x_i - y_j|^2
        for every pair (up to the f32 rounding of the kernel's maxima) and mean f + mean g is lower_bound."""
        x, y = self._x.double(), self._y.double()
        return (x * x).sum(1) - self._best.double(), (y * y).sum(1) + self.bias.double()


def _certificate(x, y, bias, best, perm, all_assigned):
    """(cost, lower bound) in f64 from the device vectors."""
    xd, yd = x.double(), y.double()
    N = x.shape[0]
    lower = float(((xd * xd).sum() + (yd * yd).sum() + bias.double().sum() - best.double().sum()) / N)
    cost = float(((xd - yd.index_select(0, perm)) ** 2).sum(1).mean()) if all_assigned else float("nan")
    return cost, lower


@torch.no_grad()
def exact_assignment(x, y, eps: Optional[float] = None, eps_rel: float = 1e-4, eps_start_rel: float = 0.03,
                     theta: float = 8.0, check_every: int = 32, max_rounds: int = 100000) -> AssignmentResult:
    """The optimal matching between the clouds x, y [N, P] (f32, device; P % 4 == 0, P <= 768, N <= 65536) under the cost
    |x_i - y_j|^2, within eps of the optimum in mean cost, by eps-scaled auction rounds on the device.

    eps: in units of the squared distance; None takes eps_rel x mean_cost(x, y).  Phases run eps_start_rel x the mean cost,
    divided by theta from phase to phase while above eps, then eps itself.  check_every: rounds enqueued per host read of
    the unassigned count (a round without bidders changes nothing, so the result does not depend on it).  The solve ends
    without raising when a price stops moving or after max_rounds rounds: `converged` is then False and `reason` says
    which.  N == 1 is answered on the host."""
    _check_assignment_args(x, y, eps, eps_rel, eps_start_rel, theta, check_every, max_rounds)
    x, y = x.detach().contiguous(), y.detach().contiguous()
    dev, N = x.device, x.shape[0]
    check_every, max_rounds = int(check_every), int(max_rounds)
    bias = -(y * y).sum(1)
    mc = float(mean_cost(x, y))
    eps_f = float(eps) if eps is not None else float(eps_rel) * mc
    if N == 1:
        perm = torch.zeros(1, dtype=torch.int64, device=dev)
        best = 2.0 * (x * y).sum(1) + bias
        cost, lower = _certificate(x, y, bias, best, perm, True)
        z = torch.zeros(1, dtype=torch.int32, device=dev)
        return AssignmentResult(perm=perm, cost=cost, lower_bound=lower, gap=cost - lower, eps=eps_f, n_rounds=0, n_phases=0,
                                converged=True, reason="converged", phase_rounds=(), bias=bias, assigned=z, owner=z.clone(),
                                _best=best, _x=x, _y=y)
    if not eps_f > 0:
        raise ValueError("the mean cost of the clouds is zero (every point coincides): pass eps")
    assigned = torch.empty(N, dtype=torch.int32, device=dev)
    owner = torch.empty(N, dtype=torch.int32, device=dev)
    state = torch.zeros(2, dtype=torch.int32, device=dev)          # {unassigned rows, stalled}
    eps_t = torch.empty(1, dtype=torch.float32, device=dev)
    total, phases, reason = 0, [], "converged"
    for e in eps_schedule(float(eps_start_rel) * mc, eps_f, float(theta)):
        eps_t.fill_(e)
        assigned.fill_(-1)
        owner.fill_(-1)
        done = 0
        while True:
            k = min(check_every, max_rounds - total)
            ops.auction_rounds(x, y, bias, eps_t, assigned, owner, state[0:1], state[1:2], k)
            total, done = total + k, done + k
            left, stalled = state.tolist()
            if stalled:
                reason = "stalled"
            elif left and total >= max_rounds:
                reason = "max_rounds"
            if left == 0 or reason != "converged":
                break
        phases.append(done)
        if reason != "converged":
            break
    perm = assigned.long()
    all_assigned = bool(left == 0)
    _, best, _ = ops.sim_top2_bias(x, y, torch.full((1,), 2.0, dtype=torch.float32, device=dev), bias=bias, want_gap=False)
    cost, lower = _certificate(x, y, bias, best, perm, all_assigned)
    return AssignmentResult(perm=perm, cost=cost, lower_bound=lower, gap=cost - lower, eps=eps_f, n_rounds=total,
                            n_phases=len(phases), converged=reason == "converged", reason=reason,
                            phase_rounds=tuple(phases), bias=bias, assigned=assigned, owner=owner, _best=best, _x=x, _y=y)


def wasserstein2_exact(x, y, **solver_kw):
    """mean_i |x_i - y_perm(i)|^2 under the optimal matching of exact_assignment(x, y, **solver_kw), a differentiable 0-d
    tensor: the gradients flow through the gathered rows in plain torch, dW/dx_i = 2 (x_i - y_perm(i)) / N and its mirror
    image - by the envelope theorem the permutation is a constant.  Raises RuntimeError when the solve left rows
    unassigned."""
    r = exact_assignment(x, y, **solver_kw)
    if bool((r.perm < 0).any()):
        raise RuntimeError(f"exact_assignment did not converge ({r.reason}): no matching to take the distance of")
    return ((x - y.index_select(0, r.perm)) ** 2).sum(1).mean()
