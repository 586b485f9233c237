"""Restatement of the entropic optimal transport of clip_dplm_amd.ot in plain torch on the CPU, the matrix materialised.

    C_ij = |x_i - y_j|^2,  OT_eps = min_P <P, C> + eps KL(P | a (x) b),  S = (2 / eps) x y^T
    u_i = log a_i - LSE_j(S_ij + v_j),  v_j = log b_j - LSE_i(S_ij + u_i),  start v = log b, one iteration = u then v
    P_ij = exp(S_ij + u_i + v_j),  f = eps (u - log a) + |x|^2,  g = eps (v - log b) + |y|^2,  OT_eps = <a, f> + <b, g>
    symmetric (x = y, a = b): u <- (u + log a - LSE(S + u)) / 2
    S_eps = OT_eps(x, y) - OT_eps(x, x) / 2 - OT_eps(y, y) / 2

It runs where its inputs are: on the CPU, except that the GPU tests hand it device tensors for their largest shapes
(100003 keys, a 4097 x 4097 self problem under autograd), where torch's own f64 / f32 kernels take seconds off a case.
dtype=torch.float64 is the reference; dtype=torch.float32 on the same inputs is the yardstick for tolerances (what plain
f32 arithmetic in another summation order makes of the same formulae).  Everything is differentiable torch, so autograd
through the unrolled iterations checks the envelope gradients.
"""
import math
from types import SimpleNamespace

import torch
from torch.utils.checkpoint import checkpoint


def weights(n, w, dtype, device=None):
    return torch.full((n,), 1.0 / n, dtype=dtype, device=device) if w is None else w.to(device=device, dtype=dtype)


def cost_matrix(x, y):
    return (x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2.0 * x @ y.T


def mean_cost_explicit(x, y, a=None, b=None):
    """sum_ij a_i b_j C_ij over the explicit matrix (what ot.mean_cost gets in closed form)."""
    a, b = weights(len(x), a, x.dtype, x.device), weights(len(y), b, x.dtype, x.device)
    return a @ cost_matrix(x, y) @ b


def half_iteration(x, y, scale, bias=None, logw=None, rows=512):
    """logw_i - LSE_j(scale <x_i, y_j> + bias_j), the rows in chunks (the matrix of the large cases stays small)."""
    out = []
    for i in range(0, len(x), rows):
        s = scale * (x[i:i + rows] @ y.T)
        if bias is not None:
            s = s + bias[None, :]
        out.append(-torch.logsumexp(s, dim=1))
    out = torch.cat(out)
    return out if logw is None else out + logw


def marginal_error_term(logw, prev, nv):
    """sum_i w_i |exp(prev_i - nv_i) - 1|: the L1 marginal error of the potential `prev` that the update nv replaces."""
    return (logw.exp() * ((prev - nv).exp() - 1.0).abs()).sum()


def solve(x, y, eps=None, eps_rel=0.05, a=None, b=None, n_iters=100, symmetric=False, dtype=torch.float64):
    """n_iters Sinkhorn iterations.  Returns u, v, f, g, eps, value, S (the scaled similarity), loga, logb, a, b and the
    squared norms, in `dtype`."""
    x, y = x.to(dtype), y.to(dtype)
    a, b = weights(len(x), a, dtype, x.device), weights(len(y), b, dtype, x.device)
    if eps is None:
        eps = eps_rel * mean_cost_explicit(x.detach(), y.detach(), a, b)
    eps = torch.as_tensor(eps, dtype=dtype, device=x.device)
    S = (2.0 / eps) * (x @ y.T)
    loga, logb = a.log(), b.log()

    def sym_step(u):
        return 0.5 * (u + loga - torch.logsumexp(S + u[None, :], dim=1))

    def step(v):
        u = loga - torch.logsumexp(S + v[None, :], dim=1)
        return u, logb - torch.logsumexp(S + u[:, None], dim=0)

    # under autograd a large problem keeps the potentials only and recomputes an iteration's matrix in the backward pass
    # (the same arithmetic): a hundred saved M x N matrices are gigabytes
    if S.requires_grad and S.numel() > (1 << 20):
        plain_sym, plain = sym_step, step
        sym_step = lambda u: checkpoint(plain_sym, u, use_reentrant=False)
        step = lambda v: checkpoint(plain, v, use_reentrant=False)
    if symmetric:
        u = loga
        for _ in range(n_iters):
            u = sym_step(u)
        v = u
    else:
        v = logb
        for _ in range(n_iters):
            u, v = step(v)
    nx, ny = (x * x).sum(1), (y * y).sum(1)
    f, g = eps * (u - loga) + nx, eps * (v - logb) + ny
    return SimpleNamespace(u=u, v=v, f=f, g=g, eps=eps, value=a @ f + b @ g, S=S, loga=loga, logb=logb, a=a, b=b, nx=nx, ny=ny,
                           x=x, y=y)


def plan(r):
    return (r.S + r.u[:, None] + r.v[None, :]).exp()


def plan_sums(x, y, scale, u, v, rows=512):
    """(mass, bary, cost) of the plan exp(scale x y^T + u_i + v_j), the rows in chunks: sum_j P_ij, sum_j P_ij y_j,
    sum_j P_ij C_ij."""
    mass, bary, cost = [], [], []
    ny = (y * y).sum(1)
    for i in range(0, len(x), rows):
        xc = x[i:i + rows]
        d = xc @ y.T
        p = (scale * d + u[i:i + rows, None] + v[None, :]).exp()
        mass.append(p.sum(1))
        bary.append(p @ y)
        cost.append((p * ((xc * xc).sum(1)[:, None] + ny[None, :] - 2.0 * d)).sum(1))
    return torch.cat(mass), torch.cat(bary), torch.cat(cost)


def marginal_error(r):
    """L1 distance of the plan's row marginal from a."""
    return (plan(r).sum(1) - r.a).abs().sum()


def transport_cost(r):
    return (plan(r) * cost_matrix(r.x, r.y)).sum()


def barycentric_map(r):
    p = plan(r)
    return (p @ r.y) / p.sum(1)[:, None]


def envelope_gradients(r):
    """(dOT/dx, dOT/dy) = (2 (r_i x_i - sum_j P_ij y_j), 2 (c_j y_j - sum_i P_ij x_i)) from the potentials."""
    p = plan(r)
    return 2.0 * (p.sum(1)[:, None] * r.x - p @ r.y), 2.0 * (p.sum(0)[:, None] * r.y - p.T @ r.x)


def divergence(x, y, eps, a=None, b=None, n_iters=100, dtype=torch.float64):
    """S_eps as a differentiable scalar (autograd runs through the unrolled iterations).  A cloud with itself (y is x, b
    is a): the cross term is a symmetric problem too."""
    xy = solve(x, y, eps, a=a, b=b, n_iters=n_iters, symmetric=y is x and b is a, dtype=dtype)
    xx = solve(x, x, xy.eps, a=a, b=a, n_iters=n_iters, symmetric=True, dtype=dtype)
    yy = solve(y, y, xy.eps, a=b, b=b, n_iters=n_iters, symmetric=True, dtype=dtype)
    return xy.value - 0.5 * xx.value - 0.5 * yy.value


def divergence_envelope_gradients(x, y, eps, a=None, b=None, n_iters=100, dtype=torch.float64):
    """(S_eps, d/dx, d/dy, OT_eps(x, y)): the gradients by the envelope theorem, the cross term's gradient minus the self
    term's row gradient."""
    xy = solve(x, y, eps, a=a, b=b, n_iters=n_iters, dtype=dtype)
    xx = solve(x, x, xy.eps, a=a, b=a, n_iters=n_iters, symmetric=True, dtype=dtype)
    yy = solve(y, y, xy.eps, a=b, b=b, n_iters=n_iters, symmetric=True, dtype=dtype)
    gx, gy = envelope_gradients(xy)
    value = xy.value - 0.5 * xx.value - 0.5 * yy.value
    return value, gx - envelope_gradients(xx)[0], gy - envelope_gradients(yy)[0], xy.value


def unit_clouds(M, N, P, seed, shift=0.3):
    """Seeded unit-norm rows in f32, the keys shifted by shift * sqrt(P) along the first axis before normalising."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, P, generator=g, dtype=torch.float64)
    y = torch.randn(N, P, generator=g, dtype=torch.float64)
    y[:, 0] += shift * math.sqrt(P)
    n = torch.nn.functional.normalize
    return n(x, dim=1).float(), n(y, dim=1).float()


def random_weights(n, seed):
    g = torch.Generator().manual_seed(seed)
    w = 0.5 + torch.rand(n, generator=g, dtype=torch.float64)
    return (w / w.sum()).float()
