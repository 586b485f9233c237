"""Restatement of the bf16x3 Sinkhorn (include/clipk.h: clipk_sim_lse_bias_x3; ot.sinkhorn(..., precision="bf16x3")) in
plain torch on the CPU, the matrix materialised.

    hi = bf16(x) (round to nearest even), lo = bf16(x - hi)            x - hi is exact in f32
    A_ij = sum_p hi(x)hi(y) + hi(x)lo(y) + lo(x)hi(y)                  in f64 here, from the planes
    half-iteration:  nv_i = logw_i - LSE_j(scale A_ij + bias_j)
    solve:  the iterations of sinkhorn_ref.solve on scale A, then one iteration on the exact scale <x, y>

and the error bound of the split logits and what follows from it for a converged solve (DESIGN.md has the derivation):

    |scale A_ij - scale <x_i, y_j>| <= eta = |scale| max|x| max|y| eps_rel + eps_abs
    row-marginal L1 error <= e^{2 eta} - 1,  |value - OT_eps| <= 4 eps eta,
    |envelope gradient of row i - exact| <= (e^{4 eta} - 1) 2 a_i (|x_i| + max|y|)
"""
import math
from types import SimpleNamespace

import torch

import sinkhorn_ref as ref

F64 = torch.float64
V = 2.0 ** -8                      # unit roundoff of bf16


def split(x):
    """(hi, lo) of an f32 tensor, in f64."""
    x = x.float()
    hi = x.bfloat16().float()
    lo = (x - hi).bfloat16().float()
    return hi.double(), lo.double()


def product(x, y):
    """A [M, N] in f64 from the planes of the f32 clouds x, y."""
    xh, xl = split(x)
    yh, yl = split(y)
    return xh @ yh.T + xh @ yl.T + xl @ yh.T


def eps_rel(P):
    """retrieval.prefilter_eps_rel(P, "bf16x3"), restated: dropped terms + MFMA accumulation + the f32 kernel + scale."""
    return 3 * V * V + 7 * V ** 3 + accumulation_term(P) + P * 2.0 ** -23 + 2.0 ** -22


def accumulation_term(P):
    """The part of eps_rel that bounds the f32 accumulation of the 3 P exact products (gamma = n 2^-22)."""
    return 3 * P * 2.0 ** -22 * (1 + V) ** 2 * (1 + 2 * V)


def logit_error_bound(x, y, scale):
    """eta: a float, from f64 norms."""
    xn, yn = float(x.double().norm(dim=1).max()), float(y.double().norm(dim=1).max())
    s, P = abs(float(scale)), x.shape[1]
    return s * xn * yn * eps_rel(P) + (s * P * (xn + yn + 1.0) + 1.0) * 2.0 ** -120


def half_iteration(x, y, scale, bias=None, logw=None):
    """logw_i - LSE_j(scale A_ij + bias_j) in f64 over the split products."""
    s = float(scale) * product(x, y)
    if bias is not None:
        s = s + bias.double()[None, :]
    out = -torch.logsumexp(s, dim=1)
    return out if logw is None else out + logw.double()


def _iterate(S, loga, logb, u, v, n, symmetric):
    for _ in range(n):
        if symmetric:
            u = 0.5 * (u + loga - torch.logsumexp(S + u[None, :], dim=1))
            v = u
        else:
            u = loga - torch.logsumexp(S + v[None, :], dim=1)
            v = logb - torch.logsumexp(S + u[:, None], dim=0)
    return u, v


def solve(x, y, eps, a=None, b=None, n_split=100, n_exact=1, symmetric=False):
    """n_split iterations on scale A, then n_exact on the exact scale <x, y>, all in f64; the fields of
    sinkhorn_ref.solve (S is the EXACT scaled similarity: plan() and marginal_error() of sinkhorn_ref apply), plus
    split_error, the row-marginal error of the split plan before the exact iterations, and eta."""
    x64, y64 = x.double(), y.double()
    a, b = ref.weights(len(x), a, F64), ref.weights(len(y), b, F64)
    eps = torch.as_tensor(eps, dtype=F64)
    scale = 2.0 / eps
    S = scale * (x64 @ y64.T)
    SA = scale * product(x, y)
    loga, logb = a.log(), b.log()
    u, v = _iterate(SA, loga, logb, loga, logb, n_split, symmetric)
    split_error = float(((SA + u[:, None] + v[None, :]).exp().sum(1) - a).abs().sum()) if n_split else float("nan")
    u, v = _iterate(S, loga, logb, u, v, n_exact, symmetric)
    nx, ny = (x64 * x64).sum(1), (y64 * y64).sum(1)
    f, g = eps * (u - loga) + nx, eps * (v - logb) + ny
    return SimpleNamespace(u=u, v=v, f=f, g=g, eps=eps, value=a @ f + b @ g, S=S, loga=loga, logb=logb, a=a, b=b, nx=nx,
                           ny=ny, x=x64, y=y64, split_error=split_error, eta=logit_error_bound(x, y, scale))


def gradient_bound(r):
    """[M]: the bound on |envelope gradient of row i - exact|, (e^{4 eta} - 1) 2 a_i (|x_i| + max|y|)."""
    return math.expm1(4 * r.eta) * 2.0 * r.a * (r.x.norm(dim=1) + r.y.norm(dim=1).max())
