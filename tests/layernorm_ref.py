"""Plain f64 references of the LayerNorm family in csrc/rowwise.hip (forward with fused activation, first and second
backward, LayerNorm + masked mean pooling), the seeded input families the LayerNorm tests share, and the per-element
tolerances they allow.  Pure torch on the CPU; the activations come from tests/elementwise_ref.py; nothing is imported
from clip_dplm_amd.  Inputs are the f32 or bf16-rounded values the kernel sees, widened to f64.

tests/test_layernorm_ref_host.py pins every function here against torch's own f64 F.layer_norm + autograd and checks that
the f32 stand-in tests/ops_emulator.py stays within a quarter of every bound; tests/test_gpu_layernorm.py compares the HIP
kernels with them.

Tolerances (all against f64, none taken from GPU output).  u = 2^-23; per row A = max(1, max|x| rstd); G = max|gamma|;
t = dy act'(n) with n the pre-activation; D = max|t gamma| of the row:
    y32      8 u A G + 2 u |ref|  (+ elementwise_ref.act_tol of the activation)
    mean     4 u max|x|                                  (5.6 u on family (b), 7.2 u on (d): MEAN_K below)
    rstd     8 u A rstd
    dx32     8 u A rstd D + 2 u |ref|  (+ the bf16 half-ulp of dx_add where it is bf16)
    dbeta    4e-7 sum_r |t| + 1e-6                      (the project's column-sum bound; 5.0e-7 .. 7.5e-7: DBETA_K below)
    dgamma   8 u sum_r A_r |t| + 1e-6
    second order   2e-4 max(1, max|ref|)
The statistics are sums of at most 80 f32 terms per lane and a 6-step butterfly, x - mean loses max|x| u / 2 absolute, i.e.
A u / 2 of a normalised value of order one: hence the factor A everywhere.  The f32 stand-in measured on families (a)-(c)
stays below 1.6 u A (y) and 6 u A rstd (dx, D ~ 4), so the constants leave about 5x.

Mean pooling (L <= 9 rows per sample here: at most 3 sequential adds per wave, 3 adds across the waves, the rounded 1 / n and
its product: 8 roundings of 2^-24 = 4 u):
    row_weight   u w
    pooled       sum_valid w (y bound) + 4 u sum_valid w |y|
    dx, dgamma   the first-order bounds with dy = dpooled[b] w  (the product's u / 2 sits inside the 8 u A terms)
    dbeta        1.4e-6 sum_r |dy| + 1e-6  (the L rows of a sample carry the SAME rounded dy = dpooled[b] w, so that rounding
                 adds up coherently in the column sum; 4x the stand-in's worst error + 10 %: POOL_DBETA_K below)
"""
import torch

import elementwise_ref as E

F64 = torch.float64
U = 2.0 ** -23
FAMILIES = ("a", "b", "c", "d")
CONST = 3.7                      # family (d): the value of the constant row


def _w(t):
    return None if t is None else t.detach().cpu().to(F64)


# ---------------------------------------------------------------------------------------------- inputs
def randn(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float32) * scale + shift).to(torch.float32)


def family(name, rows, cols, seed, eps, bf16=False):
    """(x f32 [rows, cols], eps) of an input family: (a) N(0, 2^2); (b) 100 + N(0, 1); (c) N(0, 1e-6) with eps 1e-5;
    (d) N(0, 2^2) with row rows // 2 constant (CONST), eps 1e-5.  bf16: the values rounded to bf16 (still an f32 tensor)."""
    if name == "a":
        x = randn((rows, cols), seed, 2.0)
    elif name == "b":
        x = randn((rows, cols), seed, 1.0, 100.0)
    elif name == "c":
        x, eps = randn((rows, cols), seed, 1e-3), 1e-5
    elif name == "d":
        x, eps = randn((rows, cols), seed, 2.0), 1e-5
        x[rows // 2] = CONST
    else:
        raise ValueError(name)
    if bf16:
        x = x.to(torch.bfloat16).to(torch.float32)
    return x, eps


def params(cols, seed):
    """gamma = 1 + 0.2 N, beta = 0.1 N (f32)."""
    return randn((cols,), seed, 0.2, 1.0), randn((cols,), seed + 1, 0.1)


# ---------------------------------------------------------------------------------------------- first order
def _fwd(x, gamma, beta, eps):
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    rstd = ((xc * xc).mean(-1, keepdim=True) + eps) ** -0.5
    xh = xc * rstd
    return xh, xh * gamma + beta, mean, rstd


def _bwd(dy, x, gamma, beta, eps, act):
    """Closed form: t = dy act'(n), u = t gamma, dx = rstd (u - mean u - xh mean(u xh)), dgamma = sum_r t xh, dbeta = sum_r t."""
    xh, n, _, rstd = _fwd(x, gamma, beta, eps)
    t = dy if act is None else dy * E.act_grad(n, act)
    u = t * gamma
    dx = rstd * (u - u.mean(-1, keepdim=True) - xh * (u * xh).mean(-1, keepdim=True))
    return dx, (t * xh).sum(0), t.sum(0), t


def layernorm(x, gamma, beta, eps, act=None):
    """y = act(LayerNorm(x)) with the biased variance, mean [rows], rstd [rows]."""
    _, n, mean, rstd = _fwd(_w(x), _w(gamma), _w(beta), eps)
    return (n if act is None else E.act(n, act)), mean.squeeze(-1), rstd.squeeze(-1)


def layernorm_bwd(dy, x, gamma, beta, eps, act=None, dx_add=None):
    """dx (+ dx_add), dgamma, dbeta."""
    dx, dg, db, _ = _bwd(_w(dy), _w(x), _w(gamma), _w(beta), eps, act)
    return (dx if dx_add is None else dx + _w(dx_add)), dg, db


def layernorm_bwd2(g, dy, a, gamma, beta, eps, act=None):
    """Backward of the first backward da(dy, a, gamma, beta) under the cotangent g, by f64 autograd over the closed form:
    (d_dy, d_a, d_gamma, d_beta); d_beta = 0 without an activation."""
    dy, a, gamma, beta = (_w(t).requires_grad_(True) for t in (dy, a, gamma, beta))
    with torch.enable_grad():
        da = _bwd(dy, a, gamma, beta, eps, act)[0]
        outs = torch.autograd.grad(da, [dy, a, gamma, beta], _w(g), allow_unused=True)
    return tuple(torch.zeros_like(p) if o is None else o for o, p in zip(outs, (dy, a, gamma, beta)))


def bwd2_tol(ref):
    return 2e-4 * max(1.0, float(ref.abs().max()))


def half_ulp_bf16(v):
    v = v.to(F64).abs().clamp(min=2.0 ** -126)
    return 2.0 ** (torch.floor(torch.log2(v)) - 8)


# Constants raised from the table's 4 u (mean) and 4e-7 (dbeta) where the f32 stand-in missed a quarter of the bound: each is
# 4x the stand-in's worst error in that case plus 10 %, since the stand-in's own summation order - and with it its worst error,
# by 1.3 % between two machines tried - depends on the CPU's vector width (tests/test_layernorm_ref_host.py records the figures).
MEAN_K = {"a": 4 * U, "b": 5.6 * U, "c": 4 * U, "d": 7.2 * U}
DBETA_K = {None: 5.0e-7, "gelu": 7.5e-7, "celu": 6.3e-7, "softplus": 5.0e-7}
# Backward through an activation is compared on these families only: at |mean| >> std (b) and on a constant row (d) the
# error of the normalised value, A u, reaches t = dy act'(n) through act'' and the column-sum bounds above do not model it
# (the stand-in is off by 1e3 .. 1e5 times the dbeta constant there); forward with an activation runs on every family.
ACT_BWD_FAMILIES = ("a", "c")
POOL_DBETA_K = 1.4e-6


def bounds(x, gamma, beta, eps, act=None, dy=None, dx_add=None, add_bf16=False, fam="a"):
    """Allowed |kernel - f64| as a dict: y [rows, cols], mean, rstd [rows]; with dy also dx [rows, cols], dgamma, dbeta
    [cols] (module docstring); fam: the input family, for the two raised constants."""
    x, gamma, beta = _w(x), _w(gamma), _w(beta)
    _, n, _, rstd = _fwd(x, gamma, beta, eps)
    xmax = x.abs().amax(-1, keepdim=True)
    A = (xmax * rstd).clamp(min=1.0)
    G = float(gamma.abs().max())
    y = n if act is None else E.act(n, act)
    out = {"y": 8 * U * A * G + 2 * U * y.abs() + (0.0 if act is None else E.act_tol(n, act, False, y)),
           "mean": MEAN_K[fam] * xmax.squeeze(-1), "rstd": (8 * U * A * rstd).squeeze(-1)}
    if dy is not None:
        dx, _, _, t = _bwd(_w(dy), x, gamma, beta, eps, act)
        if dx_add is not None:
            dx = dx + _w(dx_add)
        D = (t * gamma).abs().amax(-1, keepdim=True)
        out["dx"] = 8 * U * A * rstd * D + 2 * U * dx.abs()
        if dx_add is not None and add_bf16:
            out["dx"] = out["dx"] + half_ulp_bf16(_w(dx_add))
        out["dbeta"] = DBETA_K[act] * t.abs().sum(0) + 1e-6
        out["dgamma"] = 8 * U * (A * t.abs()).sum(0) + 1e-6
    return out


# ---------------------------------------------------------------------------------------------- mean pooling
def _weights(B, L, mask):
    m = torch.ones(B * L, dtype=F64) if mask is None else (mask.detach().cpu().view(-1) != 0).to(F64)
    n = m.view(B, L).sum(1)
    inv = torch.where(n > 0, 1.0 / n.clamp(min=1.0), torch.zeros_like(n))
    return m * inv.repeat_interleave(L)


def meanpool(x, gamma, beta, eps, B, L, mask=None):
    """pooled [B, cols] = mean over the valid rows of LayerNorm(x) (0 for a sample without any) and row_weight [B * L]
    (1 / #valid rows of the row's sample, 0 for a masked row)."""
    y, _, _ = layernorm(x, gamma, beta, eps)
    w = _weights(B, L, mask)
    return (y * w[:, None]).view(B, L, -1).sum(1), w


def meanpool_bwd(dpooled, x, gamma, beta, eps, B, L, mask=None):
    """dx, dgamma, dbeta of meanpool: the first backward with dy[r] = dpooled[r // L] row_weight[r]."""
    dy = _w(dpooled).repeat_interleave(L, 0) * _weights(B, L, mask)[:, None]
    return layernorm_bwd(dy, x, gamma, beta, eps)


def meanpool_bounds(x, gamma, beta, eps, B, L, mask=None, dpooled=None):
    """pooled [B, cols], row_weight [B * L]; with dpooled also dx, dgamma, dbeta (module docstring)."""
    w = _weights(B, L, mask)
    dy = None if dpooled is None else _w(dpooled).repeat_interleave(L, 0) * w[:, None]
    b = bounds(x, gamma, beta, eps, dy=dy)
    y, _, _ = layernorm(x, gamma, beta, eps)
    out = {"pooled": ((b["y"] + 4 * U * y.abs()) * w[:, None]).view(B, L, -1).sum(1), "row_weight": U * w}
    if dpooled is not None:
        out.update(dx=b["dx"], dgamma=b["dgamma"], dbeta=POOL_DBETA_K * dy.abs().sum(0) + 1e-6)
    return out
