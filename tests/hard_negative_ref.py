"""Torch restatement of the hard-negative-weighted InfoNCE (include/clipk.h: clipk_simce_lse_hard /
clipk_simce_grad_hard) on materialised logits: the importance weighting of Robinson et al., "Contrastive Learning with
Hard Negative Samples" (ICLR 2021) with tau_plus = 0.

Two uses: the reference (f64 when given f64) the GPU tests compare the kernels with, and - as `simce_lse_hard` /
`simce_grad_hard` with the signatures of clip_dplm_amd.ops - a stand-in for the kernels in the CPU tests of the rank
bookkeeping (gloo), as tests/class_aware_ref.py is for the class-aware loss.  The reference project has no values for
this variant, so tests/test_hard_negative_host.py pins this file against an independent transcription first.
"""
import math

import torch

NEG_INF = float("-inf")


def neg_mask(Mx, Ny, Nc, label_offset, cls_x, cls_y, device):
    """(neg, diag), each bool [Mx, Ny + Nc]: Neg_i = {j != l_i} minus the same-class batch keys; cache keys stay."""
    j = torch.arange(Ny + Nc, device=device)
    i = torch.arange(Mx, device=device)
    diag = (j[None, :] == (label_offset + i)[:, None]) & (j[None, :] < Ny)
    neg = ~diag
    if cls_x is not None:
        neg[:, :Ny] &= cls_x.reshape(-1, 1) != cls_y.reshape(1, -1)
    return neg, diag


def stats(S, Ny, label_offset, cls_x, cls_y, beta):
    """S [Mx, Ny + Nc] (the cache columns last) -> dict of the definition's per-row quantities, in S's dtype."""
    Mx, Nk = S.shape
    neg, diag = neg_mask(Mx, Ny, Nk - Ny, label_offset, cls_x, cls_y, S.device)
    n = neg.sum(1).to(S.dtype)
    some = n > 0
    # rows without negatives: A = C = logNg = -inf by definition.  They are computed over all keys instead and then
    # replaced, so that autograd sees no (-inf) - (-inf): torch.where passes such a row a zero gradient.
    safe = neg | ~some[:, None]
    ninf = torch.full_like(n, NEG_INF)
    A_s = torch.logsumexp((beta * S).masked_fill(~safe, NEG_INF), 1)
    C_s = torch.logsumexp(((1.0 + beta) * S).masked_fill(~safe, NEG_INF), 1)
    pos = (S * diag.to(S.dtype)).sum(1)
    lng_s = torch.log(n.clamp(min=1)) + C_s - A_s
    lse_h = torch.where(some, torch.logaddexp(pos, lng_s), pos)
    return dict(neg=neg, diag=diag, n=n, A=torch.where(some, A_s, ninf), C=torch.where(some, C_s, ninf),
                logNg=torch.where(some, lng_s, ninf), pos=pos, lse_h=lse_h, loss=lse_h - pos)


def coefficients(st, beta):
    """[3, Mx]: q = exp(logNg - lse_h), k1 = log(q (1 + beta)) - C, k2 = log(q beta) - A (-inf where the factor is 0)."""
    some = st["n"] > 0
    ninf = torch.full_like(st["n"], NEG_INF)
    zero = torch.zeros_like(ninf)
    lq = torch.where(some, st["logNg"] - st["lse_h"], ninf)
    k1 = torch.where(some, lq + math.log1p(beta) - torch.where(some, st["C"], zero), ninf)
    k2 = torch.where(some, lq + math.log(beta) - torch.where(some, st["A"], zero), ninf) if beta > 0 else ninf
    return torch.stack([torch.exp(lq), k1, k2])


def direction_grad(S, Ny, label_offset, cls_x, cls_y, beta, coef=None):
    """Closed-form g = d sum_i loss_i / dS of one direction, [Mx, Ny + Nc]."""
    st = stats(S, Ny, label_offset, cls_x, cls_y, beta)
    q, k1, k2 = coefficients(st, beta) if coef is None else coef.to(S.dtype)
    e1 = torch.exp(((1.0 + beta) * S + k1[:, None]).masked_fill(~st["neg"], NEG_INF))     # selected, never multiplied
    e2 = torch.exp((beta * S + k2[:, None]).masked_fill(~st["neg"], NEG_INF)) if beta > 0 else torch.zeros_like(S)
    return e1 - e2 - q[:, None] * st["diag"].to(S.dtype)


def loss_from_logits(S, Ny, cls, beta, w_row, w_col):
    """Global loss of a square pair batch: S [Bg, Bg + Nc] = scale a_g [b_g | cache]^T, cls [Bg] (or None)."""
    Bg = S.shape[0]
    out = w_row * stats(S, Ny, 0, cls, cls, beta)["loss"].sum()
    if w_col != 0.0:
        out = out + w_col * stats(S[:, :Ny].t(), Ny, 0, cls, cls, beta)["loss"].sum()
    return out / Bg


# ---- stand-ins for clip_dplm_amd.ops (same signatures and return values)
def _keys(y, cache):
    return y if cache is None else torch.cat([y, cache], 0)


def simce_lse_hard(x, y, scale, beta, cls_x=None, cls_y=None, label_offset=0, cache=None):
    with torch.no_grad():
        S = scale.reshape(()) * (x @ _keys(y, cache).t())
        st = stats(S, y.shape[0], label_offset, cls_x, cls_y, beta)
        return st["lse_h"], st["pos"], coefficients(st, beta)


def simce_grad_hard(x, y, scale, beta, coef_x, coef_y, w_row, w_col, inv_bg, cls_x=None, cls_y=None, label_offset=0,
                    cache=None, upstream=None):
    """G from the coefficients (include/clipk.h), then dX = scale G K and dscale partials = rowsum(G * X K^T)."""
    with torch.no_grad():
        K = _keys(y, cache)
        Mx, Ny = x.shape[0], y.shape[0]
        D = x @ K.t()
        S = scale.reshape(()) * D
        neg, diag = neg_mask(Mx, Ny, K.shape[0] - Ny, label_offset, cls_x, cls_y, x.device)
        b1 = 1.0 + beta

        def g(Sd, q, k1, k2, negd, diagd):            # q, k1, k2 broadcast along the direction's own rows
            e = torch.exp((b1 * Sd + k1).masked_fill(~negd, NEG_INF)) - torch.exp((beta * Sd + k2).masked_fill(~negd, NEG_INF))
            return e - q * diagd.to(Sd.dtype)
        G = w_row * g(S, coef_x[0][:, None], coef_x[1][:, None], coef_x[2][:, None], neg, diag)
        G[:, :Ny] += w_col * g(S[:, :Ny], coef_y[0][None, :], coef_y[1][None, :], coef_y[2][None, :], neg[:, :Ny],
                               diag[:, :Ny])
        G = G * (inv_bg if upstream is None else inv_bg * upstream.reshape(()))
        return scale.reshape(()) * (G @ K), (G * D).sum(1)
