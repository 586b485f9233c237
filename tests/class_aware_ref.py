"""Torch restatement of the class-aware InfoNCE (include/clipk.h: clipk_simce_lse_cls / clipk_simce_grad_cls and
clipk_sim_rank_cls) on materialised logits.

Two uses: the f64 reference the GPU tests compare the kernels with, and - as `simce_lse_cls` / `simce_grad_cls` with
the signatures of clip_dplm_amd.ops - a stand-in for the kernels in the CPU tests of the rank bookkeeping (gloo), the
way tests/ops_emulator.py stands in for the plain ones.
"""
import torch


def masks(Mx, Ny, Nc, label_offset, cls_x, cls_y, same_class, device):
    """(same, diag, in_d), each bool [Mx, Ny + Nc]."""
    j = torch.arange(Ny + Nc, device=device)
    i = torch.arange(Mx, device=device)
    diag = (j[None, :] == (label_offset + i)[:, None]) & (j[None, :] < Ny)
    same = diag.clone()
    if cls_x is not None:
        same[:, :Ny] |= cls_x.reshape(-1, 1) == cls_y.reshape(1, -1)
    in_d = torch.ones_like(same) if same_class == "positive" else ~(same & ~diag)
    return same, diag, in_d


def stats(S, Ny, label_offset, cls_x, cls_y, same_class, eps):
    """S [Mx, Ny + Nc] (the cache columns last) -> (lse, tgt, cnt, T, in_d) of the definitions, in S's dtype."""
    Mx, Nk = S.shape
    same, diag, in_d = masks(Mx, Ny, Nk - Ny, label_offset, cls_x, cls_y, same_class, S.device)
    c = same.sum(1).to(S.dtype)
    n = in_d.sum(1).to(S.dtype)
    q = same.to(S.dtype) / c[:, None] if same_class == "positive" else diag.to(S.dtype)
    T = (1.0 - eps) * q + eps / n[:, None] * in_d.to(S.dtype)
    lse = torch.logsumexp(S.masked_fill(~in_d, float("-inf")), 1)
    tgt = (T * S).sum(1)
    return lse, tgt, c, T, in_d


def loss_from_logits(S, Ny, cls, same_class, eps, w_row, w_col):
    """Global loss of a square pair batch: S [Bg, Bg + Nc] = scale a_g [b_g | cache]^T, cls [Bg] (or None)."""
    Bg = S.shape[0]
    lse_r, tgt_r = stats(S, Ny, 0, cls, cls, same_class, eps)[:2]
    out = w_row * (lse_r - tgt_r).sum()
    if w_col != 0.0:
        lse_c, tgt_c = stats(S[:, :Ny].t(), Ny, 0, cls, cls, same_class, eps)[:2]
        out = out + w_col * (lse_c - tgt_c).sum()
    return out / Bg


# ---- stand-ins for clip_dplm_amd.ops (same signatures and return values)
def _keys(y, cache):
    return y if cache is None else torch.cat([y, cache], 0)


def simce_lse_cls(x, y, scale, cls_x=None, cls_y=None, same_class="mask", eps=0.0, label_offset=0, cache=None):
    S = scale.reshape(()) * (x @ _keys(y, cache).t())
    lse, tgt, cnt = stats(S, y.shape[0], label_offset, cls_x, cls_y, same_class, eps)[:3]
    return lse.detach(), tgt.detach(), cnt.detach()


def simce_grad_cls(x, y, scale, lse_x, lse_y, cnt_x, cnt_y, w_row, w_col, inv_bg, nkeys_y, cls_x=None, cls_y=None,
                   same_class="mask", eps=0.0, label_offset=0, cache=None, upstream=None):
    """G from the definitions (include/clipk.h), then dX = scale G K and dscale partials = rowsum(G * X K^T)."""
    with torch.no_grad():
        K = _keys(y, cache)
        Ny, Nk = y.shape[0], K.shape[0]
        D = x @ K.t()
        S = scale.reshape(()) * D
        same, diag, in_d = masks(x.shape[0], Ny, Nk - Ny, label_offset, cls_x, cls_y, same_class, x.device)
        pos = same_class == "positive"
        f = lambda m: m.to(S.dtype)
        G = torch.zeros_like(S)
        if w_row != 0.0:
            cx = cnt_x.to(S.dtype)[:, None]
            nx = float(Nk) if pos else Nk - (cx - 1.0)
            q = f(same) / cx if pos else f(diag)
            T = (1.0 - eps) * q + eps / nx * f(in_d)
            G += w_row * (f(in_d) * torch.exp(S - lse_x[:, None]) - T)
        if w_col != 0.0:
            cy = cnt_y.to(S.dtype)[None, :]
            ny = float(nkeys_y) if pos else nkeys_y - (cy - 1.0)
            q = f(same[:, :Ny]) / cy if pos else f(diag[:, :Ny])
            T = (1.0 - eps) * q + eps / ny * f(in_d[:, :Ny])
            G[:, :Ny] += w_col * (f(in_d[:, :Ny]) * torch.exp(S[:, :Ny] - lse_y[None, :]) - T)
        G = G * (inv_bg if upstream is None else inv_bg * upstream.reshape(()))
        return scale.reshape(()) * (G @ K), (G * D).sum(1)


def filtered_rank(S, labels, cls):
    """rank_i = #{j : cls[j] != cls[l_i] and (S[i,j] > S[i,l_i] or (S[i,j] == S[i,l_i] and j < l_i))}."""
    i = torch.arange(S.shape[0], device=S.device)
    p = S[i, labels][:, None]
    j = torch.arange(S.shape[1], device=S.device)[None, :]
    before = (S > p) | ((S == p) & (j < labels[:, None]))
    other = cls[None, :] != cls[labels][:, None]
    return (before & other).sum(1)
