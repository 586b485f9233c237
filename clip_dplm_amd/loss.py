"""Fused CLIP / InfoNCE loss on the simce kernels — the B x B (or B_local x B_global) logits never exist.

Reference losses covered (weights select the variant):
  * one-sided  CE(S, arange)                      old/ablation.py:16, run1/full.py:133      (w_row=1, w_col=0)
  * symmetric  (CE(S) + CE(S^T)) / 2              current/rna_clip_codes.ipynb:1952-1953    (0.5, 0.5)
  * cache-negative variant                        old/clip_opt.py:130-151                   (0.5, 0.5, cache=...)
  * global batch over ranks                       old/clip_opt.py:102-112 — but differentiable
  * class-aware / label-smoothed InfoNCE          class_ids=, same_class=, label_smoothing= (include/clipk.h:
                                                  clipk_simce_lse_cls): pairs that share a partner stop being each
                                                  other's negatives ("mask") or become positives ("positive")
  * hard-negative-weighted InfoNCE                run1/full.py:347 'hard_negative', configuration_hybrid_clip.py:105-106
                                                  hard_negative_beta= (include/clipk.h: clipk_simce_lse_hard)

Multi-GPU scheme: one all-gather of the stacked embeddings [2, B_l, P], one
all-gather of the two LSE vectors [2, B_l]; every rank then computes the COMPLETE gradient of the global
loss w.r.t. its own rows locally — no embedding-gradient reduce-scatter is needed.  Parameter gradients are
summed across ranks afterwards by the optimiser's reduce-scatter.
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.distributed as dist

from . import ops

# kernel namespace; tests of the rank bookkeeping (gloo, CPU) substitute a torch restatement here — the product
# itself never does: ops.* raise on anything but device tensors.
_kernels = ops


def _gather_cat(t: torch.Tensor, group) -> torch.Tensor:
    world = dist.get_world_size(group)
    t = t.contiguous()
    out = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    dist.all_gather_into_tensor(out, t, group=group)          # concatenation along dim 0 (works on nccl and gloo)
    return out.view((world,) + tuple(t.shape))


_INF = {}


def _inf_like(t: torch.Tensor) -> torch.Tensor:
    """A read-only +inf vector of t's shape, made once per (device, length): the one-sided loss's unused direction."""
    key = (str(t.device), t.numel())
    v = _INF.get(key)
    if v is None:
        v = _INF[key] = torch.full((t.numel(),), float("inf"), dtype=torch.float32, device=t.device)
    return v.view(t.shape)


class ClipLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, scale, w_row, w_col, cache, group):
        a, b = a.contiguous(), b.contiguous()
        scale = scale.reshape(1).contiguous()
        bl = a.shape[0]
        if group is not None:
            world, rank = dist.get_world_size(group), dist.get_rank(group)
            both = _gather_cat(torch.stack([a, b]), group)                 # [W, 2, Bl, P]
            a_g = both[:, 0].reshape(world * bl, -1)
            b_g = both[:, 1].reshape(world * bl, -1)
        else:
            world, rank, a_g, b_g = 1, 0, a, b
        off = rank * bl
        bg = world * bl
        lse_r, pos_r = _kernels.simce_lse(a, b_g, scale, label_offset=off, cache=cache)
        pos_c = None
        if w_col != 0.0:
            lse_c, pos_c = _kernels.simce_lse(b, a_g, scale, label_offset=off)
        else:
            lse_c = _inf_like(lse_r)                       # exp(s - inf) = 0: the unused direction contributes nothing
        if group is None:                                  # single process: sums, weights and the mean in one launch
            out = _kernels.ce_combine(lse_r, pos_r, lse_c if pos_c is not None else None, pos_c, w_row, w_col, bg)
            ctx.meta = (w_row, w_col, off, bg, cache)
            ctx.save_for_backward(a, b, a_g, b_g, scale, lse_r, lse_c, lse_r, lse_c)
            return out
        local = w_row * (lse_r - pos_r).sum()
        if pos_c is not None:
            local = local + w_col * (lse_c - pos_c).sum()
        if group is not None:
            lses = _gather_cat(torch.stack([lse_r, lse_c]), group)          # [W, 2, Bl]
            lse_r_g = lses[:, 0].reshape(-1).contiguous()
            lse_c_g = lses[:, 1].reshape(-1).contiguous()
            dist.all_reduce(local, group=group)
        else:
            lse_r_g, lse_c_g = lse_r, lse_c
        ctx.meta = (w_row, w_col, off, bg, cache)
        ctx.save_for_backward(a, b, a_g, b_g, scale, lse_r, lse_c, lse_r_g, lse_c_g)
        return local / bg

    @staticmethod
    def backward(ctx, dloss):
        a, b, a_g, b_g, scale, lse_r, lse_c, lse_r_g, lse_c_g = ctx.saved_tensors
        w_row, w_col, off, bg, cache = ctx.meta
        # rows of a: row-direction softmax uses their own LSE, column direction the keys' LSE
        # the incoming gradient (1.0 from loss.backward()) is folded into the kernels' 1 / Bg factor: no `grad * g` launches
        g = dloss.reshape(1).contiguous() if dloss.numel() == 1 else None
        da, dsa = _kernels.simce_grad(a, b_g, scale, lse_r, lse_c_g, w_row, w_col, 1.0 / bg, label_offset=off, cache=cache,
                                      upstream=g)
        # rows of b are the queries of the column direction
        db, _ = _kernels.simce_grad(b, a_g, scale, lse_c, lse_r_g, w_col, w_row, 1.0 / bg, label_offset=off, upstream=g)
        dscale = dsa.sum().reshape(1)          # this rank's rows only; the optimiser sums parameter grads over ranks
        return da, db, dscale, None, None, None, None


class ClassAwareClipLossFn(torch.autograd.Function):
    """ClipLossFn with class ids on the pairs and / or label smoothing (clipk_simce_lse_cls / clipk_simce_grad_cls).
    Multi-GPU: the ids take one more all-gather, the same-class counts travel with the LSE gather ([W, 4, Bl])."""

    @staticmethod
    def forward(ctx, a, b, scale, ids, same_class, eps, w_row, w_col, cache, group):
        a, b = a.contiguous(), b.contiguous()
        cache = None if cache is None else cache.contiguous()
        scale = scale.reshape(1).contiguous()
        bl = a.shape[0]
        if group is not None:
            world, rank = dist.get_world_size(group), dist.get_rank(group)
            both = _gather_cat(torch.stack([a, b]), group)                 # [W, 2, Bl, P]
            a_g = both[:, 0].reshape(world * bl, -1)
            b_g = both[:, 1].reshape(world * bl, -1)
            ids_g = None if ids is None else _gather_cat(ids, group).reshape(-1)
        else:
            world, rank, a_g, b_g, ids_g = 1, 0, a, b, ids
        off = rank * bl
        bg = world * bl
        nc = 0 if cache is None else cache.shape[0]
        kw = dict(cls_x=ids, cls_y=ids_g, same_class=same_class, eps=eps, label_offset=off)
        lse_r, tgt_r, cnt_r = _kernels.simce_lse_cls(a, b_g, scale, cache=cache, **kw)
        if w_col != 0.0:
            lse_c, tgt_c, cnt_c = _kernels.simce_lse_cls(b, a_g, scale, **kw)
        else:
            lse_c, tgt_c, cnt_c = _inf_like(lse_r), None, cnt_r       # the unused direction contributes nothing
        if group is None:
            out = _kernels.ce_combine(lse_r, tgt_r, lse_c if tgt_c is not None else None, tgt_c, w_row, w_col, bg)
            lse_r_g, lse_c_g, cnt_r_g, cnt_c_g = lse_r, lse_c, cnt_r, cnt_c
        else:
            local = w_row * (lse_r - tgt_r).sum()
            if tgt_c is not None:
                local = local + w_col * (lse_c - tgt_c).sum()
            stats = _gather_cat(torch.stack([lse_r, lse_c, cnt_r, cnt_c]), group)    # [W, 4, Bl]
            lse_r_g, lse_c_g, cnt_r_g, cnt_c_g = (stats[:, k].reshape(-1).contiguous() for k in range(4))
            dist.all_reduce(local, group=group)
            out = local / bg
        ctx.meta = (same_class, eps, w_row, w_col, off, bg, nc, cache)
        ctx.save_for_backward(a, b, a_g, b_g, scale, ids, ids_g, lse_r, lse_c, cnt_r, cnt_c, lse_r_g, lse_c_g, cnt_r_g,
                              cnt_c_g)
        return out

    @staticmethod
    def backward(ctx, dloss):
        a, b, a_g, b_g, scale, ids, ids_g, lse_r, lse_c, cnt_r, cnt_c, lse_r_g, lse_c_g, cnt_r_g, cnt_c_g = ctx.saved_tensors
        same_class, eps, w_row, w_col, off, bg, nc, cache = ctx.meta
        g = dloss.reshape(1).contiguous() if dloss.numel() == 1 else None
        kw = dict(cls_x=ids, cls_y=ids_g, same_class=same_class, eps=eps, label_offset=off, upstream=g)
        # rows of a: their own direction has the cache keys, the column direction (rows of b) has the Bg rows of a
        da, dsa = _kernels.simce_grad_cls(a, b_g, scale, lse_r, lse_c_g, cnt_r, cnt_c_g, w_row, w_col, 1.0 / bg, bg,
                                          cache=cache, **kw)
        # rows of b are the queries of the column direction; the keys' (a's) own direction has Bg + Nc keys
        db, _ = _kernels.simce_grad_cls(b, a_g, scale, lse_c, lse_r_g, cnt_c, cnt_r_g, w_col, w_row, 1.0 / bg, bg + nc,
                                        **kw)
        dscale = dsa.sum().reshape(1)
        return da, db, dscale, None, None, None, None, None, None, None


_NULL_COEF = {}


def _null_coef(like: torch.Tensor) -> torch.Tensor:
    """Read-only coefficients (q, k1, k2) = (0, -inf, -inf) of like's shape [3, n], made once per (device, n): the
    one-sided loss's unused direction (exp(... - inf) = 0, as _inf_like for the plain loss)."""
    key = (str(like.device), like.shape[1])
    v = _NULL_COEF.get(key)
    if v is None:
        v = torch.full(tuple(like.shape), float("-inf"), dtype=torch.float32, device=like.device)
        v[0] = 0.0
        _NULL_COEF[key] = v
    return v


class HardNegativeClipLossFn(torch.autograd.Function):
    """ClipLossFn with hard-negative importance weights (clipk_simce_lse_hard / clipk_simce_grad_hard), optionally with
    class ids ("mask": same-class keys leave the negatives first).  Multi-GPU: the ids take one more all-gather, the
    per-row coefficients of both directions travel in the one statistics gather ([W, 6, Bl]) the LSE vectors take in
    ClipLossFn (the gradient pass needs the coefficients only)."""

    @staticmethod
    def forward(ctx, a, b, scale, beta, ids, w_row, w_col, cache, group):
        a, b = a.contiguous(), b.contiguous()
        cache = None if cache is None else cache.contiguous()
        scale = scale.reshape(1).contiguous()
        bl = a.shape[0]
        if group is not None:
            world, rank = dist.get_world_size(group), dist.get_rank(group)
            both = _gather_cat(torch.stack([a, b]), group)                 # [W, 2, Bl, P]
            a_g = both[:, 0].reshape(world * bl, -1)
            b_g = both[:, 1].reshape(world * bl, -1)
            ids_g = None if ids is None else _gather_cat(ids, group).reshape(-1)
        else:
            world, rank, a_g, b_g, ids_g = 1, 0, a, b, ids
        off = rank * bl
        bg = world * bl
        kw = dict(cls_x=ids, cls_y=ids_g, label_offset=off)
        lse_r, pos_r, coef_r = _kernels.simce_lse_hard(a, b_g, scale, beta, cache=cache, **kw)
        if w_col != 0.0:
            lse_c, pos_c, coef_c = _kernels.simce_lse_hard(b, a_g, scale, beta, **kw)
        else:
            lse_c, pos_c, coef_c = None, None, _null_coef(coef_r)     # the unused direction contributes nothing
        if group is None:
            out = _kernels.ce_combine(lse_r, pos_r, lse_c, pos_c, w_row, w_col, bg)
            coef_r_g, coef_c_g = coef_r, coef_c
        else:
            local = w_row * (lse_r - pos_r).sum()
            if pos_c is not None:
                local = local + w_col * (lse_c - pos_c).sum()
            stats = _gather_cat(torch.cat([coef_r, coef_c]), group)                  # [W, 6, Bl]
            coef_r_g = stats[:, :3].permute(1, 0, 2).reshape(3, -1).contiguous()
            coef_c_g = stats[:, 3:].permute(1, 0, 2).reshape(3, -1).contiguous()
            dist.all_reduce(local, group=group)
            out = local / bg
        ctx.meta = (beta, w_row, w_col, off, bg, cache)
        ctx.save_for_backward(a, b, a_g, b_g, scale, ids, ids_g, coef_r, coef_c, coef_r_g, coef_c_g)
        return out

    @staticmethod
    def backward(ctx, dloss):
        a, b, a_g, b_g, scale, ids, ids_g, coef_r, coef_c, coef_r_g, coef_c_g = ctx.saved_tensors
        beta, w_row, w_col, off, bg, cache = ctx.meta
        g = dloss.reshape(1).contiguous() if dloss.numel() == 1 else None
        kw = dict(cls_x=ids, cls_y=ids_g, label_offset=off, upstream=g)
        # rows of a: their own direction has the cache keys; the column direction is the keys' (rows of b) own loss
        da, dsa = _kernels.simce_grad_hard(a, b_g, scale, beta, coef_r, coef_c_g, w_row, w_col, 1.0 / bg, cache=cache, **kw)
        # rows of b are the queries of the column direction
        db, _ = _kernels.simce_grad_hard(b, a_g, scale, beta, coef_c, coef_r_g, w_col, w_row, 1.0 / bg, **kw)
        dscale = dsa.sum().reshape(1)
        return da, db, dscale, None, None, None, None, None, None


SAME_CLASS_MODES = ("mask", "positive")


def _check_class_args(a, b, cache, class_ids, same_class, label_smoothing):
    """Validate the class-aware arguments (ValueError); returns (ids as contiguous int64 or None, eps)."""
    if same_class not in SAME_CLASS_MODES:
        raise ValueError(f"same_class must be one of {SAME_CLASS_MODES}, got {same_class!r}")
    if isinstance(label_smoothing, bool) or not isinstance(label_smoothing, (int, float)):
        raise ValueError(f"label_smoothing must be a number in [0, 1), got {label_smoothing!r}")
    eps = float(label_smoothing)
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1), got {eps}")
    if class_ids is None and eps == 0.0:
        return None, eps
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError(f"embeddings must be two [B, P] tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    for name, t in (("a_embeds", a), ("b_embeds", b), ("cache", cache)):
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"class-aware / label-smoothed InfoNCE takes float32 embeddings, {name} is {t.dtype}")
    P = a.shape[1]
    if cache is not None and (cache.dim() != 2 or cache.shape[1] != P):
        raise ValueError(f"cache must be [Nc, {P}], got {tuple(cache.shape)}")
    if P % 4 or P > 512:
        raise ValueError(f"class-aware / label-smoothed InfoNCE supports P % 4 == 0 and P <= 512, got P = {P}")
    if class_ids is None:
        return None, eps
    if not torch.is_tensor(class_ids):
        raise ValueError(f"class_ids must be a tensor, got {type(class_ids).__name__}")
    if class_ids.dtype.is_floating_point or class_ids.dtype.is_complex or class_ids.dtype == torch.bool:
        raise ValueError(f"class_ids must be an integer tensor, got {class_ids.dtype}")
    if tuple(class_ids.shape) != (a.shape[0],):
        raise ValueError(f"class_ids must have shape ({a.shape[0]},), got {tuple(class_ids.shape)}")
    if class_ids.device != a.device:
        raise ValueError(f"class_ids are on {class_ids.device}, the embeddings on {a.device}")
    return class_ids.to(torch.int64).contiguous(), eps


def _check_hard_args(a, b, cache, same_class, eps, hard_negative_beta) -> float:
    """Validate hard_negative_beta and what it may be combined with (ValueError); returns beta as a float."""
    beta = hard_negative_beta
    if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not 0.0 <= float(beta) < float("inf"):
        raise ValueError(f"hard_negative_beta must be a finite number >= 0, got {beta!r}")
    beta = float(beta)
    if beta == 0.0:
        return beta
    if same_class == "positive":
        raise ValueError('hard_negative_beta > 0 cannot be combined with same_class="positive"')
    if eps > 0.0:
        raise ValueError("hard_negative_beta > 0 cannot be combined with label_smoothing > 0")
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError(f"embeddings must be two [B, P] tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    for name, t in (("a_embeds", a), ("b_embeds", b), ("cache", cache)):
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"hard-negative InfoNCE takes float32 embeddings, {name} is {t.dtype}")
    P = a.shape[1]
    if cache is not None and (cache.dim() != 2 or cache.shape[1] != P):
        raise ValueError(f"cache must be [Nc, {P}], got {tuple(cache.shape)}")
    if P % 4 or P > 512:
        raise ValueError(f"hard-negative InfoNCE supports P % 4 == 0 and P <= 512, got P = {P}")
    return beta


def clip_loss(a_embeds: torch.Tensor, b_embeds: torch.Tensor, logit_scale_exp: torch.Tensor, *,
              symmetric: bool = True, cache: Optional[torch.Tensor] = None, group=None,
              w_row: Optional[float] = None, w_col: Optional[float] = None,
              class_ids: Optional[torch.Tensor] = None, same_class: str = "mask",
              label_smoothing: float = 0.0, hard_negative_beta: float = 0.0) -> torch.Tensor:
    """InfoNCE over L2-normalised embeddings [B_local, P] (f32).  `logit_scale_exp` = exp(logit_scale)
    (already clamped if the model clamps, old/clip_opt.py:100).  With `group`, the batch is the concatenation
    over ranks in rank order and the returned value is the global-batch loss on every rank.

    class_ids: integer [B_local] on the embeddings' device, one id per pair (pairs that share a partner share an id).
    same_class="mask" drops the other same-class keys from each row's softmax; "positive" keeps them and spreads the
    target over them (supervised contrastive).  label_smoothing: eps in [0, 1), torch's convention (eps / N on every
    key of the row's softmax).  Cache rows carry no class.  hard_negative_beta: beta >= 0 of the hard-negative
    importance weights exp(beta S) / mean exp(beta S) on each row's negatives (include/clipk.h: clipk_simce_lse_hard;
    the reference's 'hard_negative' variant, its hard_negative_weight); with class_ids ("mask" only) the same-class keys
    leave the negatives first; not combinable with same_class="positive" or label_smoothing.  Defaults: exactly the
    plain loss and its kernels."""
    ids, eps = _check_class_args(a_embeds, b_embeds, cache, class_ids, same_class, label_smoothing)
    beta = _check_hard_args(a_embeds, b_embeds, cache, same_class, eps, hard_negative_beta)
    if w_row is None:
        w_row, w_col = (0.5, 0.5) if symmetric else (1.0, 0.0)
    if group is None and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        group = dist.group.WORLD
    if group is not None and dist.get_world_size(group) == 1 and not os.environ.get("CLIPK_FORCE_DIST"):
        group = None                         # (CLIPK_FORCE_DIST keeps the collective path for 1-rank RCCL rehearsals)
    if beta > 0.0:
        return HardNegativeClipLossFn.apply(a_embeds, b_embeds, logit_scale_exp, beta, ids, float(w_row), float(w_col),
                                            cache, group)
    if ids is None and eps == 0.0:
        return ClipLossFn.apply(a_embeds, b_embeds, logit_scale_exp, float(w_row), float(w_col), cache, group)
    return ClassAwareClipLossFn.apply(a_embeds, b_embeds, logit_scale_exp, ids, same_class, eps, float(w_row),
                                      float(w_col), cache, group)


def contrastive_loss(x: torch.Tensor, y: torch.Tensor, temperature: float = 0.1, queue: Optional[torch.Tensor] = None,
                     group=None, hard_negative_beta: float = 0.0) -> torch.Tensor:
    """tong/utils/losses.py:4-19: InfoNCE with an optional memory queue — both inputs L2-normalised, the queue rows
    appended to the keys as extra negatives (detached), one-sided CE(x y^T / temperature, arange).  Same fused kernels as
    clip_loss (w_row = 1, w_col = 0, cache = queue): neither the [B, B + Q] logits nor the concatenated keys exist.
    hard_negative_beta > 0: clip_loss's hard-negative weights; the queue rows are negatives like the batch's."""
    from . import functional as KF
    scale = torch.full((1,), 1.0 / float(temperature), dtype=torch.float32, device=x.device)
    # a private copy, as the reference's `queue.clone().detach()`: the queue is overwritten in place by the next
    # enqueue, which may come before this loss's backward
    cache = None if queue is None else queue.detach().to(dtype=torch.float32).clone()
    return clip_loss(KF.l2_normalize(x), KF.l2_normalize(y), scale, symmetric=False, cache=cache, group=group,
                     hard_negative_beta=hard_negative_beta)


_TRI_PAIRS = ((0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1))      # (cell,pert) (pert,cell) (cell,prot) ...


class TriModalLossFn(torch.autograd.Function):
    """The three pairwise symmetric InfoNCE losses of current/tf_clip_codes (1).ipynb:13150-13163 on ONE logit scale:
    six directed similarity + LSE problems in one launch (clipk_simce_lse_pairs), six gradient problems in one more
    (clipk_simce_grad_pairs).  Returns (cell_pert, cell_protein, pert_protein) losses; any combination of upstream
    gradients is honoured."""

    @staticmethod
    def forward(ctx, cell, pert, prot, scale):
        E = torch.stack([cell, pert, prot]).contiguous()                # [3, B, P]
        sc = scale.reshape(1).contiguous()
        lse, pos = _kernels.simce_lse_pairs(E, _TRI_PAIRS, sc)
        per = (lse - pos).mean(1)                                       # six one-directional CE values
        ctx.save_for_backward(E, sc, lse)
        ctx.scale_shape = scale.shape
        return 0.5 * (per[0] + per[1]), 0.5 * (per[2] + per[3]), 0.5 * (per[4] + per[5])

    @staticmethod
    def backward(ctx, g_cp, g_ce, g_pe):
        E, sc, lse = ctx.saved_tensors
        B = E.shape[1]
        dX, dsc = _kernels.simce_grad_pairs(E, _TRI_PAIRS, sc, lse, 0.5, 0.5, 1.0 / B)
        # problem (a, b) holds d L_ab / d E_a complete (both directions): combine per modality — [B, P] adds: plumbing
        dcell = g_cp * dX[0] + g_ce * dX[2]
        dpert = g_cp * dX[1] + g_pe * dX[4]
        dprot = g_ce * dX[3] + g_pe * dX[5]
        dscale = (g_cp * dsc[0].sum() + g_ce * dsc[2].sum() + g_pe * dsc[4].sum()).reshape(ctx.scale_shape)
        return dcell, dpert, dprot, dscale


def tri_modal_loss(cell_embed: torch.Tensor, pert_embed: torch.Tensor, protein_embed: torch.Tensor,
                   logit_scale_exp: torch.Tensor, group=None):
    """Tri-modal contrastive objective of current/tf_clip_codes (1).ipynb:13150-13176: three pairwise symmetric
    InfoNCE losses sharing one logit_scale on the fused similarity + CE kernels (no B x B logits).  Single process:
    one batched launch per pass for all three pairs (TriModalLossFn); with a process group: three global-batch
    clip_loss calls.  Returns the loss entries of the reference's ContrastiveModel.forward dict."""
    if group is None and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        group = dist.group.WORLD
    if group is not None and dist.get_world_size(group) > 1:
        cp = clip_loss(cell_embed, pert_embed, logit_scale_exp, symmetric=True, group=group)
        ce = clip_loss(cell_embed, protein_embed, logit_scale_exp, symmetric=True, group=group)
        pe = clip_loss(pert_embed, protein_embed, logit_scale_exp, symmetric=True, group=group)
    else:
        cp, ce, pe = TriModalLossFn.apply(cell_embed.contiguous(), pert_embed.contiguous(), protein_embed.contiguous(),
                                          logit_scale_exp)
    return {"loss": cp + ce + pe, "cell_pert_loss": cp, "cell_protein_loss": ce, "pert_protein_loss": pe}
