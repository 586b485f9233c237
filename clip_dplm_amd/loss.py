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
from typing import Callable, NamedTuple, Optional

import torch
import torch.distributed as dist

from . import ops
from ._ffi import ClipkError

# kernel namespace; tests of the rank bookkeeping (gloo, CPU) substitute a torch restatement here — the product
# itself never does: ops.* raise on anything but device tensors.
_kernels = ops


def _gather_cat(t: torch.Tensor, group) -> torch.Tensor:
    world = dist.get_world_size(group)
    t = t.contiguous()
    out = torch.empty((world * t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    dist.all_gather_into_tensor(out, t, group=group)          # concatenation along dim 0 (works on nccl and gloo)
    return out.view((world,) + tuple(t.shape))


_CONST = {}


def _const_like(t: torch.Tensor, fill: float, row0: Optional[float] = None) -> torch.Tensor:
    """A read-only f32 tensor of t's shape filled with `fill` (row 0 with `row0` where given), made once per (device,
    shape, values): the statistic of the one-sided loss's unused direction."""
    key = (str(t.device), tuple(t.shape), fill, row0)
    v = _CONST.get(key)
    if v is None:
        v = _CONST[key] = torch.full(tuple(t.shape), fill, dtype=torch.float32, device=t.device)
        if row0 is not None:
            v[0] = row0
    return v


class _Variant(NamedTuple):
    """What tells one InfoNCE variant from another inside InfoNCEFn.  `stat` is the tuple of per-row tensors (last
    dimension: the rows) that travel from the LSE pass to the gradient pass, of one direction.
      lse(x, keys, scale, off, cache, ids_x, ids_keys) -> (lse, tgt, stat)
      null(stat_r) -> stat of the unused direction of the one-sided loss (it contributes nothing)
      grad(x, keys, scale, stat_x, stat_keys, w_x, w_keys, inv_bg, nkeys, off, cache, ids_x, ids_keys, upstream)
          -> (dx, dscale partials); nkeys: the key count of the keys' own direction."""
    lse: Callable
    null: Callable
    grad: Callable


def _plain_lse(x, keys, scale, off, cache, ids_x, ids_keys):
    lse, pos = _kernels.simce_lse(x, keys, scale, label_offset=off, cache=cache)
    return lse, pos, (lse,)


_PLAIN = _Variant(
    lse=_plain_lse,
    null=lambda stat: (_const_like(stat[0], float("inf")),),              # exp(s - inf) = 0
    grad=lambda x, keys, scale, sx, sk, w_x, w_keys, inv_bg, nkeys, off, cache, ids_x, ids_keys, g:
        _kernels.simce_grad(x, keys, scale, sx[0], sk[0], w_x, w_keys, inv_bg, label_offset=off, cache=cache, upstream=g))


def _class_aware(same_class: str, eps: float) -> _Variant:
    """Class ids on the pairs and / or label smoothing (clipk_simce_lse_cls / clipk_simce_grad_cls): stat = (lse, cnt),
    the same-class counts travel with the LSE vectors."""
    def lse(x, keys, scale, off, cache, ids_x, ids_keys):
        lse, tgt, cnt = _kernels.simce_lse_cls(x, keys, scale, cache=cache, cls_x=ids_x, cls_y=ids_keys,
                                               same_class=same_class, eps=eps, label_offset=off)
        return lse, tgt, (lse, cnt)

    def grad(x, keys, scale, sx, sk, w_x, w_keys, inv_bg, nkeys, off, cache, ids_x, ids_keys, g):
        return _kernels.simce_grad_cls(x, keys, scale, sx[0], sk[0], sx[1], sk[1], w_x, w_keys, inv_bg, nkeys, cache=cache,
                                       cls_x=ids_x, cls_y=ids_keys, same_class=same_class, eps=eps, label_offset=off,
                                       upstream=g)
    return _Variant(lse, lambda stat: (_const_like(stat[0], float("inf")), stat[1]), grad)


def _hard_negative(beta: float) -> _Variant:
    """Hard-negative importance weights (clipk_simce_lse_hard / clipk_simce_grad_hard), optionally with class ids
    ("mask": same-class keys leave the negatives first): stat = (coef [3, rows],), the gradient pass needs the per-row
    coefficients (q, k1, k2) only; (0, -inf, -inf) contribute nothing."""
    def lse(x, keys, scale, off, cache, ids_x, ids_keys):
        lse, pos, coef = _kernels.simce_lse_hard(x, keys, scale, beta, cache=cache, cls_x=ids_x, cls_y=ids_keys,
                                                 label_offset=off)
        return lse, pos, (coef,)

    def grad(x, keys, scale, sx, sk, w_x, w_keys, inv_bg, nkeys, off, cache, ids_x, ids_keys, g):
        return _kernels.simce_grad_hard(x, keys, scale, beta, sx[0], sk[0], w_x, w_keys, inv_bg, cache=cache, cls_x=ids_x,
                                        cls_y=ids_keys, label_offset=off, upstream=g)
    return _Variant(lse, lambda stat: (_const_like(stat[0], float("-inf"), 0.0),), grad)


class InfoNCEFn(torch.autograd.Function):
    """The fused InfoNCE of every variant (_Variant): two directed LSE passes, the loss, two gradient passes with the
    roles of the two sides swapped.  Multi-GPU: one all-gather of the embeddings [W, 2, Bl, P], one of the class ids
    where there are any, one of both directions' statistics ([W, 2, Bl] plain, [W, 4, Bl] class-aware, [W, 6, Bl]
    hard-negative) and one all-reduce of the local sum."""

    @staticmethod
    def forward(ctx, a, b, scale, variant, ids, w_row, w_col, cache, group):
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
        lse_r, tgt_r, stat_r = variant.lse(a, b_g, scale, off, cache, ids, ids_g)
        if w_col != 0.0:
            lse_c, tgt_c, stat_c = variant.lse(b, a_g, scale, off, None, ids, ids_g)
        else:
            lse_c, tgt_c, stat_c = None, None, variant.null(stat_r)
        if group is None:                                  # single process: sums, weights and the mean in one launch
            out = _kernels.ce_combine(lse_r, tgt_r, lse_c, tgt_c, w_row, w_col, bg)
            stat_r_g, stat_c_g = stat_r, stat_c
        else:
            local = w_row * (lse_r - tgt_r).sum()
            if tgt_c is not None:
                local = local + w_col * (lse_c - tgt_c).sum()
            # one gather of both directions' rows, [W, K, Bl], laid out back to each tensor's [..., W * Bl]
            each = [t for pair in zip(stat_r, stat_c) for t in pair]
            stats = _gather_cat(torch.cat([t.reshape(-1, bl) for t in each]), group)
            stats = [g.permute(1, 0, 2).reshape(t.shape[:-1] + (bg,)).contiguous()
                     for g, t in zip(stats.split([t.numel() // bl for t in each], dim=1), each)]
            stat_r_g, stat_c_g = tuple(stats[0::2]), tuple(stats[1::2])
            dist.all_reduce(local, group=group)
            out = local / bg
        ctx.meta = (variant, w_row, w_col, off, bg, cache)
        ctx.save_for_backward(a, b, a_g, b_g, scale, ids, ids_g, *stat_r, *stat_c, *stat_r_g, *stat_c_g)
        return out

    @staticmethod
    def backward(ctx, dloss):
        a, b, a_g, b_g, scale, ids, ids_g, *stats = ctx.saved_tensors
        variant, w_row, w_col, off, bg, cache = ctx.meta
        n = len(stats) // 4
        stat_r, stat_c, stat_r_g, stat_c_g = (stats[k * n:(k + 1) * n] for k in range(4))
        nc = 0 if cache is None else cache.shape[0]
        # the incoming gradient (1.0 from loss.backward()) is folded into the kernels' 1 / Bg factor: no `grad * g` launches
        g = dloss.reshape(1).contiguous() if dloss.numel() == 1 else None
        # rows of a: their own direction has the cache keys; the column direction (rows of b) has the Bg rows of a
        da, dsa = variant.grad(a, b_g, scale, stat_r, stat_c_g, w_row, w_col, 1.0 / bg, bg, off, cache, ids, ids_g, g)
        # rows of b are the queries of the column direction; the keys' (a's) own direction has Bg + Nc keys
        db, _ = variant.grad(b, a_g, scale, stat_c, stat_r_g, w_col, w_row, 1.0 / bg, bg + nc, off, None, ids, ids_g, g)
        dscale = dsa.sum().reshape(1)          # this rank's rows only; the optimiser sums parameter grads over ranks
        return da, db, dscale, None, None, None, None, None, None


SAME_CLASS_MODES = ("mask", "positive")


def _check_embeddings(a, b, cache, what: str) -> None:
    """Shapes, dtypes and P of the embeddings and the cache for the class-aware and hard-negative kernels (ValueError)."""
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError(f"embeddings must be two [B, P] tensors of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    for name, t in (("a_embeds", a), ("b_embeds", b), ("cache", cache)):
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"{what} takes float32 embeddings, {name} is {t.dtype}")
    P = a.shape[1]
    if cache is not None and (cache.dim() != 2 or cache.shape[1] != P):
        raise ValueError(f"cache must be [Nc, {P}], got {tuple(cache.shape)}")
    if P % 4 or P > 512:
        raise ValueError(f"{what} supports P % 4 == 0 and P <= 512, got P = {P}")


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
    _check_embeddings(a, b, cache, "class-aware / label-smoothed InfoNCE")
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
    _check_embeddings(a, b, cache, "hard-negative InfoNCE")
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
        variant = _hard_negative(beta)
    elif ids is None and eps == 0.0:
        variant = _PLAIN
    else:
        variant = _class_aware(same_class, eps)
    return InfoNCEFn.apply(a_embeds, b_embeds, logit_scale_exp, variant, ids, float(w_row), float(w_col), cache, group)


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


class _TriVariant(NamedTuple):
    """What tells one variant of the batched tri-modal loss from another inside TriModalLossFn (the _Variant of the six
    directed problems of _TRI_PAIRS).  `stat`: the tensors [6, ...] that travel from the LSE pass to the gradient pass.
      lse(E, scale, ids6) -> (lse, tgt, stat)
      grad(E, scale, stat, inv_b, ids6, upstream) -> (dX [6, B, P], dscale partials [6, B]); upstream: f32 [6], the
          incoming gradient of each problem's loss
      folds: grad multiplies upstream in, inside the kernel; else the caller does, on [B, P]."""
    lse: Callable
    grad: Callable
    folds: bool


def _tri_plain_lse(E, scale, ids6):
    lse, pos = _kernels.simce_lse_pairs(E, _TRI_PAIRS, scale)
    return lse, pos, (lse,)


def _tri_plain_slice_ok(P: int) -> bool:
    """clipk_simce_grad_pairs's rule (csrc/simce.hip: make_plan): its gradient pass walks each wave's slice of P - P
    over 1, 2, 4 or 8 waves of at most 128 columns, rounded up to 8 - in blocks of 32 columns.
    tests/test_simce_ref_host.py holds this to the restatement of make_plan in tests/simce_ref.py."""
    nw = 1
    while nw < 8 and -(-P // nw) > 128:
        nw *= 2
    return ((-(-P // nw) + 7) & ~7) % 32 == 0


def _tri_plain_grad(E, scale, stat, inv_b, ids6, g):
    """clipk_simce_grad_pairs; at a width it refuses (P = 36, 48, 160, ...) up to 512 the batched class-aware gradient
    pass without ids and smoothing, from the same LSE vectors and with every same-class count 1: the same gradient, as
    clipk_simce_grad_scaled sends such P to the tiled pass.  (Above 512 the entry's own refusal stands.)"""
    P = E.shape[-1]
    if _tri_plain_slice_ok(P) or P > 512:
        return _kernels.simce_grad_pairs(E, _TRI_PAIRS, scale, stat[0], 0.5, 0.5, inv_b)
    return _kernels.simce_grad_pairs_cls(E, _TRI_PAIRS, scale, stat[0], torch.ones_like(stat[0]), 0.5, 0.5, inv_b)


_TRI_PLAIN = _TriVariant(lse=_tri_plain_lse, grad=_tri_plain_grad, folds=False)


def _tri_class_aware(same_class: str, eps: float) -> _TriVariant:
    """clipk_simce_{lse,grad}_pairs_cls: stat = (lse, cnt)."""
    def lse(E, scale, ids6):
        lse, tgt, cnt = _kernels.simce_lse_pairs_cls(E, _TRI_PAIRS, scale, ids=ids6, same_class=same_class, eps=eps)
        return lse, tgt, (lse, cnt)

    def grad(E, scale, stat, inv_b, ids6, g):
        return _kernels.simce_grad_pairs_cls(E, _TRI_PAIRS, scale, stat[0], stat[1], 0.5, 0.5, inv_b, ids=ids6,
                                             same_class=same_class, eps=eps, upstream=g)
    return _TriVariant(lse, grad, True)


def _tri_hard_negative(beta: float) -> _TriVariant:
    """clipk_simce_{lse,grad}_pairs_hard: stat = (coef [6, 3, B],)."""
    def lse(E, scale, ids6):
        lse, pos, coef = _kernels.simce_lse_pairs_hard(E, _TRI_PAIRS, scale, beta, ids=ids6)
        return lse, pos, (coef,)

    def grad(E, scale, stat, inv_b, ids6, g):
        return _kernels.simce_grad_pairs_hard(E, _TRI_PAIRS, scale, beta, stat[0], 0.5, 0.5, inv_b, ids=ids6, upstream=g)
    return _TriVariant(lse, grad, True)


class TriModalLossFn(torch.autograd.Function):
    """The three pairwise symmetric InfoNCE losses of current/tf_clip_codes (1).ipynb:13150-13163 on ONE logit scale, of
    every variant (_TriVariant): six directed similarity + LSE problems in one launch (clipk_simce_lse_pairs[_cls|_hard]),
    six gradient problems in one more (clipk_simce_grad_pairs[...]).  ids: the id vectors of (cell, pert), (cell, protein)
    and (pert, protein), each int64 [B] or None (all distinct).  Returns (cell_pert, cell_protein, pert_protein) losses;
    any combination of upstream gradients is honoured."""

    @staticmethod
    def forward(ctx, cell, pert, prot, scale, variant=_TRI_PLAIN, ids_cp=None, ids_ce=None, ids_pe=None):
        E = torch.stack([cell, pert, prot]).contiguous()                # [3, B, P]
        sc = scale.reshape(1).contiguous()
        lse, tgt, stat = variant.lse(E, sc, (ids_cp, ids_cp, ids_ce, ids_ce, ids_pe, ids_pe))
        per = (lse - tgt).mean(1)                                       # six one-directional CE values
        ctx.save_for_backward(E, sc, ids_cp, ids_ce, ids_pe, *stat)
        ctx.scale_shape = scale.shape
        ctx.variant = variant
        return 0.5 * (per[0] + per[1]), 0.5 * (per[2] + per[3]), 0.5 * (per[4] + per[5])

    @staticmethod
    def backward(ctx, g_cp, g_ce, g_pe):
        E, sc, ids_cp, ids_ce, ids_pe, *stat = ctx.saved_tensors
        variant = ctx.variant
        B = E.shape[1]
        ids6 = (ids_cp, ids_cp, ids_ce, ids_ce, ids_pe, ids_pe)
        # problem (a, b) holds d L_ab / d E_a complete (both directions): combine per modality — [B, P] adds: plumbing
        if variant.folds:                       # the three incoming gradients go into the kernel, one per problem
            g = torch.stack([g_cp, g_cp, g_ce, g_ce, g_pe, g_pe]).to(torch.float32)
            dX, dsc = variant.grad(E, sc, stat, 1.0 / B, ids6, g)
            dcell, dpert, dprot = dX[0] + dX[2], dX[1] + dX[4], dX[3] + dX[5]
            dscale = dsc[0::2].sum().reshape(ctx.scale_shape)
        else:
            dX, dsc = variant.grad(E, sc, stat, 1.0 / B, ids6, None)
            dcell = g_cp * dX[0] + g_ce * dX[2]
            dpert = g_cp * dX[1] + g_pe * dX[4]
            dprot = g_ce * dX[3] + g_pe * dX[5]
            dscale = (g_cp * dsc[0].sum() + g_ce * dsc[2].sum() + g_pe * dsc[4].sum()).reshape(ctx.scale_shape)
        return dcell, dpert, dprot, dscale, None, None, None, None


TRI_PAIR_KEYS = ("cell_pert", "cell_protein", "pert_protein")


def _tri_class_ids(class_ids) -> tuple:
    """class_ids of tri_modal_loss -> the three pairs' ids in the order of TRI_PAIR_KEYS (ValueError on an unknown key)."""
    if class_ids is None or torch.is_tensor(class_ids):
        if torch.is_tensor(class_ids) and class_ids.dtype in (torch.int32, torch.int16, torch.int8, torch.uint8):
            class_ids = class_ids.to(torch.int64)              # once for the three pairs, not once per pair
        return (class_ids,) * 3
    if not hasattr(class_ids, "keys"):
        raise ValueError(f"class_ids must be a tensor or a mapping with keys among {TRI_PAIR_KEYS}, got "
                         f"{type(class_ids).__name__}")
    unknown = [k for k in class_ids.keys() if k not in TRI_PAIR_KEYS]
    if unknown:
        raise ValueError(f"class_ids has keys {unknown}; the pairs are {TRI_PAIR_KEYS}")
    return tuple(class_ids.get(k) for k in TRI_PAIR_KEYS)


def tri_modal_loss(cell_embed: torch.Tensor, pert_embed: torch.Tensor, protein_embed: torch.Tensor,
                   logit_scale_exp: torch.Tensor, group=None, *, class_ids=None, same_class: str = "mask",
                   label_smoothing: float = 0.0, hard_negative_beta: float = 0.0):
    """Tri-modal contrastive objective of current/tf_clip_codes (1).ipynb:13150-13176: three pairwise symmetric
    InfoNCE losses sharing one logit_scale on the fused similarity + CE kernels (no B x B logits).  Single process:
    one batched launch per pass for all three pairs (TriModalLossFn); with a process group: three global-batch
    clip_loss calls.  Returns the loss entries of the reference's ContrastiveModel.forward dict.

    class_ids, same_class, label_smoothing, hard_negative_beta: clip_loss's, applied to every pair.  class_ids is one
    integer tensor [B] used for all three pairs (a PerturbAtlas batch, whose perturbation and protein rows repeat, one
    per cell: class_ids=pert_id), or a mapping with keys among "cell_pert", "cell_protein", "pert_protein"; a pair
    without ids is all distinct.  Defaults: exactly the plain loss and its kernels, at every P % 4 == 0 up to 512
    (at a width the plain batched gradient pass does not take, P = 36, 48, 160, ..., the backward runs the class-aware
    gradient pass without ids: the same gradient); above 512 ClipkError unless the slice of P per wave, there P / 8
    rounded up to 8, is a multiple of 32 (768)."""
    pairs = ((cell_embed, pert_embed), (cell_embed, protein_embed), (pert_embed, protein_embed))
    ids = []
    for (a, b), t in zip(pairs, _tri_class_ids(class_ids)):
        t, eps = _check_class_args(a, b, None, t, same_class, label_smoothing)
        ids.append(t)
    for a, b in pairs[:2]:                                 # (they cover the three embeddings)
        beta = _check_hard_args(a, b, None, same_class, eps, hard_negative_beta)
    if group is None and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        group = dist.group.WORLD
    if group is not None and dist.get_world_size(group) > 1:
        kw = dict(symmetric=True, group=group, same_class=same_class, label_smoothing=label_smoothing,
                  hard_negative_beta=hard_negative_beta)
        cp, ce, pe = (clip_loss(a, b, logit_scale_exp, class_ids=t, **kw) for (a, b), t in zip(pairs, ids))
    else:
        args = (cell_embed.contiguous(), pert_embed.contiguous(), protein_embed.contiguous(), logit_scale_exp)
        if beta > 0.0:
            cp, ce, pe = TriModalLossFn.apply(*args, _tri_hard_negative(beta), *ids)
        elif eps > 0.0 or any(t is not None for t in ids):
            cp, ce, pe = TriModalLossFn.apply(*args, _tri_class_aware(same_class, eps), *ids)
        elif cell_embed.shape[-1] <= 512 or cell_embed.shape[-1] % 4 or _tri_plain_slice_ok(cell_embed.shape[-1]):
            cp, ce, pe = TriModalLossFn.apply(*args)
        else:                                              # no gradient pass takes it: say so before the forward pass
            raise ClipkError(f"tri_modal_loss: unsupported projection width P = {cell_embed.shape[-1]}: above 512 the "
                             f"gradient pass needs a slice of P per wave that is a multiple of 32, as P = 768 gives")
    return {"loss": cp + ce + pe, "cell_pert_loss": cp, "cell_protein_loss": ce, "pert_protein_loss": pe}
