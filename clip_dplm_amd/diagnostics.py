"""Embedding-space diagnostics of trained dual encoders without the similarity matrix.

The reference's evaluation code answers every question beyond "where does the positive rank" from the materialised
N x N matrix: `evaluate` returns cosine_sims (run1/full.py:142-160, reduced with .mean() at :253-254),
`track_training_dynamics` wants per-epoch similarity statistics (:401-414), `analyze_failure_cases` the wrong argmax
and its softmax confidence (:415-430), `analyze_hard_negatives_impact` how close the best negative comes (:449-461),
the confusion matrix and confusion rates come from the row argmax (:257-268, :297-306).  Here one fused pass
(include/clipk.h: clipk_sim_stats, `ops.sim_stats`) keeps the row statistics and the histogram of S = scale * a . b^T
while walking gallery tiles; S is never written.  Everything below reduces those per-row tensors.

With `class_ids` the statistics follow the `same_class="mask"` rule of the class-aware loss: keys of the query's class
other than its positive are neither negatives nor part of the softmax.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, Dict, Iterable, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import ops
from .retrieval import _as_f32, _as_ids, default_embed_fn


def _f64(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy().astype(np.float64)


@dataclasses.dataclass
class SimilarityStats:
    """The tensors of `ops.sim_stats` for queries a against gallery b, plus the labels and the histogram range.
    Per query [M]: pos, best, best_idx, hard, hard_idx, lse, neg_sum (f64), neg_sumsq (f64); hist_neg / hist_pos
    int64 [bins + 2] (slot 0: below range[0], slot bins + 1: at or above range[1]); n_keys: rows of b."""
    labels: torch.Tensor
    pos: torch.Tensor
    best: torch.Tensor
    best_idx: torch.Tensor
    hard: torch.Tensor
    hard_idx: torch.Tensor
    lse: torch.Tensor
    neg_sum: torch.Tensor
    neg_sumsq: torch.Tensor
    hist_neg: torch.Tensor
    hist_pos: torch.Tensor
    range: Tuple[float, float]
    scale: float
    n_keys: int

    @property
    def correct(self) -> torch.Tensor:
        """best_idx == label: the reference's logits.argmax(dim=1) == labels."""
        return self.best_idx == self.labels

    @property
    def confidence(self) -> torch.Tensor:
        """exp(best - lse): logits[i].softmax(0)[p] of the predicted key (run1/full.py:424)."""
        return torch.exp(self.best - self.lse)

    @property
    def p_pos(self) -> torch.Tensor:
        """exp(pos - lse): the softmax probability of the positive."""
        return torch.exp(self.pos - self.lse)

    @property
    def margin(self) -> torch.Tensor:
        """pos - hard: how far the positive clears the best negative (negative: a violation)."""
        return self.pos - self.hard

    @property
    def bins(self) -> int:
        return int(self.hist_neg.numel()) - 2

    @property
    def bin_edges(self) -> torch.Tensor:
        """f64 [bins + 1]: slot 1 + b of the histograms covers [edges[b], edges[b + 1]) up to the f32 binning rule."""
        lo, hi = self.range
        return torch.linspace(lo, hi, self.bins + 1, dtype=torch.float64)

    def summary(self) -> Dict[str, float]:
        """Python floats, reduced in f64 on the host.  neg_mean / neg_std come from the f64 sums and the exact
        negative count (the histogram's total); confidence_on_failures is NaN without failures."""
        pos, hard = _f64(self.pos), _f64(self.hard)
        ok = ~np.isnan(pos)
        if not ok.any():
            raise ValueError("no row with a label inside the gallery")
        correct = self.correct.detach().cpu().numpy()[ok]
        conf, ppos = _f64(self.confidence)[ok], _f64(self.p_pos)[ok]
        pos, hard = pos[ok], hard[ok]
        n_neg = int(self.hist_neg.sum())
        s1, s2 = float(_f64(self.neg_sum).sum()), float(_f64(self.neg_sumsq).sum())
        neg_mean = s1 / n_neg if n_neg else float("nan")
        neg_var = max(s2 / n_neg - neg_mean * neg_mean, 0.0) if n_neg else float("nan")
        has_neg = np.isfinite(hard)
        margin = (pos - hard)[has_neg]
        outside = int(self.hist_neg[0] + self.hist_neg[-1] + self.hist_pos[0] + self.hist_pos[-1])
        return {
            "n": int(ok.sum()),
            "top1": float(np.mean(correct)),
            "pos_mean": float(np.mean(pos)),
            "pos_std": float(np.std(pos)),
            "neg_mean": neg_mean,
            "neg_std": float(np.sqrt(neg_var)),
            "margin_mean": float(np.mean(margin)) if margin.size else float("nan"),
            "margin_min": float(np.min(margin)) if margin.size else float("nan"),
            "violations": float(np.mean(hard[has_neg] >= pos[has_neg])) if margin.size else float("nan"),
            "confidence_mean": float(np.mean(conf)),
            "confidence_on_failures": float(np.mean(conf[~correct])) if (~correct).any() else float("nan"),
            "p_pos_mean": float(np.mean(ppos)),
            "out_of_range": outside / float(n_neg + int(self.hist_pos.sum())),
        }


def _class_id_pair(class_ids, na: int, nb: int, labels, device):
    """(ids_a [na], ids_b [nb]) from one id tensor for pairs (one per row of b; a row of a has its positive's id) or a
    pair (ids_a, ids_b)."""
    if class_ids is None:
        return None, None
    if isinstance(class_ids, (tuple, list)):
        if len(class_ids) != 2 or class_ids[0] is None or class_ids[1] is None:
            raise ValueError("class_ids must be one id tensor or a pair (ids_a, ids_b), ids on both sides")
        return _as_ids(class_ids[0], na, device, "class_ids[0]"), _as_ids(class_ids[1], nb, device, "class_ids[1]")
    ids_b = _as_ids(class_ids, nb, device, "class_ids")
    if labels is None:
        if na != nb:
            raise ValueError(f"one id tensor for pairs needs equal counts, got {na} and {nb}")
        return ids_b, ids_b
    return ids_b[labels.clamp(0, nb - 1)].contiguous(), ids_b


def similarity_stats(a: torch.Tensor, b: torch.Tensor, *, scale: float = 1.0, labels: Optional[torch.Tensor] = None,
                     class_ids=None, bins: int = 64,
                     range: Optional[Tuple[float, float]] = None) -> SimilarityStats:  # noqa: A002 (numpy's name)
    """Statistics of S = scale * a . b^T: a_i's positive is b[labels[i]] (b_i when labels is None).

    class_ids: one id tensor for pairs (as `retrieval.ranks`) or a pair (ids_a, ids_b).  range defaults to
    (-|scale|, |scale|), right for unit-norm rows; scores outside land in the two outer histogram slots and are
    reported by summary()["out_of_range"], not dropped."""
    bins = int(bins)
    if not 1 <= bins <= 256:
        raise ValueError(f"bins must be in [1, 256], got {bins}")
    sc = float(scale)
    lo, hi = (-abs(sc), abs(sc)) if range is None else (float(range[0]), float(range[1]))
    if not lo < hi:
        raise ValueError(f"need range[0] < range[1], got ({lo}, {hi})")
    qa, gb = _as_f32(a, "a"), _as_f32(b, "b")
    if qa.device != gb.device:
        raise ValueError(f"a on {qa.device} but b on {gb.device}")
    na, nb = qa.shape[0], gb.shape[0]
    if labels is not None:
        labels = labels.to(device=qa.device, dtype=torch.int64).reshape(-1).contiguous()
        if labels.numel() != na:
            raise ValueError(f"labels must hold {na} indices, got {labels.numel()}")
    elif na > nb:
        raise ValueError(f"paired embeddings need a positive per row of a, got {na} and {nb} rows")
    ids_a, ids_b = _class_id_pair(class_ids, na, nb, labels, qa.device)
    st = ops.sim_stats(qa, gb, scale=sc, labels=labels, cls_x=ids_a, cls_y=ids_b, nbins=bins, lo=lo, hi=hi)
    lab = labels if labels is not None else torch.arange(na, device=qa.device)
    return SimilarityStats(lab, *st, range=(lo, hi), scale=sc, n_keys=nb)


def failures(stats: SimilarityStats):
    """(rows int64 [F], predicted int64 [F], confidence f32 [F]) of the rows whose argmax is not their label:
    analyze_failure_cases (run1/full.py:415-430)."""
    rows = torch.nonzero(~stats.correct).flatten()
    return rows, stats.best_idx[rows], stats.confidence[rows]


def _groups(t, n: int, device, name: str) -> torch.Tensor:
    g = _as_ids(t, n, device, name)
    if n and int(g.min()) < 0:
        raise ValueError(f"{name} must be non-negative group indices")
    return g


def confusion_matrix(stats: SimilarityStats, groups_a, groups_b=None, num_groups: Optional[int] = None) -> torch.Tensor:
    """int64 [G, G]: rows = group of the query, columns = group of its predicted key best_idx (run1/full.py:257-268,
    per group).  groups_a [M], groups_b [n_keys] (None: groups_a, paired sets).  Rows without a prediction are skipped."""
    dev = stats.best_idx.device
    ga = _groups(groups_a, stats.best_idx.numel(), dev, "groups_a")
    gb = ga if groups_b is None else _groups(groups_b, stats.n_keys, dev, "groups_b")
    if gb.numel() != stats.n_keys:
        raise ValueError(f"groups_b must hold {stats.n_keys} indices, got {gb.numel()}")
    G = int(num_groups) if num_groups is not None else int(max(ga.max(), gb.max())) + 1
    if int(max(ga.max(), gb.max())) >= G:
        raise ValueError(f"group index outside [0, {G})")
    ok = stats.best_idx >= 0
    flat = ga[ok] * G + gb[stats.best_idx[ok]]
    return torch.bincount(flat, minlength=G * G).reshape(G, G)


def confusion_rates(conf: torch.Tensor, pairs: Sequence[Tuple[int, int]]) -> Dict[Tuple[int, int], float]:
    """{(g, h): conf[g, h] / conf[g].sum()} for the asked pairs (run1/full.py:297-306); NaN for an empty row."""
    c = conf.detach().cpu().numpy().astype(np.float64)
    tot = c.sum(1)
    return {(int(g), int(h)): (float(c[g, h] / tot[g]) if tot[g] > 0 else float("nan")) for g, h in pairs}


def _uniformity_from(st: SimilarityStats, t: float) -> float:
    """Uniformity from a self-similarity pass at scale 2 t with the diagonal as label."""
    n = st.pos.numel()
    lse, pos = _f64(st.lse), _f64(st.pos)
    row = lse + np.log(-np.expm1(np.minimum(pos - lse, 0.0)))            # log(exp(lse) - exp(pos))
    m = row.max()
    return float(m + np.log(np.exp(row - m).sum()) - 2.0 * float(t) - np.log(float(n) * (n - 1)))


def uniformity(a: torch.Tensor, t: float = 2.0) -> float:
    """log mean_{i != j} exp(-t |a_i - a_j|^2), Wang and Isola's uniformity, for unit-norm rows: there
    -t |a_i - a_j|^2 = 2 t <a_i, a_j> - 2 t, so the row sums are the lse of one self-similarity pass at scale 2 t with
    the diagonal as label, minus the diagonal term; the rows are joined by a log-sum-exp in f64."""
    if a.shape[0] < 2:
        raise ValueError("uniformity needs at least two rows")
    return _uniformity_from(similarity_stats(a, a, scale=2.0 * float(t), bins=1), t)


def alignment(a: torch.Tensor, b: torch.Tensor) -> float:
    """mean |a_i - b_i|^2 of paired unit-norm rows = 2 - 2 mean <a_i, b_i>."""
    return 2.0 - 2.0 * float(_f64(similarity_stats(a, b, scale=1.0, bins=1).pos).mean())


def _group_means(x: torch.Tensor, groups: torch.Tensor, G: int) -> torch.Tensor:
    """f32 [G, P] means of the normalised rows per group, summed in f64 by a one-hot product (deterministic)."""
    xn, _ = ops.l2norm_fwd(x)
    onehot = torch.zeros((G, x.shape[0]), dtype=torch.float64, device=x.device)
    onehot[groups, torch.arange(x.shape[0], device=x.device)] = 1.0
    cnt = onehot.sum(1, keepdim=True)
    return ((onehot @ xn.double()) / cnt).float().contiguous()           # an empty group: NaN row


def group_similarity(a: torch.Tensor, groups_a, b: Optional[torch.Tensor] = None, groups_b=None,
                     num_groups: Optional[int] = None) -> torch.Tensor:
    """f32 [G, G]: mean cosine similarity between the rows of group g of a and group h of b (b = None: a itself; the
    diagonal is then analyze_embedding_collapse's per-group number, run1/full.py:307-315, self pairs included as
    there).  No pass over the similarity matrix: the mean of <a_i, b_j> over a group pair is the dot product of the two
    group means, so the rows are normalised (ops.l2norm_fwd), the [G, P] group means are formed in f64 and
    ops.sim_logits multiplies them.  Empty groups give NaN."""
    xa = _as_f32(a, "a")
    ga = _groups(groups_a, xa.shape[0], xa.device, "groups_a")
    if b is None:
        xb, gb = xa, (ga if groups_b is None else _groups(groups_b, xa.shape[0], xa.device, "groups_b"))
    else:
        xb = _as_f32(b, "b")
        if groups_b is None:
            raise ValueError("groups_b is needed with b")
        gb = _groups(groups_b, xb.shape[0], xa.device, "groups_b")
    if xa.shape[1] != xb.shape[1]:
        raise ValueError(f"a has {xa.shape[1]} columns, b {xb.shape[1]}")
    ops._need_cuda(xa, xb)
    G = int(num_groups) if num_groups is not None else int(max(ga.max(), gb.max())) + 1
    if int(max(ga.max(), gb.max())) >= G:
        raise ValueError(f"group index outside [0, {G})")
    ma = _group_means(xa, ga, G)
    mb = ma if (b is None and groups_b is None) else _group_means(xb, gb, G)
    return ops.sim_logits(ma, mb, torch.ones(1, dtype=torch.float32, device=xa.device))


def _model_scale(model) -> float:
    """exp(logit_scale) of the first submodule that has one, clamped where the model clamps it; else 1."""
    from .modeling_clip import OptimizedCLIPModule
    for m in model.modules():
        ls = getattr(m, "logit_scale", None)
        if torch.is_tensor(ls):
            s = ls.detach().float().exp()
            if isinstance(m, OptimizedCLIPModule):
                s = s.clamp(max=100)
            return float(s)
    return 1.0


@torch.no_grad()
def evaluate_embeddings(model, loader: Iterable, *, embed_fn: Optional[Callable] = None,
                        class_ids_fn: Optional[Callable] = None, scale: Optional[float] = None, bins: int = 64,
                        device=None) -> Dict[str, Union[float, Dict[str, float]]]:
    """The embedding statistics of a paired loader (a_i belongs with b_i), every embedding against the whole set: the
    `embedding_stats` entry of track_training_dynamics (run1/full.py:401-414).

    {"a_to_b": summary, "b_to_a": summary, "a": {"uniformity", "self_neg_mean"}, "b": {...}, "alignment",
    "modality_gap"} with summary = SimilarityStats.summary(), self_neg_mean the mean cosine between different rows of
    one set, modality_gap the norm of the difference of the two mean embeddings.  embed_fn(model, batch) -> (a, b)
    overrides retrieval.default_embed_fn; class_ids_fn(batch) -> ids [B] gives the pairs' class ids; scale None:
    exp(model.logit_scale) where the model has one (clamped as the model clamps it), else 1."""
    model.eval()
    fn = embed_fn if embed_fn is not None else default_embed_fn
    a_all, b_all, ids = [], [], []
    for batch in loader:
        batch = tuple(t.to(device) if (device is not None and torch.is_tensor(t)) else t for t in batch)
        a, b = fn(model, batch)
        a_all.append(_as_f32(a, "a embeddings"))
        b_all.append(_as_f32(b, "b embeddings"))
        if class_ids_fn is not None:
            ids.append(torch.as_tensor(class_ids_fn(batch)).reshape(-1))
    if not a_all:
        raise ValueError("empty loader")
    a, b = torch.cat(a_all), torch.cat(b_all)
    cls = torch.cat(ids) if ids else None
    sc = _model_scale(model) if scale is None else float(scale)
    out = {"a_to_b": similarity_stats(a, b, scale=sc, class_ids=cls, bins=bins).summary(),
           "b_to_a": similarity_stats(b, a, scale=sc, class_ids=cls, bins=bins).summary()}
    t = 2.0
    for name, e in (("a", a), ("b", b)):                  # one self pass per side: its lse gives the uniformity, its
        n = e.shape[0]                                    # negative sums (scaled by 2 t) the mean cosine of other rows
        if n < 2:
            out[name] = {"uniformity": float("nan"), "self_neg_mean": float("nan")}
            continue
        self_st = similarity_stats(e, e, scale=2.0 * t, bins=1)
        out[name] = {"uniformity": _uniformity_from(self_st, t),
                     "self_neg_mean": float(_f64(self_st.neg_sum).sum() / (2.0 * t) / (n * (n - 1)))}
    out["alignment"] = 2.0 - 2.0 * out["a_to_b"]["pos_mean"] / sc if sc != 0.0 else float("nan")
    out["modality_gap"] = float((a.double().mean(0) - b.double().mean(0)).norm())
    return out
