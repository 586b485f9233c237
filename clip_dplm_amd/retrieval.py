"""Cross-modal retrieval with trained dual encoders: top-k search and ranking metrics over embedding galleries.

The reference scores its models by `logits.argmax(dim=1) == arange(B)` per batch (run1/full.py:138,152), builds a
confusion matrix and failure analysis from that argmax (:265, :423) and materialises the full cosine-similarity matrix
(:157).  Here the similarity S = scale * queries . gallery^T is never written: `topk` and `ranks` are fused HIP kernels
(include/clipk.h: clipk_sim_topk, clipk_sim_rank) that keep the selection in registers while walking gallery tiles.

Order everywhere: score descending, equal scores by the lower gallery index (torch.argmax's first-occurrence rule), so
rank 0 is exactly the reference's "correct" and results do not depend on how the gallery is split or chunked.

Class ids (`class_ids=`): where several pairs share a partner (one RBP bound by many RNAs), their gallery rows are
identical and tie-breaking by index caps recall@1 below 1 even for a perfect model.  With ids the rank counts only gallery
rows of another class than the positive (include/clipk.h: clipk_sim_rank_cls); with all ids distinct it is the plain rank.
"""
from __future__ import annotations

from typing import Callable, Dict, Iterable, Optional, Sequence

import numpy as np
import torch

from . import _ffi, ops


def _as_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dim() != 2:
        raise ValueError(f"{name} must be a 2-D tensor")
    if t.dtype == torch.bfloat16:
        return ops.to_f32(t.contiguous())                  # plumbing: the kernels read exact f32
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 or bfloat16, got {t.dtype}")
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def topk(queries: torch.Tensor, gallery: torch.Tensor, k: int, scale: Optional[float] = None):
    """(scores f32 [Mq, k], idx int64 [Mq, k]): the k gallery rows most similar to each query (1 <= k <= 64)."""
    return ops.sim_topk(_as_f32(queries, "queries"), _as_f32(gallery, "gallery"), k, scale)


def _as_ids(t: torch.Tensor, n: int, device, name: str) -> torch.Tensor:
    if not torch.is_tensor(t) or t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError(f"{name} must be an integer tensor")
    t = t.to(device=device, dtype=torch.int64).reshape(-1).contiguous()
    if t.numel() != n:
        raise ValueError(f"{name} must hold {n} ids, got {t.numel()}")
    return t


def ranks(queries: torch.Tensor, gallery: torch.Tensor, labels: Optional[torch.Tensor] = None,
          scale: Optional[float] = None, class_ids: Optional[torch.Tensor] = None) -> torch.Tensor:
    """0-based rank (int64 [Mq]) of each query's positive gallery row: labels[i], or i when labels is None.
    class_ids [Ng]: gallery class ids; only rows of another class than the positive's count."""
    q, g = _as_f32(queries, "queries"), _as_f32(gallery, "gallery")
    if labels is not None:
        labels = labels.to(device=q.device, dtype=torch.int64).contiguous()
    if class_ids is not None:
        class_ids = _as_ids(class_ids, g.shape[0], q.device, "class_ids")
    return ops.sim_rank(q, g, labels=labels, scale=scale, class_ids=class_ids)[0]


def metrics_from_ranks(ranks, ks: Sequence[int] = (1, 5, 10)) -> Dict[str, float]:
    """top1, recall@k, mrr, mean_rank and median_rank (1-based) of 0-based ranks; reduced in f64 on the host."""
    r = ranks.detach().cpu().numpy() if torch.is_tensor(ranks) else np.asarray(ranks)
    r = r.astype(np.float64).reshape(-1) + 1.0
    if r.size == 0:
        raise ValueError("no ranks")
    if (r < 1).any():
        raise ValueError("negative rank: a label was outside the gallery")
    out = {"n": int(r.size), "top1": float(np.mean(r == 1))}
    for k in ks:
        out[f"recall@{int(k)}"] = float(np.mean(r <= k))
    out["mrr"] = float(np.mean(1.0 / r))
    out["mean_rank"] = float(np.mean(r))
    out["median_rank"] = float(np.median(r))
    return out


def retrieval_metrics(a_embeds: torch.Tensor, b_embeds: torch.Tensor, ks: Sequence[int] = (1, 5, 10),
                      labels: Optional[torch.Tensor] = None,
                      class_ids: Optional[torch.Tensor] = None) -> Dict[str, Optional[Dict[str, float]]]:
    """{"a_to_b": ..., "b_to_a": ...}: a_i's positive is b[labels[i]] (b_i when labels is None).  b_to_a needs the
    inverse pairing: it is None when labels is not a permutation of range(len(b)).
    class_ids: the pairs' class ids, one per row of b (pairs that share a partner share an id); a row of a has its
    positive's id.  Both directions then rank among the rows of other classes only."""
    na, nb = a_embeds.shape[0], b_embeds.shape[0]
    ids_b = None if class_ids is None else _as_ids(class_ids, nb, a_embeds.device, "class_ids")
    if labels is None:
        if na != nb:
            raise ValueError(f"paired embeddings need equal counts, got {na} and {nb}")
        return {"a_to_b": metrics_from_ranks(ranks(a_embeds, b_embeds, class_ids=ids_b), ks),
                "b_to_a": metrics_from_ranks(ranks(b_embeds, a_embeds, class_ids=ids_b), ks)}
    labels = labels.to(device=a_embeds.device, dtype=torch.int64).reshape(-1)
    out = {"a_to_b": metrics_from_ranks(ranks(a_embeds, b_embeds, labels, class_ids=ids_b), ks), "b_to_a": None}
    if na == nb and torch.equal(torch.sort(labels).values, torch.arange(nb, device=labels.device)):
        inv = torch.empty_like(labels)
        inv[labels] = torch.arange(na, device=labels.device)
        ids_a = None if ids_b is None else ids_b[labels]
        out["b_to_a"] = metrics_from_ranks(ranks(b_embeds, a_embeds, inv, class_ids=ids_a), ks)
    return out


def _pair_from_output(out):
    if isinstance(out, dict):
        keys = [k for k in out if k.endswith("_embeds")]
        if len(keys) == 2:
            return out[keys[0]], out[keys[1]]
        raise TypeError(f"model output has embedding keys {keys}: pass embed_fn to choose the two modalities")
    if isinstance(out, (tuple, list)) and len(out) >= 2 and torch.is_tensor(out[0]) and torch.is_tensor(out[1]):
        return out[0], out[1]
    raise TypeError(f"cannot find two embeddings in a model output of type {type(out).__name__}: pass embed_fn")


def default_embed_fn(model, batch):
    """(a, b) embeddings of one batch: model.embed(*batch) where it exists (_PairCLIPModule, ProteinRNACLIP,
    OptimizedCLIPModule), else model(*batch): the first two elements of a tuple (RNARBPCLIPModel's (a, b, loss)) or the
    two `*_embeds` entries of a dict (the RNAProteinCLIP wrappers)."""
    embed = getattr(model, "embed", None)
    out = embed(*batch) if callable(embed) else model(*batch)
    return _pair_from_output(out)


@torch.no_grad()
def evaluate_retrieval(model, loader: Iterable, ks: Sequence[int] = (1, 5, 10),
                       embed_fn: Optional[Callable] = None, per_batch: bool = False, device=None):
    """Retrieval metrics of a paired loader (a_i belongs with b_i), both directions.

    per_batch=True: each batch is ranked against itself, the reference's evaluate (run1/full.py:152): top1 is then its
    accuracy, correct / total of argmax(logits, 1) == arange(B).  Default: every embedding of the loader against the whole
    set.  embed_fn(model, batch) -> (a, b) overrides default_embed_fn (needed for the tri-modal ContrastiveModel)."""
    model.eval()
    fn = embed_fn if embed_fn is not None else default_embed_fn
    a_all, b_all, r_ab, r_ba = [], [], [], []
    for batch in loader:
        batch = tuple(b.to(device) if (device is not None and torch.is_tensor(b)) else b for b in batch)
        a, b = fn(model, batch)
        if per_batch:
            r_ab.append(ranks(a, b))
            r_ba.append(ranks(b, a))
        else:
            a_all.append(_as_f32(a, "a embeddings"))
            b_all.append(_as_f32(b, "b embeddings"))
    if per_batch:
        if not r_ab:
            raise ValueError("empty loader")
        return {"a_to_b": metrics_from_ranks(torch.cat(r_ab), ks), "b_to_a": metrics_from_ranks(torch.cat(r_ba), ks)}
    if not a_all:
        raise ValueError("empty loader")
    return retrieval_metrics(torch.cat(a_all), torch.cat(b_all), ks)


class EmbeddingIndex:
    """An exact gallery for repeated top-k search: add() appends embeddings to a device buffer the index owns (grown
    geometrically), search() is one topk over everything added so far."""

    def __init__(self, dim: int, device=None):
        if dim <= 0 or dim % 4:
            raise ValueError(f"dim must be a positive multiple of 4, got {dim}")
        self.dim = int(dim)
        self.device = torch.device(device if device is not None else "cuda")
        self._buf = torch.empty((0, self.dim), dtype=torch.float32, device=self.device)
        self._n = 0

    def __len__(self) -> int:
        return self._n

    def add(self, embeds: torch.Tensor) -> None:
        if embeds.dim() != 2 or embeds.shape[1] != self.dim:
            raise ValueError(f"expected [n, {self.dim}] embeddings, got {tuple(embeds.shape)}")
        e = _as_f32(embeds.to(self.device), "embeds")
        n = e.shape[0]
        if self._n + n > self._buf.shape[0]:
            cap = max(self._n + n, 2 * self._buf.shape[0], 1024)
            buf = torch.empty((cap, self.dim), dtype=torch.float32, device=self.device)
            buf[:self._n].copy_(self._buf[:self._n])
            self._buf = buf
        self._buf[self._n:self._n + n].copy_(e)
        self._n += n

    def embeddings(self) -> torch.Tensor:
        return self._buf[:self._n]

    def search(self, queries: torch.Tensor, k: int, scale: Optional[float] = None):
        """(scores, idx) of the k best gallery rows per query, as topk(queries, all added rows, k)."""
        if self._n == 0:
            raise _ffi.ClipkError("search on an empty EmbeddingIndex")
        return topk(queries.to(self.device), self.embeddings(), k, scale)

    def state_dict(self) -> dict:
        return {"dim": self.dim, "embeds": self.embeddings().clone()}

    def load_state_dict(self, state: dict) -> None:
        e = state["embeds"]
        if int(state["dim"]) != self.dim or e.dim() != 2 or e.shape[1] != self.dim:
            raise ValueError(f"state of a {state['dim']}-wide index loaded into a {self.dim}-wide one")
        self._buf = torch.empty((0, self.dim), dtype=torch.float32, device=self.device)
        self._n = 0
        if e.shape[0]:
            self.add(e)
