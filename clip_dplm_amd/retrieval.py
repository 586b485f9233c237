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

Prefilter (`prefilter="bf16"` / `"bf16x3"` in `topk` and `EmbeddingIndex`): the same results, bit for bit, from a bf16
matrix-core candidate pass, an exact re-rank of `candidates` keys per query and a per-query certificate; queries the bound
cannot certify run the exact kernel (include/clipk.h: clipk_sim_topk_cand, clipk_sim_rerank).
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


PREFILTERS = (None, "bf16", "bf16x3")


def prefilter_eps_rel(P: int, mode: str) -> float:
    """eps_rel of the certificate (include/clipk.h, "Certificate"): a bound of |approximate - exact score| relative to
    |scale| |x| max|y|, for rows of P columns.  Operand rounding + bf16 MFMA accumulation (gamma = n 2^-22 over n
    products) + the exact f32 kernel's own error (P 2^-23) + the two multiplications by scale (2^-22)."""
    v = 2.0 ** -8                                    # bf16 keeps 8 significant bits: unit roundoff 2^-8
    if mode == "bf16":
        operands, acc = 2 * v + v * v, P * 2.0 ** -22 * (1 + v) ** 2
    elif mode == "bf16x3":
        operands, acc = 3 * v * v + 7 * v ** 3, 3 * P * 2.0 ** -22 * (1 + v) ** 2 * (1 + 2 * v)
    else:
        raise ValueError(f"prefilter must be one of {PREFILTERS}, got {mode!r}")
    return operands + acc + P * 2.0 ** -23 + 2.0 ** -22


def _prefilter_args(k, prefilter, candidates):
    """(k, kc): validated before any device work."""
    if prefilter not in PREFILTERS:
        raise ValueError(f"prefilter must be one of {PREFILTERS}, got {prefilter!r}")
    k = int(k)
    if prefilter is None:
        if candidates is not None:
            raise ValueError("candidates= needs a prefilter")
        return k, None
    if not 1 <= k <= 63:
        raise ValueError(f"k must be in [1, 63] with a prefilter, got {k}")
    if candidates is None:            # bf16's bound (~2^-7 relative) is wider than typical top-k / top-2k score gaps
        kc = 64 if prefilter == "bf16" else min(64, max(16, 2 * k))
    else:
        kc = int(candidates)
    if not k < kc <= 64:
        raise ValueError(f"candidates must satisfy k < candidates <= 64, got k = {k}, candidates = {kc}")
    return k, kc


def _new_planes(n: int, dim: int, mode: str, device):
    pp = ops.plane_pitch(dim)
    hi = torch.empty((n, pp), dtype=torch.bfloat16, device=device)
    lo = torch.empty((n, pp), dtype=torch.bfloat16, device=device) if mode == "bf16x3" else None
    return hi, lo


def _prefiltered_topk(q, g, hi, lo, norm_max, k, kc, scale, mode):
    """The four steps of include/clipk.h "Prefiltered exact top-k" on f32 q, g and g's planes."""
    Mq, P = q.shape
    Ny = g.shape[0]
    cs, ci = ops.sim_topk_cand(q, hi, lo, Ny, P, kc, scale)
    s, i, cert = ops.sim_rerank(q, g, cs, ci, k, prefilter_eps_rel(P, mode), norm_max, scale)
    bad = torch.nonzero(cert == 0).flatten()          # the one device -> host read of the call (not capturable)
    if bad.numel():                                   # the exact kernel on the uncertified rows; per-row results
        s2, i2 = ops.sim_topk(q.index_select(0, bad), g, k, scale)
        s.index_copy_(0, bad, s2)
        i.index_copy_(0, bad, i2)
    return s, i, {"queries": Mq, "certified": Mq - int(bad.numel()), "candidates": kc, "prefilter": mode}


def _exact_stats(Mq):
    return {"queries": Mq, "certified": None, "candidates": None, "prefilter": None}


def topk(queries: torch.Tensor, gallery: torch.Tensor, k: int, scale: Optional[float] = None,
         prefilter: Optional[str] = None, candidates: Optional[int] = None, return_stats: bool = False):
    """(scores f32 [Mq, k], idx int64 [Mq, k]): the k gallery rows most similar to each query (1 <= k <= 64).

    prefilter "bf16" / "bf16x3" (k <= 63): the same tensors, bit for bit, with most of the work on the bf16 matrix
    pipe; `candidates` (k < candidates <= 64; default 64 for bf16, min(64, max(16, 2 k)) for bf16x3) keys per query are
    re-scored exactly.
    The gallery's bf16 planes are built on every call (an EmbeddingIndex keeps them); the call reads one count back
    to the host.  return_stats: a third result {"queries", "certified", "candidates", "prefilter"}."""
    k, kc = _prefilter_args(k, prefilter, candidates)
    q, g = _as_f32(queries, "queries"), _as_f32(gallery, "gallery")
    if prefilter is None:
        s, i = ops.sim_topk(q, g, k, scale)
        return (s, i, _exact_stats(q.shape[0])) if return_stats else (s, i)
    Mq, Ny, P = ops._retrieval_args(q, g)
    if k > Ny:
        raise ValueError(f"k = {k} exceeds the gallery size {Ny}")
    ops._need_cuda(q, g)
    hi, lo = _new_planes(Ny, P, prefilter, g.device)
    norm_max = torch.zeros(1, dtype=torch.float32, device=g.device)
    ops.split_bf16(g, hi, lo, norm_max)
    s, i, stats = _prefiltered_topk(q, g, hi, lo, norm_max, k, kc, scale, prefilter)
    return (s, i, stats) if return_stats else (s, i)


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
    geometrically), search() is one topk over everything added so far.

    prefilter "bf16" / "bf16x3": add() also keeps the gallery's bf16 plane(s) and the running maximum row norm, and
    search() runs the prefiltered top-k on them (same results as without).  Memory: the f32 rows stay (the re-rank and
    the fallback read them); the planes add half of them (bf16: 1.5x in all) or as much again (bf16x3: 2x), with rows
    padded to a multiple of 32 columns.  state_dict() holds the f32 rows only; load_state_dict() rebuilds the planes."""

    def __init__(self, dim: int, device=None, prefilter: Optional[str] = None):
        if dim <= 0 or dim % 4:
            raise ValueError(f"dim must be a positive multiple of 4, got {dim}")
        if prefilter not in PREFILTERS:
            raise ValueError(f"prefilter must be one of {PREFILTERS}, got {prefilter!r}")
        self.dim = int(dim)
        self.prefilter = prefilter
        self.device = torch.device(device if device is not None else "cuda")
        self._reset()

    def _reset(self) -> None:
        self._buf = torch.empty((0, self.dim), dtype=torch.float32, device=self.device)
        self._n = 0
        if self.prefilter is not None:
            self._hi, self._lo = _new_planes(0, self.dim, self.prefilter, self.device)
            self._norm = torch.zeros(1, dtype=torch.float32, device=self.device)

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
            if self.prefilter is not None:
                hi, lo = _new_planes(cap, self.dim, self.prefilter, self.device)
                hi[:self._n].copy_(self._hi[:self._n])
                if lo is not None:
                    lo[:self._n].copy_(self._lo[:self._n])
                self._hi, self._lo = hi, lo
        self._buf[self._n:self._n + n].copy_(e)
        if self.prefilter is not None and n:
            rows = slice(self._n, self._n + n)
            ops.split_bf16(self._buf[rows], self._hi[rows], None if self._lo is None else self._lo[rows], self._norm)
        self._n += n

    def embeddings(self) -> torch.Tensor:
        return self._buf[:self._n]

    def search(self, queries: torch.Tensor, k: int, scale: Optional[float] = None, candidates: Optional[int] = None,
               return_stats: bool = False):
        """(scores, idx) of the k best gallery rows per query, as topk(queries, all added rows, k); with the index's
        prefilter, from its planes (candidates / return_stats as in topk)."""
        k, kc = _prefilter_args(k, self.prefilter, candidates)
        if self._n == 0:
            raise _ffi.ClipkError("search on an empty EmbeddingIndex")
        if self.prefilter is None:
            s, i = topk(queries.to(self.device), self.embeddings(), k, scale)
            return (s, i, _exact_stats(s.shape[0])) if return_stats else (s, i)
        q, g = _as_f32(queries.to(self.device), "queries"), self.embeddings()
        _, Ny, _ = ops._retrieval_args(q, g)
        if k > Ny:
            raise ValueError(f"k = {k} exceeds the gallery size {Ny}")
        lo = None if self._lo is None else self._lo[:self._n]
        s, i, stats = _prefiltered_topk(q, g, self._hi[:self._n], lo, self._norm, k, kc, scale, self.prefilter)
        return (s, i, stats) if return_stats else (s, i)

    def state_dict(self) -> dict:
        return {"dim": self.dim, "embeds": self.embeddings().clone()}

    def load_state_dict(self, state: dict) -> None:
        e = state["embeds"]
        if int(state["dim"]) != self.dim or e.dim() != 2 or e.shape[1] != self.dim:
            raise ValueError(f"state of a {state['dim']}-wide index loaded into a {self.dim}-wide one")
        self._reset()
        if e.shape[0]:
            self.add(e)
