"""Torch restatement of clipk_sim_stats (include/clipk.h) on the materialised similarity matrix: the f64 reference the
GPU tests compare the kernel with, and the f32 binning rule of its histograms.

Reference sites restated: the cosine_sims matrix of evaluate (run1/full.py:142-160), the argmax and its softmax
confidence of analyze_failure_cases (:415-430), the hardest negative of analyze_hard_negatives_impact (:449-461), the
argmax behind the confusion matrix (:257-268).  For query i with label l_i: E_i = {j != l_i : cls_y[j] == cls_x[i]},
N_i = {j : j != l_i, j not in E_i}; everything is taken over {l_i} u N_i or over N_i.
"""
import numpy as np
import torch


def inv_width(nbins, lo, hi):
    """nbins / (hi - lo) from the two f32 values in f64, rounded once to f32."""
    return np.float32(nbins / (float(np.float32(hi)) - float(np.float32(lo))))


def slots(S32, nbins, lo, hi):
    """int64 slots of f32 scores: 0 below lo, nbins + 1 at or above hi, else 1 + min(int((S - lo) * inv_w), nbins - 1)
    with the subtraction and the product as two separate f32 operations."""
    assert S32.dtype == torch.float32
    lo32, hi32 = float(np.float32(lo)), float(np.float32(hi))
    t = S32 - lo32                                       # f32
    t = t * float(inv_width(nbins, lo, hi))              # f32 (a python float that is an f32 value: no double rounding)
    b = t.clamp(min=0).to(torch.int64).clamp(max=nbins - 1)
    out = 1 + b
    out = torch.where(S32 >= hi32, torch.full_like(out, nbins + 1), out)
    return torch.where(S32 < lo32, torch.zeros_like(out), out)


def histogram(slot, mask, nbins):
    return torch.bincount(slot[mask].reshape(-1), minlength=nbins + 2)


def masks(Mx, Ny, labels, cls_x, cls_y, device):
    """(is_label, negative), each bool [Mx, Ny]; labels int64 [Mx] inside [0, Ny)."""
    j = torch.arange(Ny, device=device)
    is_label = j[None, :] == labels[:, None]
    excluded = torch.zeros_like(is_label)
    if cls_x is not None:
        excluded = (cls_x[:, None] == cls_y[None, :]) & ~is_label
    return is_label, ~is_label & ~excluded


def first_max(S, mask):
    """(max, lowest index attaining it) of every row over mask; (-inf, -1) for an empty row."""
    Ny = S.shape[1]
    Sm = S.masked_fill(~mask, float("-inf"))
    mx = Sm.max(1).values
    j = torch.arange(Ny, device=S.device)
    idx = torch.where((Sm == mx[:, None]) & mask, j[None, :], torch.full_like(j, Ny)[None, :]).min(1).values
    return mx, torch.where(idx == Ny, torch.full_like(idx, -1), idx)


def sim_stats(S, labels, cls_x=None, cls_y=None, nbins=64, lo=-1.0, hi=1.0):
    """S f64 [Mx, Ny] -> dict of the kernel's outputs in f64 / int64, plus "n_neg" [Mx] = |N_i|.  The histograms bin
    S rounded to f32 (exact for the tests' grid inputs)."""
    Mx, Ny = S.shape
    is_label, neg = masks(Mx, Ny, labels, cls_x, cls_y, S.device)
    keep = is_label | neg
    pos = S.gather(1, labels[:, None])[:, 0]
    best, best_idx = first_max(S, keep)
    hard, hard_idx = first_max(S, neg)
    lse = torch.logsumexp(S.masked_fill(~keep, float("-inf")), 1)
    Sn = S.masked_fill(~neg, 0.0)
    sl = slots(S.float(), nbins, lo, hi)
    return {"pos": pos, "best": best, "best_idx": best_idx, "hard": hard, "hard_idx": hard_idx, "lse": lse,
            "neg_sum": Sn.sum(1), "neg_sumsq": (Sn * Sn).sum(1), "n_neg": neg.sum(1),
            "hist_neg": histogram(sl, neg, nbins),
            "hist_pos": torch.bincount(slots(pos.float(), nbins, lo, hi), minlength=nbins + 2),
            "neg_mask": neg, "keep_mask": keep}


def summary(S, labels, cls_x=None, cls_y=None):
    """The floats of diagnostics.SimilarityStats.summary() from the f64 matrix (no histogram entries)."""
    r = sim_stats(S, labels, cls_x, cls_y)
    pos, hard = r["pos"], r["hard"]
    correct = r["best_idx"] == labels
    conf = torch.exp(r["best"] - r["lse"])
    n_neg = int(r["n_neg"].sum())
    neg_mean = float(r["neg_sum"].sum()) / n_neg
    neg_var = float(r["neg_sumsq"].sum()) / n_neg - neg_mean ** 2
    margin = pos - hard
    n = S.shape[0]
    return {"top1": int(correct.sum()) / n, "pos_mean": float(pos.mean()),
            "pos_std": float(pos.std(unbiased=False)), "neg_mean": neg_mean, "neg_std": neg_var ** 0.5,
            "margin_mean": float(margin.mean()), "margin_min": float(margin.min()),
            "violations": int((hard >= pos).sum()) / n, "confidence_mean": float(conf.mean()),
            "confidence_on_failures": float(conf[~correct].mean()) if (~correct).any() else float("nan"),
            "p_pos_mean": float(torch.exp(pos - r["lse"]).mean())}


def uniformity(a, t=2.0):
    """log mean_{i != j} exp(-t |a_i - a_j|^2) in f64 from the pairwise distances."""
    a = a.double()
    d2 = torch.cdist(a, a).pow(2)
    n = a.shape[0]
    off = ~torch.eye(n, dtype=torch.bool, device=a.device)
    return float(torch.logsumexp((-t * d2)[off], 0) - np.log(n * (n - 1)))


def group_similarity(a, ga, b, gb, G):
    """Brute mean of the materialised cosine blocks in f64 (analyze_embedding_collapse, run1/full.py:307-315)."""
    an = a.double() / a.double().norm(dim=1, keepdim=True)
    bn = b.double() / b.double().norm(dim=1, keepdim=True)
    C = an @ bn.t()
    out = torch.full((G, G), float("nan"), dtype=torch.float64, device=a.device)
    for g in range(G):
        for h in range(G):
            blk = C[ga == g][:, gb == h]
            if blk.numel():
                out[g, h] = blk.mean()
    return out
