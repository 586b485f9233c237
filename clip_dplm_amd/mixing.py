"""Exact LISI mixing scores over embedding clouds on the device, without the N x N matrix.

The reference asks whether the modalities of a trained model landed in one space with KMeans(n_clusters=10) + ARI per
cloud (analyze_embedding_alignment) and hand-picked cosine groups (analyze_embedding_collapse).  The score single-cell
integration work reports for that question is LISI, the local inverse Simpson's index (Korsunsky et al. 2019): the
effective number of distinct labels in each point's perplexity-calibrated neighbourhood.  iLISI takes the modality (or
batch) as the label - high means mixed; cLISI takes the cell type - low means conserved.

Definition used here.  With the conditional distribution of exact t-SNE at the given perplexity over the WHOLE cloud, on
SQUARED distances (manifold.perplexity_bandwidths: beta_i, dmin_i),

    w_ij = exp(-beta_i (d_ij - dmin_i)),  j != i        out[i, g] = sum_{j : label_j = g} w_ij        mass_i = sum_g out[i, g]
    p_i(g) = out[i, g] / mass_i                         LISI_i = 1 / sum_g p_i(g)^2 = mass_i^2 / sum_g out[i, g]^2

Every pair enters.  The published implementation truncates each neighbourhood to the 3 x perplexity nearest neighbours
and puts UNSQUARED distances in the exponent; neither is done here, so values differ from that package's (tests/lisi_ref.py
has the truncated variant; DESIGN.md 3.20 records how far truncation moves the median).

    label_masses            the per-point label masses' statistics from one walk per 512 labels (ops.label_kernel_sums):
                            mass, sum of squares, the heaviest label and its share; the [N, G] shares only when asked for.
    lisi                    mass^2 / sumsq per point.
    label_transfer          the leave-one-out kernel vote the same masses give: (predicted label, its share).
    integration_scores      iLISI over the concatenated clouds with the cloud index as label; with annotations also cLISI
                            and the label-transfer accuracy, on the same bandwidths.

The walk has no CPU fallback; the small reductions (median_score, scale_ilisi, scale_clisi, merge_label_blocks) are torch
glue that also takes host tensors.
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import torch

from . import manifold, ops
from .cluster import _labels_arg

__all__ = ["LabelMasses", "label_masses", "lisi", "label_transfer", "label_transfer_accuracy", "integration_scores",
           "median_score", "scale_ilisi", "scale_clisi", "merge_label_blocks"]

MAX_LABELS = ops.LABEL_DIST_MAX_LABELS              # in blocks of ops.LABEL_DIST_MAX_G, one walk each
BLOCK_BYTES = 256 << 20                             # the [rows, G] slab of one row block (default row_block)


@dataclasses.dataclass
class LabelMasses:
    """mass, sumsq f32 [N]; top int64 [N]: the heaviest label of each row as a position in 0..G-1 (equal masses: the
    lower); confidence f32 [N] = its mass / mass; beta, entropy f32 [N] from the calibration; p f32 [N, G] = the label
    shares, only with return_matrix; values: the label value of every position (None with num_labels: the positions are
    the labels); num_labels = G."""
    mass: torch.Tensor
    sumsq: torch.Tensor
    top: torch.Tensor
    confidence: torch.Tensor
    beta: torch.Tensor
    entropy: torch.Tensor
    p: Optional[torch.Tensor]
    values: Optional[torch.Tensor]
    num_labels: int

    @property
    def lisi(self) -> torch.Tensor:
        return self.mass * self.mass / self.sumsq

    @property
    def predicted(self) -> torch.Tensor:
        return self.top if self.values is None else self.values.to(self.top.device)[self.top]


# ------------------------------------------------------------------------------------------------ glue (host or device)
def merge_label_blocks(blocks):
    """(mass, sumsq, best, top) of all labels from the per-block tuples of consecutive label blocks, ascending, `top`
    already counted from the first label of all: the masses and the squares add, the maximum goes to the later block only
    where it is strictly larger - equal values stay with the lower label."""
    mass, sumsq, best, top = blocks[0]
    for m, q, b, t in blocks[1:]:
        later = b > best
        mass, sumsq = mass + m, sumsq + q
        best, top = torch.where(later, b, best), torch.where(later, t, top)
    return mass, sumsq, best, top


def median_score(values) -> float:
    """The median of per-point scores (any float tensor, host or device) as a Python float: the mean of the two middle
    values for an even count; rows that are NaN (no mass) are left out."""
    v = values.detach().double().flatten()
    v = v[~torch.isnan(v)].sort().values
    n = v.shape[0]
    if n == 0:
        return float("nan")
    return float(0.5 * (v[(n - 1) // 2] + v[n // 2]))


def scale_ilisi(median: float, num_labels: int) -> float:
    """(median - 1) / (G - 1): 0 for no mixing, 1 for G evenly mixed labels - the scaling of integration benchmarks."""
    return (median - 1.0) / (num_labels - 1) if num_labels > 1 else float("nan")


def scale_clisi(median: float, num_labels: int) -> float:
    """(G - median) / (G - 1): 1 for neighbourhoods of one label, 0 for G evenly mixed ones."""
    return (num_labels - median) / (num_labels - 1) if num_labels > 1 else float("nan")


# ------------------------------------------------------------------------------------------------ argument checks
def _check_args(x, labels, perplexity, metric, bandwidths, num_labels, row_block, return_matrix):
    """Every argument error, before any device work; the labels as an int64 vector."""
    manifold._check_cloud(x)
    N = x.shape[0]
    manifold._check_perplexity(perplexity, N)
    manifold._check_metric(metric)
    labels = _labels_arg("labels", labels)
    if labels.shape[0] != N:
        raise ValueError(f"labels has {labels.shape[0]} entries for {N} rows")
    if num_labels is not None:
        if isinstance(num_labels, bool) or not isinstance(num_labels, int) or not 1 <= num_labels <= MAX_LABELS:
            raise ValueError(f"num_labels must be None or an int in [1, {MAX_LABELS}], got {num_labels!r}")
    if row_block is not None and (isinstance(row_block, bool) or not isinstance(row_block, int) or row_block < 1):
        raise ValueError(f"row_block must be None or a positive int, got {row_block!r}")
    if not isinstance(return_matrix, bool):
        raise ValueError(f"return_matrix must be a bool, got {return_matrix!r}")
    if bandwidths is not None:
        if not isinstance(bandwidths, (tuple, list)) or len(bandwidths) != 4:
            raise ValueError("bandwidths must be the (beta, dmin, log_s0, entropy) tuple of manifold.perplexity_bandwidths")
        for name, t in zip(("beta", "dmin", "log_s0", "entropy"), bandwidths):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (N,):
                raise ValueError(f"bandwidths: {name} must be a float32 tensor of shape ({N},)")
    ts = [x] + (list(bandwidths) if bandwidths is not None else []) + ([labels] if num_labels is not None else [])
    if not all(t.is_cuda for t in ts):
        raise ValueError("LISI needs device tensors (there is no CPU fallback)")
    return labels


# ------------------------------------------------------------------------------------------------ the masses
@torch.no_grad()
def label_masses(x, labels, perplexity: float = 30.0, metric: str = "sqeuclidean", bandwidths=None,
                 num_labels: Optional[int] = None, row_block: Optional[int] = None,
                 return_matrix: bool = False) -> LabelMasses:
    """The label masses of every row's neighbourhood in the cloud x [N, P] (f32, device; N >= 3, P % 4 == 0, P <= 512)
    under the integer annotation labels [N]: LabelMasses.

    The neighbourhood of row i is the t-SNE conditional distribution at `perplexity` over the whole cloud on squared
    distances (metric "cosine": on 1 - cos), the row itself left out; see the module docstring for how that differs from
    the published LISI.  bandwidths: the tuple of manifold.perplexity_bandwidths(x, perplexity, metric=metric) - iLISI and
    cLISI of one cloud then share the ten calibration walks; None calibrates here.
    num_labels=None relabels with torch.unique (any integer values, device or host; the one host read: G is a shape).
    num_labels=G: the labels are already 0..G-1 on the device, nothing is read back and the call can be captured in a
    graph; a label outside [0, G) then belongs to no column - the point still is a row and a neighbour of no label.
    Rows go through in blocks of row_block against the whole cloud (default: about 256 MiB of [rows, G] partial sums).
    More than 512 labels cost one walk per 512; the blocks' statistics are merged by merge_label_blocks.
    The [N, G] shares are written only with return_matrix.
    A row's mass is 0 - its LISI and confidence NaN - only if every other labelled point's term underflows: with the
    calibrated shift the nearest neighbour's term is exactly 1, so this needs num_labels with the near points left out."""
    labels = _check_args(x, labels, perplexity, metric, bandwidths, num_labels, row_block, return_matrix)
    N = x.shape[0]
    if num_labels is None:
        values, inv = torch.unique(labels, return_inverse=True)
        G = values.shape[0]
        if G > MAX_LABELS:
            raise ValueError(f"at most {MAX_LABELS} distinct labels, got {G}")
    else:
        values, inv, G = None, labels, num_labels
    x = manifold._prepare(x, metric)
    nx = (x * x).sum(1)
    beta, dmin, _, entropy = bandwidths if bandwidths is not None else manifold._bandwidths(x, nx, perplexity, 8)
    beta, dmin = beta.contiguous(), dmin.contiguous()
    lab32 = inv.to(x.device).int()
    GB = ops.LABEL_DIST_MAX_G
    if row_block is None:
        row_block = max(64, BLOCK_BYTES // (4 * min((G + 3) // 4 * 4, GB)) // 64 * 64)
    label_blocks = [(g0, min(GB, G - g0), lab32 if g0 == 0 else lab32 - g0) for g0 in range(0, G, GB)]
    rows = []
    for r0 in range(0, N, row_block):
        r1 = min(N, r0 + row_block)
        parts, outs = [], []
        for g0, Gb, lab in label_blocks:
            out, mass, sumsq, top, best = ops.label_kernel_sums(x[r0:r1], x, lab, Gb, beta[r0:r1], dmin[r0:r1], nx[r0:r1],
                                                                nx, diag_offset=r0, want_out=return_matrix)
            parts.append((mass, sumsq, best, top.long() + g0))
            outs.append(out)
        rows.append((*merge_label_blocks(parts), torch.cat(outs, 1) if return_matrix else None))
    mass, sumsq, best, top, p = (torch.cat(c) if c[0] is not None else None for c in zip(*rows))
    if p is not None:
        p = p / mass[:, None]
    return LabelMasses(mass, sumsq, top, best / mass, beta, entropy, p, values, G)


def lisi(x, labels, **kw) -> torch.Tensor:
    """f32 [N] on the device: the local inverse Simpson's index mass^2 / sumsq = 1 / sum_g p_g^2 of every row - the
    effective number of labels in its neighbourhood, between 1 and G.  Arguments as label_masses.  NaN for a row without
    mass (label_masses says when that can happen)."""
    return label_masses(x, labels, **kw).lisi


def label_transfer(x, labels, **kw):
    """(predicted [N] int64 in the values of `labels`, confidence f32 [N]): the leave-one-out kernel vote - each row
    gets the label with the largest mass among the OTHER rows (equal masses: the lower label) and that label's share of
    the mass; the soft-kNN classifier the LISI masses give for free.  Arguments as label_masses."""
    m = label_masses(x, labels, **kw)
    return m.predicted, m.confidence


def label_transfer_accuracy(x, labels, **kw) -> torch.Tensor:
    """The mean agreement of label_transfer's prediction with `labels`: a 0-d f32 device tensor."""
    predicted, _ = label_transfer(x, labels, **kw)
    return (predicted == _labels_arg("labels", labels).to(predicted.device)).float().mean()


# ------------------------------------------------------------------------------------------------ the scores of a model
def _cloud_list(clouds):
    if isinstance(clouds, dict):
        names = [n for n in manifold.SPACES if n in clouds] + [n for n in clouds if n not in manifold.SPACES]
        clouds = [clouds[n] for n in names]
    elif not isinstance(clouds, (list, tuple)):
        raise ValueError("clouds must be a sequence or a dict of 2-D float32 device tensors")
    if len(clouds) < 2:
        raise ValueError(f"at least two clouds, got {len(clouds)}")
    for c in clouds:
        if not isinstance(c, torch.Tensor) or c.dim() != 2 or c.dtype != torch.float32:
            raise ValueError("clouds must be 2-D float32 device tensors")
        if c.shape[1] != clouds[0].shape[1]:
            raise ValueError(f"the clouds must have one width, got {c.shape[1]} and {clouds[0].shape[1]}")
        if c.shape[0] == 0:
            raise ValueError("an empty cloud")
    return list(clouds)


@torch.no_grad()
def integration_scores(clouds, labels=None, perplexity: float = 30.0, metric: str = "cosine") -> dict:
    """How well the modalities of a model share one space.  clouds: a sequence or dict of f32 device clouds of one width
    (the reference's {'cell_emb', 'pert_emb', 'protein_emb'} in that order; other keys after them); they are concatenated
    and the cloud index is the modality label.  Returns Python floats:

        "ilisi"         the median LISI of the modality label over all rows: 1 = every neighbourhood of one modality,
                        G = evenly mixed
        "ilisi_scaled"  (median - 1) / (G - 1)

    and with labels (one integer id per row of the concatenation - a cell type, a perturbation), on the same bandwidths:

        "clisi", "clisi_scaled" = (G_l - median) / (G_l - 1)     1 = the annotation is conserved in every neighbourhood
        "label_transfer_accuracy"                                the leave-one-out kernel vote against the annotation."""
    clouds = _cloud_list(clouds)
    x = torch.cat([c.detach() for c in clouds]).contiguous()
    manifold._check_cloud(x)
    N, G = x.shape[0], len(clouds)
    manifold._check_perplexity(perplexity, N)
    manifold._check_metric(metric)
    if labels is not None:
        labels = _labels_arg("labels", labels)
        if labels.shape[0] != N:
            raise ValueError(f"labels has {labels.shape[0]} entries for {N} rows of the concatenated clouds")
    manifold._check_device(x)
    modality = torch.repeat_interleave(torch.arange(G, device=x.device),
                                       torch.tensor([c.shape[0] for c in clouds], device=x.device), output_size=N)
    bw = manifold.perplexity_bandwidths(x, perplexity, metric=metric)
    med = median_score(label_masses(x, modality, perplexity, metric, bandwidths=bw, num_labels=G).lisi)
    out = {"ilisi": med, "ilisi_scaled": scale_ilisi(med, G)}
    if labels is not None:
        m = label_masses(x, labels, perplexity, metric, bandwidths=bw)
        med = median_score(m.lisi)
        out["clisi"], out["clisi_scaled"] = med, scale_clisi(med, m.num_labels)
        out["label_transfer_accuracy"] = float((m.predicted == labels.to(x.device)).double().mean())
    return out
