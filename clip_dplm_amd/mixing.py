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
has the truncated variant; DESIGN.md 3.20 records how far truncation moves the median).  lisi_knn below IS the published
definition, on the exact k-nearest-neighbour graph of neighbors.knn_graph, for comparison against published tables.

    label_masses            the per-point label masses' statistics from one walk per 512 labels (ops.label_kernel_sums):
                            mass, sum of squares, the heaviest label and its share; the [N, G] shares only when asked for.
    lisi                    mass^2 / sumsq per point.
    label_transfer          the leave-one-out kernel vote the same masses give: (predicted label, its share).
    integration_scores      iLISI over the concatenated clouds with the cloud index as label; with annotations also cLISI
                            and the label-transfer accuracy, on the same bandwidths.

    kbet                    the k-nearest-neighbour batch-effect test (Buettner et al. 2019): per row a chi-square test of its
                            neighbours' batch counts against the global shares; the rejection rate.
    lisi_knn                the published LISI: 3 x perplexity nearest neighbours, unsquared distances, its own bisection.

The walk has no CPU fallback; the small reductions (median_score, scale_ilisi, scale_clisi, merge_label_blocks) are torch
glue that also takes host tensors.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional

import torch

from . import _args, manifold, neighbors, ops

__all__ = ["LabelMasses", "label_masses", "lisi", "label_transfer", "label_transfer_accuracy", "integration_scores",
           "median_score", "scale_ilisi", "scale_clisi", "merge_label_blocks", "KBETResult", "kbet", "lisi_knn"]

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
    N = manifold.check_cloud(x, perplexity, metric)
    labels = _args.labels_arg("labels", labels, N)
    _args.int_in("num_labels", num_labels, 1, MAX_LABELS, optional=True)
    _args.int_in("row_block", row_block, 1, optional=True)
    if not isinstance(return_matrix, bool):
        raise ValueError(f"return_matrix must be a bool, got {return_matrix!r}")
    if bandwidths is not None:
        if not isinstance(bandwidths, (tuple, list)) or len(bandwidths) != 4:
            raise ValueError("bandwidths must be the (beta, dmin, log_s0, entropy) tuple of manifold.perplexity_bandwidths")
        for name, t in zip(("beta", "dmin", "log_s0", "entropy"), bandwidths):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (N,):
                raise ValueError(f"bandwidths: {name} must be a float32 tensor of shape ({N},)")
    _args.need_device("LISI needs", x, *(bandwidths or ()), labels if num_labels is not None else None)
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
    x = _args.prepare(x, metric)
    nx = (x * x).sum(1)
    beta, dmin, _, entropy = bandwidths if bandwidths is not None else manifold.calibrate(x, nx, perplexity, 8)
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
    return (predicted == _args.labels_arg("labels", labels).to(predicted.device)).float().mean()


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
    N, G = manifold.check_cloud(x, perplexity, metric), len(clouds)
    if labels is not None:
        labels = _args.labels_arg("labels", labels)
        if labels.shape[0] != N:
            raise ValueError(f"labels has {labels.shape[0]} entries for {N} rows of the concatenated clouds")
    _args.need_device("t-SNE needs", x)
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


# ------------------------------------------------------------------------------------------------ scores on the kNN graph
@dataclasses.dataclass
class KBETResult:
    """stat, pvalue f64 [N]: each row's chi-square statistic and its upper-tail probability; rejection_rate, acceptance:
    0-d f64 tensors, mean(pvalue < alpha) and 1 - that; expected_rejection_rate: the same under one random permutation of
    the labels on the same graph (None without a generator); k: the neighbours used; dof: 0-d int64 tensor, the non-empty
    labels - 1."""
    stat: torch.Tensor
    pvalue: torch.Tensor
    rejection_rate: torch.Tensor
    acceptance: torch.Tensor
    expected_rejection_rate: Optional[torch.Tensor]
    k: int
    dof: torch.Tensor


def _graph_rows(x, graph):
    """N of the cloud x, or of the graph given in its place; the argument errors of either."""
    if graph is not None:
        neighbors.check_graph(graph)
        return graph.indices.shape[0]
    _args.check_cloud(x)
    if x.shape[0] < 2:
        raise ValueError("at least 2 rows")
    return x.shape[0]


def _graph_labels(name, labels, num_labels, N):
    """The labels as positions 0..G-1 (int64 [N]) and G; every argument error first."""
    labels = _args.labels_arg(name, labels, N)
    _args.int_in("num_labels", num_labels, 1, optional=True)
    return labels


def _label_positions(labels, num_labels):
    """(the labels as positions 0..G-1, G): as they came with num_labels, else by torch.unique."""
    if num_labels is not None:
        return labels, num_labels
    values, inv = torch.unique(labels, return_inverse=True)
    return inv, values.shape[0]


def _check_k(k, N):
    kmax = min(neighbors.MAX_K, N - 1)
    _args.int_in("k", k, 1, kmax, what=f"None or an int in [1, min(1024, N - 1)] = [1, {kmax}]", optional=True)


def _graph_arg(x, graph, k, N):
    """The graph's first k columns (all of them for k None); builds the graph when none is given."""
    if graph is None:
        return neighbors.knn_graph(x, k)
    if k is not None and k > graph.k:
        raise ValueError(f"k = {k} exceeds the graph's {graph.k} neighbours")
    if k is None or k == graph.k:
        return graph
    return neighbors.KNNGraph(graph.indices[:, :k], graph.sqdist[:, :k])


def _kbet_stat(graph, lab, G, k):
    """(stat f64 [N], dof): sum over the non-empty labels of (n_ig - k f_g)^2 / (k f_g)."""
    counts = graph.label_counts(lab, G).double()
    share = torch.bincount(lab.clamp(0, G - 1), weights=((lab >= 0) & (lab < G)).double(), minlength=G) / lab.shape[0]
    full = share > 0
    expect = torch.where(full, k * share, torch.ones_like(share))
    stat = torch.where(full, (counts - expect) ** 2 / expect, torch.zeros_like(expect)).sum(1)
    return stat, full.sum() - 1


def kbet(x, batch, k: Optional[int] = None, alpha: float = 0.05, graph=None, num_labels: Optional[int] = None,
         generator=None) -> KBETResult:
    """kBET over the cloud x [N, P] (f32, device, P % 4 == 0) with the batch labels `batch` [N]: KBETResult.

    Per row, with n_ig the counts of the labels among its k nearest OTHER rows and f_g the global label shares:
    stat_i = sum_g (n_ig - k f_g)^2 / (k f_g), pvalue_i = P(chi2_{G-1} > stat_i) = gammaincc((G - 1) / 2, stat_i / 2) in
    f64; rejection_rate = mean(pvalue < alpha): 0 for batches mixed as in the whole cloud, 1 for separate ones.
    k=None: kBET's default floor(mean batch size / 4), clipped to [10, min(1024, N - 1)]; the result reports it.
    graph: a KNNGraph of the cloud against itself (neighbors.knn_graph(x, k)) to reuse; x is then not read (None is
    allowed), host tensors work, and a smaller k takes the graph's first k columns.
    num_labels=None relabels with torch.unique; num_labels=G: the labels are 0..G-1 already.  A label without points
    leaves the sum and the degrees of freedom.  generator: also the rate under one random permutation of the labels on
    the same graph (torch.randperm on the generator's device) - the rate a cloud without batch structure would show."""
    N = _graph_rows(x, graph)
    lab = _graph_labels("batch", batch, num_labels, N)
    _check_k(k, N)
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not 0 < alpha < 1:
        raise ValueError(f"alpha must lie in (0, 1), got {alpha!r}")
    if generator is not None and not isinstance(generator, torch.Generator):
        raise ValueError("generator must be None or a torch.Generator")
    if graph is None and not x.is_cuda:
        raise ValueError("kbet needs a device cloud or graph= (there is no CPU fallback for the search)")
    lab, G = _label_positions(lab, num_labels)
    if k is None and graph is None:
        full = int((torch.bincount(lab.clamp(0, G - 1), minlength=G) > 0).sum())
        k = min(max(10, N // max(full, 1) // 4), neighbors.MAX_K, N - 1)
    graph = _graph_arg(x, graph, k, N)
    k = graph.k
    lab = lab.to(graph.indices.device)
    stat, dof = _kbet_stat(graph, lab, G, k)
    pvalue = torch.special.gammaincc(dof.double() / 2, stat / 2)
    rate = (pvalue < alpha).double().mean()
    expected = None
    if generator is not None:
        perm = torch.randperm(N, generator=generator, device=generator.device).to(lab.device)
        stat_p, _ = _kbet_stat(graph, lab[perm], G, k)
        expected = (torch.special.gammaincc(dof.double() / 2, stat_p / 2) < alpha).double().mean()
    return KBETResult(stat, pvalue, rate, 1 - rate, expected, k, dof)


LISI_KNN_TRIES = 50
LISI_KNN_TOL = 1e-5


def _check_lisi_knn(perplexity, k, N):
    if isinstance(perplexity, bool) or not isinstance(perplexity, (int, float)) or not perplexity > 0:
        raise ValueError(f"perplexity must be a positive number, got {perplexity!r}")
    _check_k(k, N)
    if k is None and not 1 <= int(3 * perplexity) - 1 <= min(neighbors.MAX_K, N - 1):
        raise ValueError(f"3 * perplexity - 1 = {int(3 * perplexity) - 1} neighbours must lie in [1, min(1024, N - 1)] = "
                         f"[1, {min(neighbors.MAX_K, N - 1)}]")


def lisi_knn(x, labels, perplexity: float = 30.0, k: Optional[int] = None, graph=None,
             num_labels: Optional[int] = None) -> torch.Tensor:
    """f32 [N]: LISI as published (Korsunsky et al. 2019, compute_lisi) on the exact k-nearest-neighbour graph of the cloud
    x [N, P] (f32, device, P % 4 == 0): k = 3 * perplexity - 1 other rows (k=None), UNSQUARED Euclidean distances d.

    Per row: P = exp(-beta d) from beta = 1; H = log(sum P) + beta sum(d P) / sum P and P /= sum P (sum P == 0: H = 0,
    P = 0); up to 50 bisection steps on beta (doubling / halving while a bound is infinite) while |H - log(perplexity)| >=
    1e-5; Simpson = sum_g (sum of P over the neighbours of label g)^2, LISI = 1 / Simpson; a row with H == 0 has Simpson
    -1 (LISI -1), as there.  Vectorised in f64 over [N, k] with 50 masked steps and no host read: with num_labels (labels
    already 0..G-1 on the device) a call can be captured.  graph: a KNNGraph of the cloud against itself to reuse (x is
    not read and may be None; host tensors work; a smaller k takes its first k columns).  iLISI / cLISI by the label."""
    N = _graph_rows(x, graph)
    lab = _graph_labels("labels", labels, num_labels, N)
    _check_lisi_knn(perplexity, k, N)
    if graph is None and not x.is_cuda:
        raise ValueError("lisi_knn needs a device cloud or graph= (there is no CPU fallback for the search)")
    if k is None and graph is None:
        k = int(3 * perplexity) - 1
    graph = _graph_arg(x, graph, k, N)
    lab, G = _label_positions(lab, num_labels)
    idx = graph.indices
    return _lisi_knn_f64(graph, lab.to(idx.device)[idx.clamp(min=0)], G, perplexity).float()


def _lisi_knn_f64(graph, lab, G, perplexity):
    """f64 [N]: lisi_knn's arithmetic; lab int64 [N, k]: the neighbours' labels as positions 0..G-1."""
    d = graph.sqdist.double().sqrt()                                 # the root in f64: no second f32 rounding
    target = math.log(perplexity)

    def entropy(beta):
        p = torch.exp(-beta[:, None] * d)
        sp = p.sum(1)
        empty = sp == 0
        safe = torch.where(empty, torch.ones_like(sp), sp)
        h = torch.where(empty, torch.zeros_like(sp), torch.log(safe) + beta * (d * p).sum(1) / safe)
        return h, torch.where(empty[:, None], torch.zeros_like(p), p / safe[:, None])

    beta = torch.ones(d.shape[0], dtype=torch.float64, device=d.device)
    lo, hi = torch.full_like(beta, -math.inf), torch.full_like(beta, math.inf)
    h, p = entropy(beta)
    for _ in range(LISI_KNN_TRIES):
        diff = h - target
        active = diff.abs() >= LISI_KNN_TOL
        up = diff > 0
        lo = torch.where(active & up, beta, lo)
        hi = torch.where(active & ~up, beta, hi)
        nb = torch.where(up, torch.where(torch.isinf(hi), beta * 2, (beta + hi) / 2),
                         torch.where(torch.isinf(lo), beta / 2, (beta + lo) / 2))
        beta = torch.where(active, nb, beta)
        h2, p2 = entropy(beta)
        h, p = torch.where(active, h2, h), torch.where(active[:, None], p2, p)
    # sum_g (sum_{t: label_t = g} P_t)^2 = sum_{t, u: label_t = label_u} P_t P_u, in row chunks of about 128 MiB: a fixed
    # order whatever G is (a float scatter_add_ on the device is atomic, so its bits change from run to run)
    p = torch.where((lab >= 0) & (lab < G), p, torch.zeros_like(p))
    k = d.shape[1]
    rows = max(1, (1 << 24) // (k * k))
    same = [((p[r:r + rows, :, None] * p[r:r + rows, None, :])
             * (lab[r:r + rows, :, None] == lab[r:r + rows, None, :])).sum((1, 2)) for r in range(0, d.shape[0], rows)]
    simpson = torch.where(h == 0, torch.full_like(h, -1.0), torch.cat(same))
    return 1.0 / simpson
