"""Clustering of embedding clouds on the device and the agreement of two clusterings: k-means on the fused Lloyd step
of csrc/kmeans.hip, the adjusted Rand index, the normalised mutual information, and the reference's alignment check.

The reference asks whether two modalities landed in one space with analyze_embedding_alignment
(tong/tests/losses/test_contrastive.py:11-16): KMeans(n_clusters=10) on the cell embeddings and on the protein
embeddings, then the adjusted Rand index between the two labelings.  cluster_agreement is that function; the cloud
never leaves the device.

One Lloyd iteration on x [N, P] with centroids c [K, P] (f32, device):

    labels[i] = argmax_c 2 <x_i, c_c> - |c_c|^2  (= argmin_c |x_i - c_c|^2; equal scores go to the lower c)
    c_c <- mean of the points with labels[i] = c;  a cluster without points keeps its centroid

K <= 64: one ops.kmeans_step call (include/clipk.h: clipk_kmeans_step) - assignment and update read each tile of x once,
the N x K scores never leave the workgroup.  K > 64: ops.sim_top2_bias assigns, ops.kmeans_step sums under those labels.
What is left to ATen is O((N + K) P) glue: the division by the counts, the centroid norms, the seeding.

Whether a labeling - a k-means result, or an annotation such as the cell types - is any good: the silhouette width per
point, per label and overall on ops.label_dist_sums (include/clipk.h: clipk_label_dist_sums; the N x N distances never
leave the workgroups), the Davies-Bouldin and Calinski-Harabasz scores as f64 glue on cluster sums, and
choose_n_clusters, which makes the reference's hard-coded 10 checkable.
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import torch

from . import _args, ops

__all__ = ["kmeans", "KMeansResult", "init_centroids", "contingency", "adjusted_rand_index", "normalized_mutual_info",
           "cluster_agreement", "silhouette_samples", "silhouette_score", "silhouette_by_label", "davies_bouldin_score",
           "calinski_harabasz_score", "label_separation", "choose_n_clusters"]

METRICS = ("euclidean", "cosine")
INITS = ("k-means++", "random")


# ------------------------------------------------------------------------------------------------ seeding
def init_centroids(x, n_clusters: int, init="k-means++", generator=None):
    """n_clusters distinct rows of x [N, P] (any device) as the initial centroids [K, P].

    "random": the first K entries of a random permutation of the rows.  "k-means++" (Arthur & Vassilvitskii 2007): the
    first centre uniformly, each further one drawn with probability proportional to the squared distance to the nearest
    centre chosen so far (torch.multinomial under `generator`); a chosen row has distance exactly 0 and is not drawn
    again.  The D^2 update per centre is one pass over x, K passes in all, and nothing is read back."""
    if init not in INITS:
        raise ValueError(f"init must be one of {INITS} or a tensor, got {init!r}")
    N = x.shape[0]
    gen = _args.generator_for(generator, x.device)
    if init == "random":
        return x[torch.randperm(N, generator=gen, device=x.device)[:n_clusters]].clone()
    idx = torch.randint(N, (1,), generator=gen, device=x.device)
    chosen = [idx]
    d2 = (x - x[idx]).square().sum(1)
    for _ in range(1, n_clusters):
        w = d2 + (d2.sum() == 0).to(d2.dtype)                    # fewer distinct rows than K: uniform, no empty draw
        idx = torch.multinomial(w, 1, generator=gen)
        chosen.append(idx)
        d2 = torch.minimum(d2, (x - x[idx]).square().sum(1))
    return x[torch.cat(chosen)].clone()


# ------------------------------------------------------------------------------------------------ k-means
@dataclasses.dataclass
class KMeansResult:
    """centroids f32 [K, P]; labels int64 [N] and inertia (0-d f32 tensor: sum_i |x_i - c_labels[i]|^2, for the cosine
    metric on the normalised rows) from one final assignment against these centroids; counts int64 [K] of those labels and
    n_empty (0-d int64 tensor) = the clusters among them without a point; n_iter Lloyd iterations run; converged: the
    stopping rule was met (always False with tol=None, which never looks)."""
    centroids: torch.Tensor
    labels: torch.Tensor
    inertia: torch.Tensor
    n_iter: int
    converged: bool
    counts: torch.Tensor
    n_empty: torch.Tensor
    metric: str = "euclidean"

    def predict(self, x):
        """The nearest centroid of every row of x [M, P] (f32, device): int64 [M], the assignment `labels` came from."""
        _check_cloud(x)
        return _assign(_args.prepare(x, self.metric, half=False), self.centroids, self.metric)[0].long()


def _check_cloud(x, n_clusters: Optional[int] = None):
    """The k-means limits.  Its own wording, not _args.check_cloud's: a non-tensor and a wrong dtype are TypeErrors here,
    and an empty cloud is reported with the dimension."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a tensor")
    if x.dtype != torch.float32:
        raise TypeError(f"x must be float32, got {x.dtype}")
    if x.dim() != 2 or x.shape[0] == 0:
        raise ValueError(f"x must be a non-empty 2-D tensor, got shape {tuple(x.shape)}")
    P = x.shape[1]
    if P == 0 or P % 4 or P > ops.KMEANS_MAX_P:
        raise ValueError(f"the width must be a multiple of 4 and at most {ops.KMEANS_MAX_P}, got {P}")
    if x.shape[0] > ops.KMEANS_MAX_N:
        raise ValueError(f"at most {ops.KMEANS_MAX_N} rows, got {x.shape[0]}")
    if n_clusters is not None:                                     # (inline: the message goes on after the value)
        if isinstance(n_clusters, bool) or not isinstance(n_clusters, int):
            raise TypeError(f"n_clusters must be an int, got {n_clusters!r}")
        if not 1 <= n_clusters <= min(x.shape[0], ops.KMEANS_MAX_K):
            raise ValueError(f"n_clusters must be in [1, min(N, {ops.KMEANS_MAX_K})], got {n_clusters} for N = {x.shape[0]}")


def _check_args(x, n_clusters, init, n_init, max_iter, tol, check_every, metric):
    """Every argument error of kmeans(), raised before anything is launched."""
    _check_cloud(x, n_clusters)
    _args.check_metric(metric, METRICS)
    if isinstance(init, torch.Tensor):
        if init.dtype != torch.float32:
            raise TypeError(f"init must be float32, got {init.dtype}")
        if init.shape != (n_clusters, x.shape[1]):
            raise ValueError(f"init must have shape ({n_clusters}, {x.shape[1]}), got {tuple(init.shape)}")
    elif init is not None and init not in INITS:
        raise ValueError(f"init must be one of {INITS} or a tensor, got {init!r}")
    for name, v, lo in (("n_init", n_init, 1), ("max_iter", max_iter, 0), ("check_every", check_every, 1)):
        _args.int_in(name, v, lo, what=f"at least {lo}", type_error=True)
    if tol is not None and not float(tol) >= 0:
        raise ValueError(f"tol must be None or a non-negative number, got {tol!r}")
    _args.need_device("kmeans needs", x, init if isinstance(init, torch.Tensor) else None)


def _norms(c, metric):
    """The nc of clipk_kmeans_step: the squared norms, or zeros for the cosine form (unit centroids)."""
    return torch.zeros(c.shape[0], dtype=torch.float32, device=c.device) if metric == "cosine" else (c * c).sum(1)


def _assign(x, c, metric):
    """(labels int32 [N], d2 f32 [N]): the nearest centroid and the squared distance to it, by ops.sim_top2_bias."""
    nc = _norms(c, metric)
    two = torch.full((1,), 2.0, dtype=torch.float32, device=x.device)
    labels, best, _ = ops.sim_top2_bias(x, c, two, bias=-nc, want_gap=False)
    if metric == "cosine":
        best = best - 1.0                                       # |c|^2 = 1 left out of the scores
    return labels, ((x * x).sum(1) - best).clamp_min(0)


def _lloyd(x, c, metric, prev):
    """One iteration on device state: (new centroids, labels int32, sum |dC|^2 (0-d), no label changed (0-d bool))."""
    nc = _norms(c, metric)
    if c.shape[0] <= ops.KMEANS_MAX_K_FUSED:
        labels, _, sums, counts = ops.kmeans_step(x, c, nc)
    else:
        two = torch.full((1,), 2.0, dtype=torch.float32, device=x.device)
        labels, _, _ = ops.sim_top2_bias(x, c, two, bias=-nc, want_best=False, want_gap=False)
        _, _, sums, counts = ops.kmeans_step(x, c, labels=labels)
    new = torch.where(counts[:, None] > 0, sums / counts.clamp_min(1.0)[:, None], c)     # an empty cluster keeps its centroid
    if metric == "cosine":
        new = torch.nn.functional.normalize(new, dim=1)
    shift = (new - c).square().sum()
    same = (labels == prev).all() if prev is not None else torch.zeros((), dtype=torch.bool, device=x.device)
    return new, labels, shift, same


def _fit(x, c, metric, max_iter, tol, check_every):
    labels = None
    n_iter, converged = 0, False
    if tol is not None:
        tol_abs = float(tol) * x.var(dim=0, unbiased=False).mean()
    while n_iter < max_iter:
        c, labels, shift, same = _lloyd(x, c, metric, labels)
        n_iter += 1
        if tol is not None and (n_iter % check_every == 0 or n_iter == max_iter):
            if bool(same | (shift <= tol_abs)):                   # the one host read per check_every iterations
                converged = True
                break
    labels, d2 = _assign(x, c, metric)
    labels = labels.long()
    # (not torch.bincount: on the device it reads the largest label back, which a graph capture cannot do)
    counts = torch.zeros(c.shape[0], dtype=torch.int64, device=x.device).scatter_add_(0, labels, torch.ones_like(labels))
    return KMeansResult(c, labels, d2.sum(), n_iter, converged, counts, (counts == 0).sum(), metric)


@torch.no_grad()
def kmeans(x, n_clusters: int, *, init=None, n_init: int = 1, max_iter: int = 300, tol: Optional[float] = 1e-4,
           check_every: int = 4, metric: str = "euclidean", generator=None) -> KMeansResult:
    """Lloyd's k-means on the cloud x [N, P] (f32, device; P % 4 == 0, P <= 512, N <= 2^24) with n_clusters <= 65536
    centroids.

    init: "k-means++", "random" (distinct rows of x) or a tensor [K, P] of starting centroids.  None = "k-means++" for
    n_clusters <= 64 and "random" beyond: the seeding costs K passes over x, which the fused iteration does not.
    n_init: runs from independent seedings, the one with the lowest inertia is returned (a tensor init is one run).
    Stopping (sklearn's rule): no label changed since the last iteration, or sum |dC|^2 <= tol x the mean over the features
    of the variance of x; looked at once per check_every iterations - the only host read of the loop - and at max_iter.
    tol=None: exactly max_iter iterations and no host read at all, so the call can be captured in a graph (with a tensor
    init or "random"; every field of the result that depends on the data is a device tensor).
    metric="cosine": spherical k-means - the rows of x are L2-normalised, the assignment is argmax <x, c>, the centroids
    are L2-normalised means.
    A cluster that loses all its points keeps its centroid; n_empty counts them in the result."""
    _check_args(x, n_clusters, init, n_init, max_iter, tol, check_every, metric)
    if init is None:
        init = "k-means++" if n_clusters <= ops.KMEANS_MAX_K_FUSED else "random"
    x = _args.prepare(x, metric, half=False)
    best = None
    for _ in range(1 if isinstance(init, torch.Tensor) else n_init):
        c = init.detach().contiguous() if isinstance(init, torch.Tensor) else init_centroids(x, n_clusters, init, generator)
        if metric == "cosine":
            c = torch.nn.functional.normalize(c, dim=1)
        res = _fit(x, c, metric, max_iter, tol, check_every)
        if best is None:
            best = res
        elif tol is None:                                         # no host read: chosen field by field on the device
            better = res.inertia < best.inertia
            best = dataclasses.replace(best, **{f: torch.where(better, getattr(res, f), getattr(best, f))
                                                for f in ("centroids", "labels", "inertia", "counts", "n_empty")})
        elif bool(res.inertia < best.inertia):
            best = res
    return best


# ------------------------------------------------------------------------------------------------ agreement of two labelings
def contingency(labels_a, labels_b):
    """int64 [Ga, Gb]: entry (g, h) counts the points with labels_a == g and labels_b == h (non-negative integer labels
    [n], device or host; Ga, Gb = the largest label + 1).  One torch.bincount over the pair index."""
    a, b = _args.labels_arg("labels_a", labels_a), _args.labels_arg("labels_b", labels_b)
    if a.shape != b.shape:
        raise ValueError(f"the labelings have {a.shape[0]} and {b.shape[0]} entries")
    if a.device != b.device:
        raise ValueError(f"the labelings are on {a.device} and {b.device}")
    if a.numel() == 0:
        return torch.zeros((0, 0), dtype=torch.int64, device=a.device)
    if int(torch.minimum(a.min(), b.min())) < 0:
        raise ValueError("labels must be non-negative")
    ga, gb = int(a.max()) + 1, int(b.max()) + 1
    return torch.bincount(a * gb + b, minlength=ga * gb).reshape(ga, gb)


def adjusted_rand_index(labels_a, labels_b) -> float:
    """The adjusted Rand index (Hubert & Arabie 1985) of two labelings of the same points, from the contingency table in
    f64: 1 for the same partition under any names, about 0 for independent ones, negative below chance.  Degenerate
    inputs - fewer than 2 points, or one cluster on both sides, or every point its own cluster on both sides - give 1.0,
    as sklearn does."""
    t = contingency(labels_a, labels_b).double()
    n = float(t.sum())
    if n < 2:
        return 1.0
    pairs = lambda v: float((v * (v - 1) / 2).sum())             # noqa: E731
    s, sa, sb, tot = pairs(t), pairs(t.sum(1)), pairs(t.sum(0)), n * (n - 1) / 2
    expected, mean = sa * sb / tot, 0.5 * (sa + sb)
    if mean == expected:                                         # both trivial: one cluster each, or all singletons
        return 1.0
    return (s - expected) / (mean - expected)


def normalized_mutual_info(labels_a, labels_b) -> float:
    """Mutual information of two labelings over the arithmetic mean of their entropies (sklearn's default
    normalisation), from the contingency table in f64, natural logarithms.  One cluster on both sides, or no points,
    gives 1.0; one cluster on one side only gives 0.0."""
    t = contingency(labels_a, labels_b).double()
    n = float(t.sum())
    if n == 0:
        return 1.0
    pa, pb, pab = t.sum(1) / n, t.sum(0) / n, t / n
    entropy = lambda p: float(-(p[p > 0] * p[p > 0].log()).sum())             # noqa: E731
    ha, hb = entropy(pa), entropy(pb)
    if ha == 0.0 and hb == 0.0:
        return 1.0
    nz = pab > 0
    mi = float((pab[nz] * (pab[nz] / (pa[:, None] * pb[None, :])[nz]).log()).sum())
    return min(max(mi / (0.5 * (ha + hb)), 0.0), 1.0)


@torch.no_grad()
def cluster_agreement(a, b, n_clusters: int = 10, labels=None, silhouette: bool = False, **kmeans_kw) -> dict:
    """The reference's analyze_embedding_alignment: k-means with n_clusters on each of the paired clouds a [N, Pa] and
    b [N, Pb] (row i of both is one sample), then {"ari", "nmi"} between the two labelings, Python floats.  labels (an
    integer annotation [N], e.g. the cell types): also "ari_a_vs_labels", "nmi_a_vs_labels", "ari_b_vs_labels",
    "nmi_b_vs_labels".  silhouette=True: also "silhouette_a", "silhouette_b" - silhouette_score of each cloud under its own
    k-means labels, in the k-means metric - and with labels "silhouette_a_vs_labels", "silhouette_b_vs_labels", each cloud
    under the annotation.  Keyword arguments go to kmeans()."""
    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise TypeError(f"{name} must be a 2-D tensor")
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"the clouds are paired row by row, got {a.shape[0]} and {b.shape[0]} rows")
    if labels is not None:
        labels = _args.labels_arg("labels", labels, a.shape[0])
    la, lb = kmeans(a, n_clusters, **kmeans_kw).labels, kmeans(b, n_clusters, **kmeans_kw).labels
    out = {"ari": adjusted_rand_index(la, lb), "nmi": normalized_mutual_info(la, lb)}
    metric = kmeans_kw.get("metric", "euclidean")
    if silhouette:
        out["silhouette_a"], out["silhouette_b"] = silhouette_score(a, la, metric), silhouette_score(b, lb, metric)
    if labels is not None:
        labels = labels.to(la.device)
        for name, l, cloud in (("a", la, a), ("b", lb, b)):
            out[f"ari_{name}_vs_labels"] = adjusted_rand_index(l, labels)
            out[f"nmi_{name}_vs_labels"] = normalized_mutual_info(l, labels)
            if silhouette:
                out[f"silhouette_{name}_vs_labels"] = silhouette_score(cloud, labels, metric)
    return out


# ------------------------------------------------------------------------------------------------ quality of one labeling
SILHOUETTE_METRICS = ops.LABEL_DIST_METRICS
SILHOUETTE_BLOCK_BYTES = 256 << 20                  # the [rows, G] sums of one row block (default row_block)
CRITERIA = ("silhouette", "calinski_harabasz", "davies_bouldin")


def _relabel(x, labels):
    """(label values [G] ascending, positions int64 [N] in 0..G-1, counts int64 [G]) of an annotation of x's rows; the
    ValueError of every score here unless 2 <= G <= N - 1.  torch.unique: the one host read (G is a shape)."""
    N = x.shape[0]
    labels = _args.labels_arg("labels", labels, N)
    values, inv, counts = torch.unique(labels, return_inverse=True, return_counts=True)
    G = values.shape[0]
    if not 2 <= G <= N - 1:
        raise ValueError(f"the number of distinct labels must be in [2, N - 1], got {G} for N = {N}")
    return values, inv, counts


def _silhouette(x, labels, metric, row_block):
    """(s f32 [N], values, inv, counts): every argument error first, then the row-block walks."""
    _check_cloud(x)
    _args.check_metric(metric, SILHOUETTE_METRICS)
    _args.int_in("row_block", row_block, 1, optional=True)
    values, inv, counts = _relabel(x, labels)
    _args.need_device("the silhouette needs", x)
    G, N = values.shape[0], x.shape[0]
    if G > ops.LABEL_DIST_MAX_LABELS:
        raise ValueError(f"at most {ops.LABEL_DIST_MAX_LABELS} distinct labels, got {G}")
    x = _args.prepare(x, metric, half=False)
    inv, counts = inv.to(x.device), counts.to(x.device)
    lab32 = inv.int()
    nx = None if metric == "cosine" else (x * x).sum(1)
    n = counts.float()
    if row_block is None:
        row_block = max(64, SILHOUETTE_BLOCK_BYTES // (4 * ((G + 3) // 4 * 4)) // 64 * 64)
    s = torch.empty(N, dtype=torch.float32, device=x.device)
    for r0 in range(0, N, row_block):
        r1 = min(N, r0 + row_block)
        d = ops.label_dist_sums(x[r0:r1], x, lab32, G, metric, None if nx is None else nx[r0:r1], nx, diag_offset=r0)
        own = inv[r0:r1, None]
        n_own = n[inv[r0:r1]]
        a = d.gather(1, own)[:, 0] / (n_own - 1).clamp_min(1.0)
        b = (d / n[None, :]).scatter_(1, own, float("inf")).min(1).values
        sil = torch.nan_to_num((b - a) / torch.maximum(a, b))             # a = b = 0 (coincident points): 0, as sklearn
        s[r0:r1] = torch.where(n_own > 1, sil, torch.zeros_like(sil))     # alone in its cluster: 0
    return s, values, inv, counts


@torch.no_grad()
def silhouette_samples(x, labels, metric: str = "euclidean", row_block: Optional[int] = None):
    """The silhouette width of every row of the cloud x [N, P] (f32, device; P % 4 == 0, P <= 512) under the integer
    annotation labels [N] (any values, device or host; 2 <= distinct labels <= N - 1): f32 [N] on the device, sklearn's
    definition.  With D[i, g] = the sum of d(x_i, x_j) over the other points j of label g (ops.label_dist_sums - the
    N x N distances never leave the workgroups):

        a_i = D[i, own] / (n_own - 1),  b_i = min over the other labels of D[i, g] / n_g,  s_i = (b_i - a_i) / max(a_i, b_i)

    and 0 for a point alone in its cluster.  metric: "euclidean", "sqeuclidean" or "cosine" (1 - cos: the rows are
    L2-normalised first).  Queries go through in blocks of row_block rows against the whole cloud, so the [rows, G]
    sums stay bounded (default: about 256 MiB of them).  More than 512 distinct labels cost one walk per 512."""
    return _silhouette(x, labels, metric, row_block)[0]


def _subset(x, labels, sample_size, generator):
    if sample_size is None:
        return x, labels
    _check_cloud(x)
    N = x.shape[0]
    _args.int_in("sample_size", sample_size, 1, N, what="None or an int in [1, N]")
    labels = _args.labels_arg("labels", labels, N)
    gdev = generator.device if generator is not None else "cpu"
    idx = torch.randperm(N, generator=generator, device=gdev)[:sample_size]
    return x[idx.to(x.device)], labels[idx.to(labels.device)]


@torch.no_grad()
def silhouette_score(x, labels, metric: str = "euclidean", sample_size: Optional[int] = None, generator=None,
                     row_block: Optional[int] = None) -> float:
    """The mean of silhouette_samples, a Python float in [-1, 1].  sample_size: the score of one random subset of the rows,
    queries and keys alike, as sklearn does - torch.randperm(N, generator=generator)[:sample_size], drawn on the
    generator's device (the host without one)."""
    x, labels = _subset(x, labels, sample_size, generator)
    return float(_silhouette(x, labels, metric, row_block)[0].double().mean())


def _label_means(v, inv, counts):
    return torch.zeros(counts.shape[0], dtype=torch.float64, device=v.device).index_add_(0, inv, v.double()) / counts.double()


@torch.no_grad()
def silhouette_by_label(x, labels, metric: str = "euclidean", row_block: Optional[int] = None):
    """(label values [G] ascending, mean silhouette width per label f64 [G], counts int64 [G]), on x's device: how well
    each annotation value - a cell type, an RBP, a perturbation - is separated from the others in the embedding space.
    A label whose points sit inside another label's cloud comes out near or below 0: the collapse the reference's
    analyze_embedding_collapse looks for with mean cosine similarities inside hand-picked groups."""
    s, values, inv, counts = _silhouette(x, labels, metric, row_block)
    return values.to(s.device), _label_means(s, inv, counts), counts


def _centroid_stats(x, labels):
    """(centroids f64 [G, P], counts f64 [G], mean distance to the own centroid f64 [G], sum of squared distances to the
    own centroid (0-d f64), N): on the device the cluster sums come from ops.kmeans_step with the labels given and the
    N x P differences are f32; host tensors go through index_add_ in f64."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or not x.is_floating_point():
        raise TypeError("x must be a 2-D floating-point tensor")
    values, inv, counts = _relabel(x, labels)
    G, P = values.shape[0], x.shape[1]
    inv = inv.to(x.device)
    cnt = counts.to(x.device).double()
    if x.is_cuda:
        _check_cloud(x)
        if G > ops.KMEANS_MAX_K:
            raise ValueError(f"at most {ops.KMEANS_MAX_K} distinct labels, got {G}")
        x = x.detach().contiguous()
        sums = ops.kmeans_step(x, torch.zeros((G, P), dtype=torch.float32, device=x.device), labels=inv.int())[2].double()
        work = x
    else:
        work = x.detach().double()
        sums = torch.zeros((G, P), dtype=torch.float64).index_add_(0, inv, work)
    c = sums / cnt[:, None]
    d2 = (work - c.to(work.dtype)[inv]).square().sum(1).double()
    intra = torch.zeros(G, dtype=torch.float64, device=x.device).index_add_(0, inv, d2.sqrt()) / cnt
    return c, cnt, intra, d2.sum(), x.shape[0]


@torch.no_grad()
def davies_bouldin_score(x, labels) -> float:
    """The Davies-Bouldin index (1979) of the labeling, sklearn's conventions: with s_g the mean distance of label g's
    points to their centroid and m_gh the distance between centroids, the mean over g of max_{h != g} (s_g + s_h) / m_gh -
    lower is better, 0 the best.  Centroid pairs at distance 0 are left out of the maximum; all s_g or all m_gh zero
    gives 0.0.  x [N, P], device (f32, the limits of kmeans) or host (any float dtype); f64 glue on cluster sums."""
    c, _, intra, _, _ = _centroid_stats(x, labels)
    m = torch.cdist(c, c, compute_mode="donot_use_mm_for_euclid_dist")          # from the differences: an exact 0 diagonal
    if bool((intra.abs() <= 1e-8).all()) or bool((m.abs() <= 1e-8).all()):       # numpy.allclose(., 0) defaults
        return 0.0
    m = torch.where(m == 0, torch.full_like(m, float("inf")), m)
    return float(((intra[:, None] + intra[None, :]) / m).max(1).values.mean())


@torch.no_grad()
def calinski_harabasz_score(x, labels) -> float:
    """The Calinski-Harabasz index (1974), sklearn's conventions: (between-cluster dispersion / (G - 1)) / (within-cluster
    dispersion / (N - G)) - higher is better; 1.0 when the within-cluster dispersion is 0.  Inputs as
    davies_bouldin_score."""
    c, cnt, _, within, N = _centroid_stats(x, labels)
    G = c.shape[0]
    mean = (c * cnt[:, None]).sum(0) / cnt.sum()
    between = float((cnt * (c - mean).square().sum(1)).sum())
    within = float(within)
    return 1.0 if within == 0.0 else between * (N - G) / (within * (G - 1))


@torch.no_grad()
def label_separation(x, labels, metric: str = "euclidean") -> dict:
    """How well an annotation (cell type, RBP, perturbation) is separated in the embedding space x [N, P] (f32, device):
    {"silhouette": the mean width, "davies_bouldin", "calinski_harabasz": the two centroid-based scores (Euclidean
    whatever the metric), "silhouette_by_label": (label values, mean width per label, counts)}.  What the reference's
    config asks of a BiologicalMetrics it never defines (tong/configs/default.yaml: compute_biological_metrics)."""
    s, values, inv, counts = _silhouette(x, labels, metric, None)
    return {"silhouette": float(s.double().mean()),
            "davies_bouldin": davies_bouldin_score(x, labels),
            "calinski_harabasz": calinski_harabasz_score(x, labels),
            "silhouette_by_label": (values.to(s.device), _label_means(s, inv, counts), counts)}


@torch.no_grad()
def choose_n_clusters(x, candidates=range(2, 17), criterion: str = "silhouette", **kmeans_kw):
    """k-means for every k in candidates, scored: (best k, {k: score}, the KMeansResult of the best k).  criterion:
    "silhouette" (in the k-means metric) or "calinski_harabasz" - the highest wins - or "davies_bouldin" - the lowest;
    equal scores go to the smaller k.  A fit that leaves fewer than two clusters with points scores nan and cannot win.
    This is the check the reference's hard-coded KMeans(n_clusters=10) never had.  Keyword arguments go to kmeans()."""
    if criterion not in CRITERIA:
        raise ValueError(f"criterion must be one of {CRITERIA}, got {criterion!r}")
    candidates = sorted(set(int(k) for k in candidates))
    if not candidates or candidates[0] < 2:
        raise ValueError("candidates must be cluster counts of at least 2")
    sign = -1.0 if criterion == "davies_bouldin" else 1.0
    scores, best = {}, None
    for k in candidates:
        res = kmeans(x, k, **kmeans_kw)
        if int((res.counts > 0).sum()) < 2:
            scores[k] = float("nan")
            continue
        if criterion == "silhouette":
            scores[k] = silhouette_score(x, res.labels, kmeans_kw.get("metric", "euclidean"))
        else:
            scores[k] = (davies_bouldin_score if criterion == "davies_bouldin" else calinski_harabasz_score)(x, res.labels)
        if best is None or sign * scores[k] > sign * scores[best[0]]:
            best = (k, res)
    if best is None:
        raise ValueError("no candidate gave two clusters with points")
    return best[0], scores, best[1]
