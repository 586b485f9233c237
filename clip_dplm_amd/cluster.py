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
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import torch

from . import ops

__all__ = ["kmeans", "KMeansResult", "init_centroids", "contingency", "adjusted_rand_index", "normalized_mutual_info",
           "cluster_agreement"]

METRICS = ("euclidean", "cosine")
INITS = ("k-means++", "random")


# ------------------------------------------------------------------------------------------------ seeding
def _generator_for(generator, device):
    """A generator on `device`: the one given, or one seeded by a draw from it when it lives elsewhere (a host
    generator with a device cloud) - a host-side draw, nothing is read back from the device."""
    if generator is None or generator.device.type == torch.device(device).type:
        return generator
    seed = int(torch.randint(2 ** 62, (1,), generator=generator, device=generator.device))
    return torch.Generator(device=device).manual_seed(seed)


def init_centroids(x, n_clusters: int, init="k-means++", generator=None):
    """n_clusters distinct rows of x [N, P] (any device) as the initial centroids [K, P].

    "random": the first K entries of a random permutation of the rows.  "k-means++" (Arthur & Vassilvitskii 2007): the
    first centre uniformly, each further one drawn with probability proportional to the squared distance to the nearest
    centre chosen so far (torch.multinomial under `generator`); a chosen row has distance exactly 0 and is not drawn
    again.  The D^2 update per centre is one pass over x, K passes in all, and nothing is read back."""
    if init not in INITS:
        raise ValueError(f"init must be one of {INITS} or a tensor, got {init!r}")
    N = x.shape[0]
    gen = _generator_for(generator, x.device)
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
        return _assign(_prepare(x, self.metric), self.centroids, self.metric)[0].long()


def _check_cloud(x, n_clusters: Optional[int] = None):
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
    if n_clusters is not None:
        if isinstance(n_clusters, bool) or not isinstance(n_clusters, int):
            raise TypeError(f"n_clusters must be an int, got {n_clusters!r}")
        if not 1 <= n_clusters <= min(x.shape[0], ops.KMEANS_MAX_K):
            raise ValueError(f"n_clusters must be in [1, min(N, {ops.KMEANS_MAX_K})], got {n_clusters} for N = {x.shape[0]}")


def _check_args(x, n_clusters, init, n_init, max_iter, tol, check_every, metric):
    """Every argument error of kmeans(), raised before anything is launched."""
    _check_cloud(x, n_clusters)
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    if isinstance(init, torch.Tensor):
        if init.dtype != torch.float32:
            raise TypeError(f"init must be float32, got {init.dtype}")
        if init.shape != (n_clusters, x.shape[1]):
            raise ValueError(f"init must have shape ({n_clusters}, {x.shape[1]}), got {tuple(init.shape)}")
    elif init is not None and init not in INITS:
        raise ValueError(f"init must be one of {INITS} or a tensor, got {init!r}")
    for name, v, lo in (("n_init", n_init, 1), ("max_iter", max_iter, 0), ("check_every", check_every, 1)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"{name} must be an int, got {v!r}")
        if v < lo:
            raise ValueError(f"{name} must be at least {lo}, got {v}")
    if tol is not None and not float(tol) >= 0:
        raise ValueError(f"tol must be None or a non-negative number, got {tol!r}")
    if not x.is_cuda or (isinstance(init, torch.Tensor) and not init.is_cuda):
        raise ValueError("kmeans needs device tensors (there is no CPU fallback)")


def _prepare(x, metric):
    x = x.detach().contiguous()
    return torch.nn.functional.normalize(x, dim=1) if metric == "cosine" else x


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
    x = _prepare(x, metric)
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
def _labels_arg(name, t):
    if not isinstance(t, torch.Tensor) or t.is_floating_point() or t.is_complex() or t.dtype == torch.bool:
        raise TypeError(f"{name} must be an integer tensor")
    if t.dim() != 1:
        raise ValueError(f"{name} must be 1-D, got shape {tuple(t.shape)}")
    return t.long()


def contingency(labels_a, labels_b):
    """int64 [Ga, Gb]: entry (g, h) counts the points with labels_a == g and labels_b == h (non-negative integer labels
    [n], device or host; Ga, Gb = the largest label + 1).  One torch.bincount over the pair index."""
    a, b = _labels_arg("labels_a", labels_a), _labels_arg("labels_b", labels_b)
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
def cluster_agreement(a, b, n_clusters: int = 10, labels=None, **kmeans_kw) -> dict:
    """The reference's analyze_embedding_alignment: k-means with n_clusters on each of the paired clouds a [N, Pa] and
    b [N, Pb] (row i of both is one sample), then {"ari", "nmi"} between the two labelings, Python floats.  labels (an
    integer annotation [N], e.g. the cell types): also "ari_a_vs_labels", "nmi_a_vs_labels", "ari_b_vs_labels",
    "nmi_b_vs_labels".  Keyword arguments go to kmeans()."""
    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise TypeError(f"{name} must be a 2-D tensor")
    if a.shape[0] != b.shape[0]:
        raise ValueError(f"the clouds are paired row by row, got {a.shape[0]} and {b.shape[0]} rows")
    if labels is not None:
        labels = _labels_arg("labels", labels)
        if labels.shape[0] != a.shape[0]:
            raise ValueError(f"labels has {labels.shape[0]} entries for {a.shape[0]} rows")
    la, lb = kmeans(a, n_clusters, **kmeans_kw).labels, kmeans(b, n_clusters, **kmeans_kw).labels
    out = {"ari": adjusted_rand_index(la, lb), "nmi": normalized_mutual_info(la, lb)}
    if labels is not None:
        labels = labels.to(la.device)
        for name, l in (("a", la), ("b", lb)):
            out[f"ari_{name}_vs_labels"] = adjusted_rand_index(l, labels)
            out[f"nmi_{name}_vs_labels"] = normalized_mutual_info(l, labels)
    return out
