"""A numpy restatement of clip_dplm_amd.cluster and of include/clipk.h: clipk_kmeans_step, in f64 and f32:
  * one Lloyd step - scores by the norm expansion as in the kernel, ties to the lower index, an empty cluster keeps its
    centre;
  * the full fit from a given init, run to its fixed point;
  * the adjusted Rand index by brute-force pair counting.
Everything works in the dtype of its inputs."""
import itertools
from types import SimpleNamespace

import numpy as np


def blobs(N, P, K, sep, seed):
    """(x f32 [N, P], truth int64 [N], centres f32 [K, P]): Gaussian blobs, centres ~ N(0, sep^2 I), unit noise."""
    rng = np.random.default_rng(seed)
    centres = (sep * rng.standard_normal((K, P))).astype(np.float32)
    truth = rng.integers(0, K, N)
    x = (centres[truth] + rng.standard_normal((N, P))).astype(np.float32)
    return x, truth.astype(np.int64), centres


def scores(x, c, nc=None):
    """score_ic = 2 <x_i, c_c> - nc_c, the form the kernel maximises (nc: |c_c|^2 unless given)."""
    if nc is None:
        nc = (c * c).sum(1)
    return 2 * (x @ c.T) - nc[None, :].astype(x.dtype)


def assign(x, c, nc=None):
    """(labels int64 [N], best [N], margin [N] = best - runner-up score, +inf with one centroid).  numpy's argmax takes
    the first of equal scores: the lower index."""
    s = scores(x, c, nc)
    labels = s.argmax(1)
    best = s[np.arange(len(x)), labels]
    if c.shape[0] == 1:
        return labels, best, np.full(len(x), np.inf)
    rest = s.copy()
    rest[np.arange(len(x)), labels] = -np.inf
    return labels, best, best - rest.max(1)


def segmented(x, labels, K):
    """(sums [K, P], counts int64 [K]) of the rows of x under labels, in x's dtype, rows added in rising order."""
    sums = np.zeros((K, x.shape[1]), dtype=x.dtype)
    np.add.at(sums, labels, x)
    return sums, np.bincount(labels, minlength=K)[:K]


def update(x, c, labels):
    """The new centroids: cluster means, an empty cluster keeps its centre."""
    sums, counts = segmented(x, labels, c.shape[0])
    new = c.copy()
    full = counts > 0
    new[full] = sums[full] / counts[full, None].astype(x.dtype)
    return new, counts


def fit(x, init, max_iter=300):
    """Lloyd from `init` to its fixed point (no label changes) or max_iter; labels, inertia and counts from a final
    assignment against the returned centroids."""
    c = init.astype(x.dtype).copy()
    prev, n_iter, converged = None, 0, False
    while n_iter < max_iter:
        labels, _, _ = assign(x, c)
        c, _ = update(x, c, labels)
        n_iter += 1
        if prev is not None and np.array_equal(labels, prev):
            converged = True
            break
        prev = labels
    labels, best, margin = assign(x, c)
    d2 = np.maximum((x * x).sum(1) - best, 0)       # the library's form: |x|^2 - max_c (2 <x, c> - |c|^2)
    counts = np.bincount(labels, minlength=c.shape[0])
    return SimpleNamespace(centroids=c, labels=labels, inertia=d2.sum(), d2=d2, n_iter=n_iter, converged=converged,
                           counts=counts, n_empty=int((counts == 0).sum()), margin=margin)


def ari_pairs(a, b):
    """The adjusted Rand index by counting, over all pairs of points, whether the two labelings put them together."""
    a, b = np.asarray(a), np.asarray(b)
    n11 = n10 = n01 = n00 = 0
    for i, j in itertools.combinations(range(len(a)), 2):
        sa, sb = a[i] == a[j], b[i] == b[j]
        n11 += sa and sb
        n10 += sa and not sb
        n01 += sb and not sa
        n00 += not sa and not sb
    if n10 == 0 and n01 == 0:
        return 1.0
    return 2.0 * (n11 * n00 - n10 * n01) / ((n11 + n10) * (n10 + n00) + (n11 + n01) * (n01 + n00))


def nmi_direct(a, b):
    """Mutual information over the arithmetic mean of the entropies, from the definition over label pairs."""
    a, b = np.asarray(a), np.asarray(b)
    n = len(a)
    ha = -sum((np.mean(a == g)) * np.log(np.mean(a == g)) for g in np.unique(a))
    hb = -sum((np.mean(b == h)) * np.log(np.mean(b == h)) for h in np.unique(b))
    if ha == 0 and hb == 0:
        return 1.0
    mi = 0.0
    for g in np.unique(a):
        for h in np.unique(b):
            pab = np.sum((a == g) & (b == h)) / n
            if pab > 0:
                mi += pab * np.log(pab / (np.mean(a == g) * np.mean(b == h)))
    return mi / (0.5 * (ha + hb))
