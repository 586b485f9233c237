"""A numpy restatement of include/clipk.h: clipk_label_dist_sums and of the labeling scores of clip_dplm_amd.cluster,
in the dtype it is given:
  * the per-label distance sums by the norm expansion as in the kernel, the diagonal term dropped (never formed);
  * the same sums from direct differences in f64;
  * the silhouette widths, the Davies-Bouldin and the Calinski-Harabasz scores, each from its definition."""
import numpy as np

METRICS = ("euclidean", "sqeuclidean", "cosine")


def distances(x, y, metric):
    """[Mx, Ny] by the kernel's formulae, in x's dtype: the norm expansion clamped at 0 (cosine: 1 - <x, y>, unit rows)."""
    s = x @ y.T
    if metric == "cosine":
        return np.maximum(1 - s, 0)
    d2 = np.maximum((x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2 * s, 0)
    return np.sqrt(d2) if metric == "euclidean" else d2


def distances_direct(x, y, metric):
    """[Mx, Ny] in f64 from the differences x_i - y_j (cosine: 1 - <x, y> of the unit rows given, clamped as the kernel
    does: the expansion is the definition there)."""
    x, y = x.astype(np.float64), y.astype(np.float64)
    if metric == "cosine":
        return np.maximum(1 - x @ y.T, 0)
    d2 = np.zeros((x.shape[0], y.shape[0]))
    for i in range(x.shape[0]):
        d2[i] = ((x[i][None, :] - y) ** 2).sum(1)
    return np.sqrt(d2) if metric == "euclidean" else d2


def sums_of(d, labels, G, diag_offset):
    """out[i, g] = sum of d[i, j] over labels[j] == g, j != i + diag_offset; a label outside [0, G) joins no column."""
    Mx, Ny = d.shape
    d = d.copy()
    if diag_offset >= 0:
        i = np.arange(Mx)
        j = i + diag_offset
        ok = j < Ny
        d[i[ok], j[ok]] = 0                          # the term is dropped
    labels = np.asarray(labels)
    out = np.zeros((Mx, G), dtype=d.dtype)
    for g in range(G):
        out[:, g] = d[:, labels == g].sum(1)
    return out


def label_dist_sums(x, y, labels, G, metric="euclidean", diag_offset=-1):
    return sums_of(distances(x, y, metric), labels, G, diag_offset)


def label_dist_sums_direct(x, y, labels, G, metric="euclidean", diag_offset=-1):
    return sums_of(distances_direct(x, y, metric), labels, G, diag_offset)


def diagonal_terms(x, metric):
    """What diag_offset = -1 adds to a cloud's own column: the kernel's formula at j == i, in x's dtype - 0 only up to the
    rounding of the product against the norms, and for the Euclidean distance the square root of that."""
    return np.diagonal(distances(x, x, metric)).copy()


def normalize(x):
    return x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-12)


def relabel(labels):
    values, inv = np.unique(np.asarray(labels), return_inverse=True)
    return values, inv, np.bincount(inv)


def silhouette_from_sums(D, inv, counts):
    """s_i = (b_i - a_i) / max(a_i, b_i) from D[i, g] (the own term dropped), 0 for a point alone in its cluster and for
    a_i = b_i = 0."""
    N = D.shape[0]
    n = counts.astype(D.dtype)
    rows = np.arange(N)
    a = D[rows, inv] / np.maximum(n[inv] - 1, 1)
    other = D / n[None, :]
    other[rows, inv] = np.inf
    b = other.min(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.nan_to_num((b - a) / np.maximum(a, b))
    s[counts[inv] == 1] = 0
    return s


def silhouette_samples(x, labels, metric="euclidean", direct=False):
    """The silhouette widths [N] in x's dtype (direct: the f64 distances from differences)."""
    _, inv, counts = relabel(labels)
    if metric == "cosine":
        x = normalize(x)
    f = label_dist_sums_direct if direct else label_dist_sums
    return silhouette_from_sums(f(x, x, inv, len(counts), metric, 0), inv, counts)


def silhouette_by_label(x, labels, metric="euclidean", direct=False):
    values, inv, counts = relabel(labels)
    s = silhouette_samples(x, labels, metric, direct)
    return values, np.array([s[inv == g].mean() for g in range(len(values))]), counts


def centroids(x, inv, G):
    return np.stack([x[inv == g].mean(0) for g in range(G)])


def davies_bouldin(x, labels):
    """mean_g max_{h != g} (s_g + s_h) / |c_g - c_h|, s_g = the mean distance of label g's points to their centroid;
    centroid pairs at distance 0 are left out, all-zero s or all-zero centroid distances give 0."""
    _, inv, counts = relabel(labels)
    G = len(counts)
    c = centroids(x, inv, G)
    s = np.array([np.sqrt(((x[inv == g] - c[g]) ** 2).sum(1)).mean() for g in range(G)])
    m = np.sqrt(((c[:, None, :] - c[None, :, :]) ** 2).sum(2))
    if np.allclose(s, 0) or np.allclose(m, 0):
        return 0.0
    best = np.zeros(G)
    for g in range(G):
        r = [(s[g] + s[h]) / m[g, h] for h in range(G) if h != g and m[g, h] > 0]
        best[g] = max(r) if r else 0.0
    return float(best.mean())


def calinski_harabasz(x, labels):
    """(sum_g n_g |c_g - mean|^2 / (G - 1)) / (sum_i |x_i - c_own|^2 / (N - G)); 1 when the denominator is 0."""
    _, inv, counts = relabel(labels)
    G, N = len(counts), len(x)
    c = centroids(x, inv, G)
    between = float((counts.astype(x.dtype) * ((c - x.mean(0)) ** 2).sum(1)).sum())
    within = float(((x - c[inv]) ** 2).sum())
    return 1.0 if within == 0 else between * (N - G) / (within * (G - 1))


def min_separation(x):
    """The smallest distance between two distinct rows, in f64 (by the expansion: at the scale the guard asks about,
    thousands of f32 roundings, the f64 roundings of the expansion do not show)."""
    d = distances(x.astype(np.float64), x.astype(np.float64), "euclidean")
    d[np.arange(len(x)), np.arange(len(x))] = np.inf
    return float(d.min())
