"""Plain numpy / Python restatements of clip_dplm_amd.paga's contract (its docstrings): the label-pair counts, the PAGA
v1.2 formulas in the stated order of roundings, Kruskal with the stated tie rule and dense modularity.  Loops, no
vectorised cleverness: these are what the tests compare the package against, on the host and on the device."""
import numpy as np

from diffusion_ref import knn_host  # noqa: F401  (the brute-force graph the host tests build their KNNGraphs from)

BLOB_SIZES = (60, 90, 120, 150, 180)


def counts_ref(idx, row_labels, G, key_labels=None):
    """int64 [G, G]: counts[a, b] = #{(i, t): row_labels[i] = a, 0 <= idx[i, t] < Ny, key_labels[idx[i, t]] = b}, only a, b
    in [0, G)."""
    idx = np.asarray(idx)
    row_labels = [int(v) for v in np.asarray(row_labels)]
    key_labels = row_labels if key_labels is None else [int(v) for v in np.asarray(key_labels)]
    Ny = len(key_labels)
    C = np.zeros((G, G), np.int64)
    for i in range(idx.shape[0]):
        a = row_labels[i]
        if not 0 <= a < G:
            continue
        for j in idx[i].tolist():
            if not 0 <= j < Ny:
                continue
            b = key_labels[j]
            if 0 <= b < G:
                C[a, b] += 1
    return C


def paga_ref(C, labels, G):
    """(ns int64 [G], expected f64 [G, G], connectivities f64 [G, G]) from the counts C and the labels: Python integers for
    the numerator, then one conversion and one division; one more division for the connectivity."""
    labels = [int(v) for v in np.asarray(labels)]
    ns = [sum(1 for v in labels if v == a) for a in range(G)]
    n = sum(ns)
    es = [int(sum(int(C[a, b]) for b in range(G))) for a in range(G)]
    expected, conn = np.zeros((G, G)), np.zeros((G, G))
    den = np.float64(max(n - 1, 1))
    for a in range(G):
        for b in range(G):
            if a == b:
                continue
            expected[a, b] = np.float64(es[a] * ns[b] + es[b] * ns[a]) / den
            sym = int(C[a, b]) + int(C[b, a])
            if sym == 0:
                conn[a, b] = 0.0
            elif expected[a, b] == 0:
                conn[a, b] = 1.0
            else:
                conn[a, b] = min(1.0, np.float64(sym) / expected[a, b])
    return np.array(ns, np.int64), expected, conn


def tree_ref(conn):
    """f64 [G, G]: Kruskal's maximum spanning forest over the pairs a < b with conn > 0, sorted by conn descending, ties by
    (a, b) ascending; the forest's edges carry conn, symmetric."""
    conn = np.asarray(conn, np.float64)
    G = conn.shape[0]
    edges = [(-conn[a, b], a, b) for a in range(G) for b in range(a + 1, G) if conn[a, b] > 0]
    edges.sort()
    comp = list(range(G))
    tree = np.zeros((G, G))
    for neg, a, b in edges:
        if comp[a] == comp[b]:
            continue
        old, new = comp[b], comp[a]
        comp = [new if c == old else c for c in comp]
        tree[a, b] = tree[b, a] = -neg
    return tree


def tree_edges(tree):
    tree = np.asarray(tree)
    return sorted((a, b) for a in range(tree.shape[0]) for b in range(a + 1, tree.shape[0]) if tree[a, b] > 0)


def modularity_ref(W, labels, G, resolution=1.0):
    """Q = sum_c [in_c / W - resolution (tot_c / W)^2] from the dense matrix W (SymGraph.to_dense()), over the entries whose
    row and column are both labelled in [0, G)."""
    W = np.asarray(W, np.float64)
    labels = [int(v) for v in np.asarray(labels)]
    N = len(labels)
    inn, tot = np.zeros(G), np.zeros(G)
    for i in range(N):
        if not 0 <= labels[i] < G:
            continue
        for j in range(N):
            if not 0 <= labels[j] < G:
                continue
            tot[labels[i]] += W[i, j]
            if labels[i] == labels[j]:
                inn[labels[i]] += W[i, j]
    total = tot.sum()
    return float(sum(inn[c] / total - resolution * (tot[c] / total) ** 2 for c in range(G)))


def blob_chain(seed, P=8, step=3.0):
    """Five Gaussian blobs of 60, 90, 120, 150 and 180 rows with unit noise, their centres `step` apart along the first
    axis: (x f32 [600, P], labels int64 [600]), rows in blob order."""
    rng = np.random.default_rng(seed)
    labels = np.repeat(np.arange(len(BLOB_SIZES)), BLOB_SIZES)
    x = rng.standard_normal((labels.shape[0], P))
    x[:, 0] += step * labels
    return x.astype(np.float32), labels.astype(np.int64)
