"""f64 numpy restatements of every definition of clip_dplm_amd.diffusion and of the arithmetic of clipk_csr_spmm_f64
(include/clipk.h), written from the definitions with plain loops - what the tests compare the product against.

numpy rounds every elementwise product and sum once and never fuses them, so csr_spmm_ref follows the kernel's stated
order operation by operation and reproduces its bits."""
import math

import numpy as np

SPMM_CHUNK = 64
UNIT_EPS = 1e-8
EPS = 2.0 ** -52


# ---- clipk_csr_spmm_f64 ---------------------------------------------------------------------------------------------
def csr_spmm_ref(indptr, indices, w, X, s=None, alpha=1.0, B=None, beta=0.0, C=None, gamma=0.0):
    """Y [N, m], bit for bit: chunk sums in ascending e from +0, partials in chunk order, the epilogue's stated order."""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    w, X = np.asarray(w, np.float64), np.asarray(X, np.float64)
    N, m = X.shape
    alpha, beta, gamma = np.float64(alpha), np.float64(beta), np.float64(gamma)
    Y = np.empty((N, m), np.float64)
    for i in range(N):
        r0, r1 = int(indptr[i]), int(indptr[i + 1])
        t = None
        for c0 in range(r0, max(r1, r0 + 1), SPMM_CHUNK):
            p = np.zeros(m, np.float64)
            for e in range(c0, min(c0 + SPMM_CHUNK, r1)):
                j = indices[e]
                if not 0 <= j < N:
                    continue
                coef = w[e] * s[j] if s is not None else w[e]
                p = p + coef * X[j]
            t = p if t is None else t + p
        r = s[i] * t if s is not None else t
        y = alpha * r
        if B is not None:
            y = y + beta * B[i]
        if C is not None:
            y = y + gamma * C[i]
        Y[i] = y
    return Y


def csr_spmm_torch(indptr, indices, w, x, s=None, alpha=1.0, b=None, beta=0.0, c=None, gamma=0.0, out=None):
    """A torch restatement of ops.csr_spmm for host tensors (the same value, not the same bits): what the host tests put in
    the place of the kernel to run the solver's torch logic."""
    import torch
    N = x.shape[0]
    rows = torch.searchsorted(indptr[1:].contiguous(), torch.arange(indices.shape[0]), right=True)
    cols = indices.long()
    coef = w if s is None else w * s[cols]
    t = torch.zeros_like(x).index_add_(0, rows, coef[:, None] * x[cols])
    y = alpha * (t if s is None else s[:, None] * t)
    if b is not None:
        y = y + beta * b
    if c is not None:
        y = y + gamma * c
    if out is not None:
        out.copy_(y)
        return out
    return y


# ---- connectivities -------------------------------------------------------------------------------------------------
def smooth_knn_ref(d):
    """(rho [N], sigma [N]) of UMAP's smooth_knn_dist on d f64 [N, k], row by row."""
    d = np.asarray(d, np.float64)
    N, k = d.shape
    target = math.log2(k + 1)
    gmean = d.mean()
    rho, sigma = np.zeros(N), np.zeros(N)
    for i in range(N):
        pos = d[i][d[i] > 0]
        rho[i] = pos.min() if pos.size else 0.0
        lo, hi, mid = 0.0, math.inf, 1.0
        for _ in range(64):
            psum = 0.0
            for j in range(k):
                x = d[i, j] - rho[i]
                psum += math.exp(-(x / mid)) if x > 0 else 1.0
            if abs(psum - target) < 1e-5:
                break
            if psum > target:
                hi = mid
                mid = (lo + hi) / 2
            else:
                lo = mid
                mid = mid * 2 if hi == math.inf else (lo + hi) / 2
        total = 0.0
        for j in range(k):                                                # in neighbour order
            total += d[i, j]
        sigma[i] = max(mid, 1e-3 * (total / k if rho[i] > 0 else gmean))
    return rho, sigma


def membership_ref(d):
    """a f64 [N, k]: 1 where d - rho <= 0, else exp(-(d - rho) / sigma); and (rho, sigma)."""
    d = np.asarray(d, np.float64)
    rho, sigma = smooth_knn_ref(d)
    a = np.ones_like(d)
    for i in range(d.shape[0]):
        for j in range(d.shape[1]):
            x = d[i, j] - rho[i]
            if x > 0:
                a[i, j] = math.exp(-(x / sigma[i]))
    return a, rho, sigma


def symmetrise_ref(idx, a):
    """(indptr int64 [N + 1], indices int32 [2 N k], weights f64 [2 N k]) of the fixed-size symmetrisation: the entries
    (i, j, a_ij) and (j, i, a_ij) sorted by (row, column); the first of two equal keys gets fl(fl(a + b) - fl(a b)), the
    second keeps its column with weight 0."""
    idx, a = np.asarray(idx, np.int64), np.asarray(a, np.float64)
    N, k = idx.shape
    ent = []
    for i in range(N):
        for t in range(k):
            j = int(idx[i, t])
            ent.append((i, j, a[i, t]))
            ent.append((j, i, a[i, t]))
    ent.sort(key=lambda r: (r[0], r[1]))
    rows = np.array([r[0] for r in ent], np.int64)
    cols = np.array([r[1] for r in ent], np.int32)
    vals = np.array([r[2] for r in ent], np.float64)
    wts = vals.copy()
    t = 0
    while t < len(ent):
        if t + 1 < len(ent) and rows[t] == rows[t + 1] and cols[t] == cols[t + 1]:
            wts[t] = (vals[t] + vals[t + 1]) - (vals[t] * vals[t + 1])
            wts[t + 1] = 0.0
            t += 2
        else:
            t += 1
    indptr = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=N), out=indptr[1:])
    return indptr, cols, wts


def dense_ref(indptr, indices, weights):
    N = len(indptr) - 1
    W = np.zeros((N, N))
    for i in range(N):
        for e in range(indptr[i], indptr[i + 1]):
            W[i, indices[e]] += weights[e]
    return W


def connectivities_ref(idx, d):
    """(indptr, indices, weights, a) from the graph's indices [N, k] and unsquared distances d [N, k]."""
    a, _, _ = membership_ref(d)
    return symmetrise_ref(idx, a) + (a,)


# ---- the transition matrix and its eigenpairs --------------------------------------------------------------------------
def transition_ref(W):
    """(T [N, N], s [N]): q = W 1, K = W / (q q^T), z = sqrt(K 1), T = K / (z z^T) = S W S with s = 1 / (q z)."""
    W = np.asarray(W, np.float64)
    q = W.sum(1)
    K = W / np.outer(q, q)
    z = np.sqrt(K.sum(1))
    return K / np.outer(z, z), 1.0 / (q * z)


def eigh_desc(T):
    lam, vec = np.linalg.eigh(T)
    return lam[::-1].copy(), vec[:, ::-1].copy()


def clusters(lam, n, tol_gap):
    """The first n reference eigenvalues (descending) cut into runs whose members lie within tol_gap of their neighbour:
    [(lo, hi, gap)] with gap = the distance of the run to the nearest reference eigenvalue outside it (lam holds at least
    n + 1 values)."""
    out, lo = [], 0
    for l in range(1, n + 1):
        if l == n or lam[l - 1] - lam[l] > tol_gap:
            gap = min(lam[lo - 1] - lam[lo] if lo else math.inf, lam[l - 1] - lam[l])
            out.append((lo, l, gap))
            lo = l
    return out


# ---- pseudotime ---------------------------------------------------------------------------------------------------------
def pseudotime_ref(lam, psi, roots, n_dcs=10):
    lam, psi = np.asarray(lam, np.float64), np.asarray(psi, np.float64)
    out = np.zeros((len(roots), psi.shape[0]))
    for r, root in enumerate(roots):
        acc = np.zeros(psi.shape[0])
        for l in range(min(n_dcs, lam.shape[0])):
            if lam[l] <= 1 - UNIT_EPS:
                wl = lam[l] / (1 - lam[l])
                acc += (wl * (psi[:, l] - psi[root, l])) ** 2
        d = np.sqrt(acc)
        out[r] = d / d.max()
    return out


def pseudotime_weights(lam, n_dcs=10):
    lam = np.asarray(lam, np.float64)
    return np.array([lam[l] / (1 - lam[l]) if l < n_dcs and lam[l] <= 1 - UNIT_EPS else 0.0 for l in range(len(lam))])


def average_ranks(v):
    v = np.asarray(v, np.float64)
    order = np.argsort(v, kind="stable")
    ranks = np.empty(len(v))
    t = 0
    while t < len(v):
        u = t
        while u + 1 < len(v) and v[order[u + 1]] == v[order[t]]:
            u += 1
        ranks[order[t:u + 1]] = (t + u) / 2
        t = u + 1
    return ranks


def spearman_ref(a, b):
    ra, rb = average_ranks(a), average_ranks(b)
    ra, rb = ra - ra.mean(), rb - rb.mean()
    return float((ra * rb).sum() / math.sqrt((ra * ra).sum() * (rb * rb).sum()))


# ---- clouds and host graphs ----------------------------------------------------------------------------------------------
def branch_cloud(N, P, seed, noise=0.05):
    """Three noisy branches from a common origin in P dimensions: (x f32 [N, P], t [N] the generating parameter - the
    distance from the origin along the branch, branch [N])."""
    rng = np.random.default_rng(seed)
    dirs = np.linalg.qr(rng.standard_normal((P, 3)))[0].T               # three orthonormal directions
    branch = np.arange(N) % 3
    t = rng.uniform(0.0, 1.0, N)
    x = t[:, None] * dirs[branch] + noise * rng.standard_normal((N, P)) / math.sqrt(P)
    return x.astype(np.float32), t, branch


def blob_cloud(N, P, seed, spread=0.3, distance=6.0, joined=1.0):
    """Four Gaussian blobs, the last one only `joined` away from the third (their graphs connect: three components):
    (x f32 [N, P], label [N])."""
    rng = np.random.default_rng(seed)
    centres = distance * rng.standard_normal((4, P)) / math.sqrt(P)
    step = rng.standard_normal(P)
    centres[3] = centres[2] + joined * step / np.linalg.norm(step)
    label = np.arange(N) % 4
    return (centres[label] + spread * rng.standard_normal((N, P))).astype(np.float32), label


def knn_host(x, k):
    """Brute-force graph of a small cloud in f64: (indices int64 [N, k], sqdist f32 [N, k]), nearest first, self excluded
    by index, ties by the lower index."""
    x = np.asarray(x, np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(2)
    np.fill_diagonal(d2, np.inf)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return idx.astype(np.int64), np.take_along_axis(d2, idx, 1).astype(np.float32)
