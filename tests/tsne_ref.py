"""Restatement of clip_dplm_amd.manifold and of the t-SNE entries of include/clipk.h in plain torch, the N x N matrices
materialised.

    d_ij    = |x_i - x_j|^2,  m_i = min_{j != i} d_ij
    p_{j|i} = exp(-beta_i (d_ij - m_i)) / s0_i,  s0_i = sum_{j != i} exp(-beta_i (d_ij - m_i))
    H_i     = log s0_i + beta_i s1_i / s0_i,  s1_i = sum_{j != i} (d_ij - m_i) exp(-beta_i (d_ij - m_i))
    P_ij    = (p_{j|i} + p_{i|j}) / (2N),  w_ij = 1 / (1 + |y_i - y_j|^2),  Z = sum_{i != j} w_ij
    grad_i  = 4 (alpha sum_j P_ij w_ij (y_i - y_j) - (1/Z) sum_j w_ij^2 (y_i - y_j))
    KL      = sum_{i != j} P_ij (log P_ij - log w_ij) + log Z,  0 log 0 = 0

The pair (i, i) is left out of every sum.  In float64 d comes from the coordinate differences and is the reference; in
float32 it comes from the norm expansion nx_i + nx_j - 2 <x_i, x_j> clamped at 0, the form the kernels use: the
yardstick for tolerances.  The search for beta has the pass structure of manifold.perplexity_bandwidths (a bracket on
log2 beta held in f64, eight candidates per pass evaluated in `dtype`).
"""
import math

import torch

F64 = torch.float64
CANDIDATES, BRACKET_OCTAVES = 8, 20.0


def sq_dists(x):
    """[N, N] squared distances of a cloud with itself: float64 from coordinate differences, other dtypes from the norm
    expansion clamped at 0."""
    if x.dtype == F64:
        rows = max(1, (1 << 24) // max(1, x.shape[0] * x.shape[1]))
        return torch.cat([((x[i:i + rows, None, :] - x[None, :, :]) ** 2).sum(-1) for i in range(0, len(x), rows)])
    nx = (x * x).sum(1)
    return (nx[:, None] + nx[None, :] - 2.0 * x @ x.T).clamp_min(0)


def off_diagonal(d):
    return ~torch.eye(d.shape[0], dtype=torch.bool, device=d.device)


def row_min(d):
    """m_i = min_{j != i} d_ij."""
    return d.masked_fill(~off_diagonal(d), math.inf).min(1).values


def entropy_sums(d, betas, shift):
    """(s0, s1) [N, B] for per-row candidates betas [N, B]: sums over j != i of exp(-beta t), t exp(-beta t), t = d - shift."""
    t = (d - shift[:, None])[:, :, None]                                  # [N, N, 1]
    e = torch.exp(-betas[:, None, :] * t).masked_fill(~off_diagonal(d)[:, :, None], 0.0)      # (exp may be inf there)
    return e.sum(1), (t * e).sum(1)


def entropy(betas, s0, s1):
    return torch.log(s0) + betas * s1 / s0


def mean_spread(x, dmin):
    """mean_{j != i} d_ij - m_i in f64, the mean in closed form."""
    N = x.shape[0]
    xd = x.double()
    nx = (xd * xd).sum(1)
    return ((N * nx + nx.sum() - 2.0 * (xd * xd.sum(0)).sum(1)) / (N - 1) - dmin.double()).clamp_min(
        torch.finfo(torch.float32).tiny)


def perplexity_bandwidths(x, perplexity, passes=8, dtype=F64, d=None):
    """(beta, dmin, log_s0, entropy) in `dtype`, and the final bracket (lo, hi) on log2 beta in f64."""
    x = x.to(dtype)
    d = sq_dists(x) if d is None else d
    dmin = row_min(d)
    centre = -torch.log2(mean_spread(x, dmin))
    lo, hi = centre - BRACKET_OCTAVES, centre + BRACKET_OCTAVES
    steps = torch.arange(CANDIDATES + 2, dtype=F64, device=x.device) / (CANDIDATES + 1)
    target = math.log(perplexity)
    for _ in range(passes):
        pts = lo[:, None] + (hi - lo)[:, None] * steps
        betas = torch.exp2(pts[:, 1:-1]).to(dtype)
        s0, s1 = entropy_sums(d, betas, dmin)
        left = (entropy(betas, s0, s1) > target).sum(1, keepdim=True)
        lo, hi = pts.gather(1, left).squeeze(1), pts.gather(1, left + 1).squeeze(1)
    beta = torch.exp2(0.5 * (lo + hi)).to(dtype)
    s0, s1 = entropy_sums(d, beta[:, None], dmin)
    return beta, dmin, torch.log(s0[:, 0]), entropy(beta[:, None], s0, s1)[:, 0], (lo, hi)


def conditional(d, beta, dmin, log_s0):
    """p_{j|i} [N, N] (row i: the distribution of point i), 0 on the diagonal."""
    return torch.exp(-beta[:, None] * (d - dmin[:, None]) - log_s0[:, None]).masked_fill(~off_diagonal(d), 0.0)


def joint(d, beta, dmin, log_s0):
    p = conditional(d, beta, dmin, log_s0)
    return (p + p.T) / (2.0 * d.shape[0])


def grad_rows(P, y):
    """rows [N, 6]: sum_j P w (y_i - y_j) (2), sum_j w^2 (y_i - y_j) (2), sum_j w, sum_j P (log P - log w)."""
    dy = y[:, None, :] - y[None, :, :]                                    # [N, N, 2]
    q = 1.0 + (dy * dy).sum(-1)
    w = off_diagonal(P) / q
    attr = ((P * w)[:, :, None] * dy).sum(1)
    rep = ((w * w)[:, :, None] * dy).sum(1)
    pos = P > 0
    kl = torch.where(pos, P * (torch.log(torch.where(pos, P, torch.ones_like(P))) + torch.log(q)), torch.zeros_like(P))
    return torch.cat([attr, rep, w.sum(1, keepdim=True), kl.sum(1, keepdim=True)], dim=1)


def gradient(rows, alpha=1.0):
    """(grad [N, 2], Z)."""
    Z = rows[:, 4].sum()
    return 4.0 * (alpha * rows[:, 0:2] - rows[:, 2:4] / Z), Z


def kl_value(rows):
    return rows[:, 5].sum() + torch.log(rows[:, 4].sum())


def update_step(grad, y, update, gains, momentum, lr):
    """The delta-bar-delta step: new (y, update, gains)."""
    inc = update * grad < 0
    gains = torch.where(inc, gains + 0.2, gains * 0.8).clamp_min(0.01)
    update = momentum * update - lr * gains * grad
    return y + update, update, gains


def auto_learning_rate(N, early_exaggeration=12.0):
    return max(N / early_exaggeration / 4.0, 50.0)


def descend(P, y0, n_iter, early_exaggeration=12.0, exaggeration_iters=250, lr=None, snapshots=()):
    """n_iter steps from y0 in P's dtype: (y, {iteration: (y, update, gains) before that iteration})."""
    lr = auto_learning_rate(P.shape[0], early_exaggeration) if lr is None else lr
    y = y0.to(P.dtype).clone()
    update, gains = torch.zeros_like(y), torch.ones_like(y)
    states = {}
    for it in range(n_iter):
        if it in snapshots:
            states[it] = (y.clone(), update.clone(), gains.clone())
        early = it < exaggeration_iters
        grad, _ = gradient(grad_rows(P, y), early_exaggeration if early else 1.0)
        y, update, gains = update_step(grad, y, update, gains, 0.5 if early else 0.8, lr)
    return y, states


def pca_init(x):
    xc = x.double() - x.double().mean(0)
    _, _, vt = torch.linalg.svd(xc, full_matrices=False)
    y = xc @ vt[:2].T
    return y / y[:, 0].std(unbiased=False) * 1e-4


def knn(z, k):
    """int64 [N, k]: the k nearest other rows by distance (f64 differences)."""
    d = sq_dists(z.double()).masked_fill(torch.eye(len(z), dtype=torch.bool, device=z.device), math.inf)
    return d.topk(k, dim=1, largest=False).indices


def knn_purity(y, labels, k=10):
    """The mean share of a point's k nearest neighbours in the map that carry its label."""
    return float((labels[knn(y, k)] == labels[:, None]).double().mean())


def knn_preservation(x, y, k=10):
    a, b = knn(x, k), knn(y, k)
    return float((a[:, :, None] == b[:, None, :]).sum()) / (len(x) * k)


def blobs(N, P, seed, n_blobs=4, spread=0.35):
    """(x f32 [N, P], labels int64 [N]): Gaussian blobs with centres N(0, 1), points at `spread` sigma, labels i % n."""
    g = torch.Generator().manual_seed(seed)
    centres = torch.randn(n_blobs, P, generator=g, dtype=F64)
    labels = torch.arange(N) % n_blobs
    return (centres[labels] + spread * torch.randn(N, P, generator=g, dtype=F64)).float(), labels


def cloud(N, P, seed):
    """A seeded f32 cloud with structure: blobs of spread 0.5, so that rows have near and far neighbours."""
    return blobs(N, P, seed, n_blobs=5, spread=0.5)[0]
