"""Exact t-SNE of embedding clouds on the device, without the N x N matrix.

The reference turns an embedding cloud into a picture in Visualizer.plot_embeddings (tong/utils/visualization.py): the
cloud goes to the host and through a library's TSNE(n_components=2).  Here the cloud stays on the device; the affinities
and the gradient are tile walks of csrc/tsne.hip (include/clipk.h: clipk_cond_entropy_sums, clipk_tsne_grad,
clipk_tsne_update has the formulae), exact - every pair enters every gradient step - and the N x N matrix is never
written.

    perplexity_bandwidths   the per-row Gaussian bandwidths beta_i with entropy log(perplexity): one minimum walk, then
                            `passes` walks of 8 candidates per row in a shrinking bracket on log2 beta, then one walk that
                            re-evaluates the chosen beta.  The narrowing is arithmetic on [N, 8] device tensors.
    tsne                    the descent with the defaults of the library the reference calls: early exaggeration 12 for
                            250 iterations at momentum 0.5, then momentum 0.8, delta-bar-delta gains, learning rate
                            max(N / 12 / 4, 50), PCA initialisation.  A fixed iteration count and no host read: the call
                            can be captured in a graph.
    embed_spaces            the maps of the reference's ['cell_emb', 'pert_emb', 'protein_emb'] - data, no plotting.
    knn_preservation        the mean overlap of the k nearest neighbours before and after: the cheap check that a map is
                            not noise.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional, Union

import torch

from . import _args, ops, retrieval

__all__ = ["perplexity_bandwidths", "tsne", "TSNEResult", "embed_spaces", "knn_preservation", "auto_learning_rate"]

METRICS = ("sqeuclidean", "cosine")
INITS = ("pca", "random")
SPACES = ("cell_emb", "pert_emb", "protein_emb")       # the reference's plot_embeddings, in its order
CANDIDATES = 8                                           # per row and walk: ops.TSNE_MAX_B
BRACKET_OCTAVES = 20.0                                   # the first bracket: +- this many octaves around 1 / mean(d - m)


def check_cloud(x, perplexity, metric) -> int:
    """The argument errors of a cloud to calibrate, in this order: the walks' limits on x, 0 < perplexity < N - 1, the
    metric.  Returns N."""
    _args.check_cloud(x, min_rows=ops.TSNE_MIN_N, max_width=ops.TSNE_MAX_P)
    N = x.shape[0]
    if isinstance(perplexity, bool) or not isinstance(perplexity, (int, float)):
        raise ValueError(f"perplexity must be a number, got {perplexity!r}")
    if not 0 < perplexity < N - 1:
        raise ValueError(f"perplexity must lie in (0, N - 1) = (0, {N - 1}), got {perplexity}")
    _args.check_metric(metric, METRICS)
    return N


def auto_learning_rate(N: int, early_exaggeration: float = 12.0) -> float:
    """learning_rate="auto": max(N / early_exaggeration / 4, 50)."""
    return max(N / early_exaggeration / 4.0, 50.0)


# ------------------------------------------------------------------------------------------------ calibration
def _entropy(beta, s0, s1):
    return torch.log(s0) + beta * s1 / s0


def calibrate(x, nx, perplexity, passes):
    """(beta, dmin, log_s0, entropy) of the prepared cloud.  The bracket [lo, hi] on log2 beta is held in f64: 40 / 9^8
    octaves is below the f32 spacing at 20."""
    N = x.shape[0]
    target = math.log(perplexity)
    dmin, _, _ = ops.cond_entropy_sums(x, nx=nx)
    # mean_{j != i} d_ij in closed form (the pair (i, i) contributes 0): (N nx_i + sum nx - 2 <x_i, sum x>) / (N - 1)
    xd = x.double()
    mean_d = (N * nx.double() + nx.double().sum() - 2.0 * (xd * xd.sum(0)).sum(1)) / (N - 1)
    spread = (mean_d - dmin.double()).clamp_min(torch.finfo(torch.float32).tiny)
    centre = -torch.log2(spread)
    lo, hi = centre - BRACKET_OCTAVES, centre + BRACKET_OCTAVES
    steps = torch.arange(CANDIDATES + 2, dtype=torch.float64, device=x.device) / (CANDIDATES + 1)
    for _ in range(passes):
        pts = lo[:, None] + (hi - lo)[:, None] * steps                   # [N, 10]: lo, the 8 candidates, hi
        betas = torch.exp2(pts[:, 1:-1]).float().contiguous()
        _, s0, s1 = ops.cond_entropy_sums(x, betas, shift=dmin, nx=nx)
        # H falls as beta grows: the candidates still above the target lie left of the crossing
        left = (_entropy(betas, s0, s1) > target).sum(1, keepdim=True)
        lo, hi = pts.gather(1, left).squeeze(1), pts.gather(1, left + 1).squeeze(1)
    beta = torch.exp2(0.5 * (lo + hi)).float().unsqueeze(1).contiguous()
    _, s0, s1 = ops.cond_entropy_sums(x, beta, shift=dmin, nx=nx)
    return beta.squeeze(1), dmin, torch.log(s0).squeeze(1), _entropy(beta, s0, s1).squeeze(1)


def perplexity_bandwidths(x, perplexity: float, passes: int = 8, metric: str = "sqeuclidean"):
    """(beta, dmin, log_s0, entropy), f32 [N] each: the bandwidth of every row of x [N, P] (f32, device) whose conditional
    distribution p_{j|i} = exp(-beta_i (d_ij - dmin_i)) / s0_i has entropy log(perplexity) nats, the row's smallest
    squared distance, log s0_i and the entropy reached.

    One minimum walk, `passes` walks with 8 geometric candidates per row inside a per-row bracket on log2 beta (first
    +-20 octaves around 1 / mean_j (d_ij - dmin_i); after each walk the ninth of it in which the entropy crosses the
    target), one walk at the chosen beta: passes + 2 walks, no host read.  Eight passes leave 40 / 9^8 octaves.
    A row whose nearest neighbour is repeated more often than the perplexity cannot reach the target: it ends at the
    upper end of its bracket, with finite values."""
    check_cloud(x, perplexity, metric)
    _args.int_in("passes", passes, 1)
    _args.need_device("t-SNE needs", x)
    x = _args.prepare(x, metric)
    return calibrate(x, (x * x).sum(1), perplexity, passes)


# ------------------------------------------------------------------------------------------------ the descent
@dataclasses.dataclass
class TSNEResult:
    """embedding f32 [N, 2]; kl_divergence: 0-d f32 device tensor, the KL value of `embedding` (with kl_every=k a 1-D
    tensor: the values before iterations k, 2k, ... and last the value of `embedding`); beta, entropy f32 [N] from the
    calibration; n_iter iterations run at learning_rate."""
    embedding: torch.Tensor
    kl_divergence: torch.Tensor
    beta: torch.Tensor
    entropy: torch.Tensor
    n_iter: int
    learning_rate: float


def pca_init(x):
    """The first two principal components of x [N, P], scaled so that the first has standard deviation 1e-4: f64 glue on
    the P x P covariance."""
    xc = x.double()
    xc = xc - xc.mean(0)
    _, vecs = torch.linalg.eigh(xc.T @ xc)                               # ascending eigenvalues
    y = xc @ vecs[:, [-1, -2]]
    return (y / y[:, 0].std(unbiased=False) * 1e-4).float().contiguous()


def _initial_map(x, init, generator):
    N = x.shape[0]
    if isinstance(init, torch.Tensor):
        return init.detach().clone().contiguous()
    if init == "pca":
        return pca_init(x)
    return 1e-4 * torch.randn((N, 2), generator=_args.generator_for(generator, x.device), dtype=torch.float32,
                              device=x.device)


def tsne(x, perplexity: float = 30.0, n_iter: int = 1000, early_exaggeration: float = 12.0, exaggeration_iters: int = 250,
         learning_rate: Union[str, float] = "auto", init="pca", generator: Optional[torch.Generator] = None,
         metric: str = "sqeuclidean", kl_every: Optional[int] = None) -> TSNEResult:
    """Exact t-SNE of x [N, P] (f32, device; P % 4 == 0, P <= 512) into two dimensions.

    The defaults are those of the reference's call: learning_rate "auto" = max(N / early_exaggeration / 4, 50); the
    attraction times early_exaggeration and momentum 0.5 for the first exaggeration_iters iterations, momentum 0.8 after;
    gains + 0.2 where update and gradient disagree in sign, x 0.8 otherwise, at least 0.01; init "pca" (the first two
    components, the first scaled to a standard deviation of 1e-4), "random" (1e-4 N(0, 1) under `generator`) or a tensor
    [N, 2].  metric "cosine": d = 1 - cos.  Every iteration is one walk over all pairs and one elementwise step; the count
    is fixed and nothing is read back, so the call can be captured in a graph (with a tensor or "random" init).
    kl_every=k also evaluates the KL value before iterations k, 2k, ...; the value of the returned map always is."""
    N = check_cloud(x, perplexity, metric)
    _args.int_in("n_iter", n_iter, 0)
    _args.int_in("exaggeration_iters", exaggeration_iters, 0)
    _args.int_in("kl_every", kl_every, 1, optional=True)
    if not float(early_exaggeration) >= 1.0:
        raise ValueError(f"early_exaggeration must be at least 1, got {early_exaggeration!r}")
    if isinstance(learning_rate, str):
        if learning_rate != "auto":
            raise ValueError(f"learning_rate must be 'auto' or a positive number, got {learning_rate!r}")
        lr = auto_learning_rate(N, float(early_exaggeration))
    else:
        lr = float(learning_rate)
        if not lr > 0:
            raise ValueError(f"learning_rate must be 'auto' or a positive number, got {learning_rate!r}")
    if isinstance(init, torch.Tensor):
        if init.dtype != torch.float32 or tuple(init.shape) != (N, 2):
            raise ValueError(f"init must be a float32 tensor of shape ({N}, 2)")
    elif init not in INITS:
        raise ValueError(f"init must be one of {INITS} or a tensor, got {init!r}")
    _args.need_device("t-SNE needs", x, init if isinstance(init, torch.Tensor) else None)

    x = _args.prepare(x, metric)
    nx = (x * x).sum(1)
    beta, dmin, log_s0, entropy = calibrate(x, nx, perplexity, 8)
    y = _initial_map(x, init, generator)
    update, gains = torch.zeros_like(y), torch.ones_like(y)
    z = torch.empty((), dtype=torch.float32, device=x.device)
    rows5 = torch.empty((N, 5), dtype=torch.float32, device=x.device)
    rows6 = torch.empty((N, 6), dtype=torch.float32, device=x.device)
    kls = []
    for it in range(n_iter):
        early = it < exaggeration_iters
        want_kl = kl_every is not None and it > 0 and it % kl_every == 0
        rows = ops.tsne_grad(x, y, beta, dmin, log_s0, nx=nx, want_kl=want_kl, out=rows6 if want_kl else rows5)
        _, kl, _ = ops.tsne_update(rows, y, update, gains, alpha=early_exaggeration if early else 1.0,
                                   momentum=0.5 if early else 0.8, lr=lr, want_kl=want_kl, z=z)
        if want_kl:
            kls.append(kl)
    rows = ops.tsne_grad(x, y, beta, dmin, log_s0, nx=nx, want_kl=True, out=rows6)
    _, kl, _ = ops.tsne_update(rows, want_kl=True, z=z)
    if kl_every is not None:
        kl = torch.stack(kls + [kl])
    return TSNEResult(y, kl, beta, entropy, n_iter, lr)


def embed_spaces(embeddings: dict, **kw) -> dict:
    """{space: TSNEResult} for the spaces of the reference's plot_embeddings that `embeddings` holds ('cell_emb',
    'pert_emb', 'protein_emb', in that order; an absent one is skipped, as there).  kw: the arguments of tsne."""
    return {name: tsne(embeddings[name], **kw) for name in SPACES if name in embeddings}


# ------------------------------------------------------------------------------------------------ is the map noise?
def _knn(x, k):
    """int64 [N, k]: the k nearest other rows of x [N, P] by Euclidean distance, nearest first.  argmax_j <x_i, x_j> -
    |x_j|^2 / 2 as one retrieval.topk search over rows widened by four columns (1, 0, 0, 0) / (-|x_j|^2 / 2, 0, 0, 0);
    k + 1 results, the row itself removed (or the last, where equal rows hid it)."""
    N, P = x.shape
    pad = (-P) % 4
    q = torch.zeros((N, P + pad + 4), dtype=torch.float32, device=x.device)
    q[:, :P] = x
    g = q.clone()
    q[:, P + pad] = 1.0
    g[:, P + pad] = -0.5 * (x * x).sum(1)
    _, idx = retrieval.topk(q, g, k + 1)
    other = idx != torch.arange(N, device=x.device)[:, None]
    keep = other & (other.cumsum(1) <= k)
    return idx[keep].view(N, k)


def knn_preservation(x, y2, k: int = 10, row_block: int = 4096) -> torch.Tensor:
    """The mean over the rows of |kNN_x(i) & kNN_y(i)| / k (0-d f32 device tensor): 1 for a map that keeps every
    neighbourhood, about k / N for a random one.  x [N, P] the cloud, y2 [N, 2] its map (f32, device), k <= 63 and
    k <= N - 2: two retrieval.topk searches."""
    if not (isinstance(x, torch.Tensor) and isinstance(y2, torch.Tensor)) or x.dim() != 2 or y2.dim() != 2:
        raise ValueError("x and y2 must be 2-D tensors")
    if x.shape[0] != y2.shape[0]:
        raise ValueError(f"x has {x.shape[0]} rows, y2 {y2.shape[0]}")
    _args.int_in("k", k, 1, min(63, x.shape[0] - 2), what="an int in [1, min(63, N - 2)]")
    if x.dtype != torch.float32 or y2.dtype != torch.float32 or not (x.is_cuda and y2.is_cuda):
        raise ValueError("x and y2 must be float32 device tensors")
    a, b = _knn(x.detach(), k), _knn(y2.detach(), k)
    hits = torch.zeros((), dtype=torch.float64, device=x.device)
    for r0 in range(0, a.shape[0], row_block):
        hits += (a[r0:r0 + row_block, :, None] == b[r0:r0 + row_block, None, :]).sum()
    return (hits / (a.shape[0] * k)).float()
