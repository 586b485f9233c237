"""Restatement of clip_dplm_amd.mixing and of clipk_label_kernel_sums (include/clipk.h) in plain torch, the N x N weights
materialised.

    w_ij      = exp(-beta_i (d_ij - shift_i)),  the pair j = i + diag_offset left out
    out[i, g] = sum_{j : label_j = g} w_ij        mass_i = sum_g out[i, g]        sumsq_i = sum_g out[i, g]^2
    LISI_i    = mass_i^2 / sumsq_i = 1 / sum_g p_i(g)^2,  p_i(g) = out[i, g] / mass_i
    vote_i    = arg max_g out[i, g] (equal values: the lower g),  confidence_i = max_g out[i, g] / mass_i

In float64 d comes from the coordinate differences and is the reference; in float32 it comes from the norm expansion
clamped at 0, the form the kernel uses: the yardstick for tolerances (tests/tsne_ref.py: sq_dists).  beta and shift come
from tsne_ref.perplexity_bandwidths - the t-SNE conditional distribution over the whole cloud.  lisi_knn is the variant
truncated to each row's k nearest neighbours (the published implementation's k = 3 x perplexity), calibrated by the same
pass structure on the truncated rows; at k = N - 1 it is the exact definition again.
"""
import math

import torch

import tsne_ref
from tsne_ref import blobs, cloud, perplexity_bandwidths, sq_dists  # noqa: F401  (re-exported for the tests)

F64 = torch.float64


def weights(d, beta, shift, diag_offset=0):
    """w [Mx, Ny] in d's dtype; row i's key i + diag_offset is left out (diag_offset = -1: none)."""
    w = torch.exp(-beta[:, None] * (d - shift[:, None]))
    if diag_offset >= 0:
        i = torch.arange(d.shape[0], device=d.device)
        keep = i + diag_offset < d.shape[1]
        w[i[keep], i[keep] + diag_offset] = 0.0
    return w


def one_hot(labels, G, dtype):
    """[Ny, G]; a label outside [0, G) belongs to no column."""
    labels = labels.long()
    ok = (labels >= 0) & (labels < G)
    h = torch.zeros((labels.shape[0], G), dtype=dtype, device=labels.device)
    h[ok.nonzero()[:, 0], labels[ok]] = 1.0
    return h


def label_sums(w, labels, G):
    """out [Mx, G] = w @ one-hot."""
    return w @ one_hot(labels.to(w.device), G, w.dtype)


def stats(out):
    """(mass, sumsq, top, best): top the lowest label among the row's largest masses."""
    best = out.max(1).values
    G = out.shape[1]
    pos = torch.arange(G, device=out.device)[None, :].expand_as(out)
    top = torch.where(out == best[:, None], pos, torch.full_like(pos, G)).min(1).values
    return out.sum(1), (out * out).sum(1), top, best


def simpson(out):
    """sum_g p_g^2 per row."""
    p = out / out.sum(1, keepdim=True)
    return (p * p).sum(1)


def lisi_from_sums(out):
    mass, sumsq, _, _ = stats(out)
    return mass * mass / sumsq


def vote(out):
    """(predicted position, confidence): the leave-one-out kernel vote (the own row is not in out)."""
    mass, _, top, best = stats(out)
    return top, best / mass


def relabel(labels):
    """(values ascending, positions in 0..G-1)."""
    values, inv = torch.unique(labels, return_inverse=True)
    return values, inv


def label_sums_exact(x, labels, perplexity, dtype=F64, d=None, G=None):
    """out [N, G] of the cloud against itself in `dtype` with the restatement's own calibration in that dtype."""
    x = x.to(dtype)
    d = sq_dists(x) if d is None else d
    beta, dmin, _, _, _ = perplexity_bandwidths(x, perplexity, dtype=dtype, d=d)
    if G is None:
        _, labels = relabel(labels)
        G = int(labels.max()) + 1
    return label_sums(weights(d, beta, dmin), labels, G)


def lisi(x, labels, perplexity, dtype=F64, d=None):
    return lisi_from_sums(label_sums_exact(x, labels, perplexity, dtype, d))


def prepare(x, metric, dtype=F64):
    """Rows whose squared distances are the metric (manifold._prepare)."""
    x = x.to(dtype)
    return torch.nn.functional.normalize(x, dim=1) * math.sqrt(0.5) if metric == "cosine" else x


# ------------------------------------------------------------------------------------------------ kNN truncation
def lisi_knn(x, labels, perplexity, k):
    """LISI in f64 with every row's neighbourhood truncated to its k nearest other rows, the bandwidth calibrated on those
    k alone (the pass structure of tsne_ref.perplexity_bandwidths, the first bracket around the whole cloud's spread)."""
    x = x.double()
    N = x.shape[0]
    d = sq_dists(x).masked_fill(torch.eye(N, dtype=torch.bool, device=x.device), math.inf)
    dk, idx = d.topk(k, dim=1, largest=False)
    dmin = dk[:, 0]
    centre = -torch.log2(tsne_ref.mean_spread(x, dmin))
    lo, hi = centre - tsne_ref.BRACKET_OCTAVES, centre + tsne_ref.BRACKET_OCTAVES
    steps = torch.arange(tsne_ref.CANDIDATES + 2, dtype=F64, device=x.device) / (tsne_ref.CANDIDATES + 1)
    t = (dk - dmin[:, None])[:, :, None]
    for _ in range(8):
        pts = lo[:, None] + (hi - lo)[:, None] * steps
        betas = torch.exp2(pts[:, 1:-1])
        e = torch.exp(-betas[:, None, :] * t)
        left = (tsne_ref.entropy(betas, e.sum(1), (t * e).sum(1)) > math.log(perplexity)).sum(1, keepdim=True)
        lo, hi = pts.gather(1, left).squeeze(1), pts.gather(1, left + 1).squeeze(1)
    beta = torch.exp2(0.5 * (lo + hi))
    w = torch.exp(-beta[:, None] * (dk - dmin[:, None]))
    _, pos = relabel(labels)
    G = int(pos.max()) + 1
    out = torch.zeros((N, G), dtype=F64, device=x.device).scatter_add_(1, pos.to(x.device)[idx], w)
    return lisi_from_sums(out)


# ------------------------------------------------------------------------------------------------ shared test inputs
U = 2.0 ** -24


def column_bounds(o64, o32):
    """The tolerance rule of tests/test_gpu_tsne.py::_close per label column: 8 x the f32 restatement's deviation from the
    f64 one, at least 64 * 2^-24 x the column's magnitude."""
    o64, o32 = o64.double().cpu(), o32.double().cpu()
    return torch.maximum(8.0 * (o32 - o64).abs().max(0).values, 64.0 * U * o64.abs().max(0).values)


def decided_rows(o64, o32):
    """bool [Mx]: the rows whose two largest f64 masses differ by more than twice the bound - there a kernel inside the
    column bounds must find the f64 arg max.  The bound of a row is the largest of the column bounds: whichever two
    columns hold its largest masses, neither moves by more.  One label: every row is decided."""
    if o64.shape[1] < 2:
        return torch.ones(o64.shape[0], dtype=torch.bool)
    two = o64.double().cpu().topk(2, dim=1).values
    return (two[:, 0] - two[:, 1]) > 2.0 * float(column_bounds(o64, o32).max())


def vote_case(N, P, G, seed):
    """(x f32 [N, P], labels int64 [N]): G blobs, the labels follow the blobs, a tenth of them moved to another label."""
    x, labels = blobs(N, P, seed, n_blobs=G)
    if G > 1:
        g = torch.Generator().manual_seed(seed + 1)
        flip = torch.rand(N, generator=g) < 0.1
        labels = torch.where(flip, (labels + torch.randint(1, G, (N,), generator=g)) % G, labels)
    return x, labels


def calibrated(x, perplexity, d64):
    """The f64 restatement's (beta, dmin) rounded to f32: what kernel and both restatements are given in the tests of the
    walk, so that all three see the same inputs."""
    beta, dmin, _, _, _ = perplexity_bandwidths(x, perplexity, d=d64)
    return beta.float(), dmin.float()


def case_perplexity(N):
    """min(30, (N - 1) / 3), 1.5 for the three-point cloud (tests/test_gpu_tsne.py::_calibrated)."""
    return min(30.0, max(1.5, (N - 1) / 3.0))


# ------------------------------------------------------------------------------------------------ the scores
def median(values):
    v = values.double().flatten().sort().values
    n = v.shape[0]
    return float(0.5 * (v[(n - 1) // 2] + v[n // 2]))


def ilisi_scaled(med, G):
    return (med - 1.0) / (G - 1)


def clisi_scaled(med, G):
    return (G - med) / (G - 1)
