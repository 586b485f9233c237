"""Restatements for the k-nearest-neighbour tests (not a test module): the total order of clipk_sim_knn with eligibility
and the cursor, the graph of neighbors.knn_graph, kBET with scipy's chi-square tail, and the published LISI's per-row loop.

Order: z descending, equal z by the lower key index.  A key is eligible for row i when it is not i + diag_offset
(diag_offset >= 0) and lies strictly after the cursor (after_s[i], after_i[i]) in that order.  Unfilled slots: (-inf, -1)."""
import math

import numpy as np
import torch


def select(z, k, diag_offset=-1, after=None):
    """(z_sel [M, k] in z's dtype as f64, idx int64 [M, k]) from the scores z [M, Ny] (f64, exact for the callers' inputs)."""
    z = z.double()
    M, Ny = z.shape
    j = torch.arange(Ny, device=z.device)[None, :]
    ok = torch.ones_like(z, dtype=torch.bool)
    if diag_offset >= 0:
        ok &= j != (torch.arange(M, device=z.device)[:, None] + diag_offset)
    if after is not None:
        a_s, a_i = after[0].double()[:, None], after[1][:, None]
        ok &= (z < a_s) | ((z == a_s) & (j > a_i))
    key = torch.where(ok, -z, torch.full_like(z, math.inf))
    skey, order = torch.sort(key, dim=1, stable=True)                    # ascending -z, equal z: the lower index first
    if k > Ny:
        pad = k - Ny
        skey = torch.cat([skey, torch.full((M, pad), math.inf, dtype=skey.dtype, device=z.device)], 1)
        order = torch.cat([order, torch.zeros((M, pad), dtype=order.dtype, device=z.device)], 1)
    skey, order = skey[:, :k], order[:, :k]
    empty = torch.isinf(skey) & (skey > 0)
    return torch.where(empty, torch.full_like(skey, -math.inf), -skey), torch.where(empty, torch.full_like(order, -1), order)


def scores(x, y, scale=1.0, bias=None):
    """z [Mx, Ny] in f64: scale * <x, y> + bias."""
    z = (x.double() @ y.double().t()) * scale
    return z if bias is None else z + bias.double()[None, :]


def sim_knn(x, y, k, scale=None, bias=None, diag_offset=-1, after=None):
    """ops.sim_knn restated in torch, for inputs whose z is exact in f32 (grid clouds): (scores f32 [Mx, k], idx [Mx, k])."""
    zs, idx = select(scores(x, y, 1.0 if scale is None else scale, bias), k, diag_offset, after)
    return zs.float(), idx


def pair_sqdist(x, y, idx, block=256):
    """f64 [M, k] from the differences; idx -1 gives +inf."""
    x, y = x.double(), y.double()
    out = []
    for r0 in range(0, x.shape[0], block):
        i = idx[r0:r0 + block]
        d = ((x[r0:r0 + block, None, :] - y[i.clamp(min=0)]) ** 2).sum(-1)
        out.append(torch.where(i < 0, torch.full_like(d, math.inf), d))
    return torch.cat(out)


def knn_graph(x, k, y=None):
    """(idx int64 [M, k], sqdist f64 [M, k], z f64 [M, Ny]) of the Euclidean graph: z = <x, y> - |y|^2 / 2 in f64, y=None
    searches x with the row itself excluded by index."""
    ys = x if y is None else y
    z = scores(x, ys, 1.0, -0.5 * (ys.double() ** 2).sum(1))
    _, idx = select(z, k, 0 if y is None else -1)
    return idx, pair_sqdist(x, ys, idx), z


def kbet_ref(indices, labels, num_labels, alpha=0.05):
    """(stat [N], pvalue [N], rejection rate) with scipy's chi-square tail; labels 0..G-1 (numpy), empty labels dropped."""
    from scipy.stats import chi2
    indices, labels = np.asarray(indices), np.asarray(labels)
    N, k = indices.shape
    share = np.bincount(labels, minlength=num_labels) / N
    full = np.nonzero(share > 0)[0]
    dof = len(full) - 1
    stat = np.zeros(N)
    for i in range(N):
        n = np.bincount(labels[indices[i]], minlength=num_labels)
        stat[i] = sum((n[g] - k * share[g]) ** 2 / (k * share[g]) for g in full)
    p = chi2.sf(stat, dof)
    return stat, p, float(np.mean(p < alpha))


def _hbeta(d, beta):
    p = np.exp(-d * beta)
    sp = p.sum()
    if sp == 0:
        return 0.0, np.zeros_like(p)
    return math.log(sp) + beta * float((d * p).sum()) / sp, p / sp


def lisi_knn_ref(distances, neighbour_labels, num_labels, perplexity=30.0, tol=1e-5):
    """The published per-row loop, literally: distances f64 [N, k] (unsquared), neighbour_labels int [N, k]."""
    distances, neighbour_labels = np.asarray(distances, dtype=np.float64), np.asarray(neighbour_labels)
    N = distances.shape[0]
    logu = math.log(perplexity)
    out = np.zeros(N)
    for i in range(N):
        d = distances[i]
        beta, betamin, betamax = 1.0, -math.inf, math.inf
        h, p = _hbeta(d, beta)
        hdiff, tries = h - logu, 0
        while abs(hdiff) >= tol and tries < 50:
            if hdiff > 0:
                betamin = beta
                beta = beta * 2 if not math.isfinite(betamax) else (beta + betamax) / 2
            else:
                betamax = beta
                beta = beta / 2 if not math.isfinite(betamin) else (beta + betamin) / 2
            h, p = _hbeta(d, beta)
            hdiff = h - logu
            tries += 1
        if h == 0:
            simpson = -1.0
        else:
            simpson = sum(float(p[neighbour_labels[i] == g].sum()) ** 2 for g in range(num_labels))
        out[i] = 1.0 / simpson
    return out
