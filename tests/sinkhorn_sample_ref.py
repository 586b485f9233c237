"""Restatement of the plan sampler (include/clipk.h: clipk_sim_sample; ops.sim_sample; SinkhornResult.sample_targets) on
the materialised logits.

    z_ij = scale <x_i, y_j> + bias_j + G(seed, stream_i, j),   idx_i = argmax_j z_ij (the lower j of equal values)

The noise is the contract's: Philox4x32-10 keyed by the 64-bit seed, counter (j >> 2, stream lo, stream hi, 0), key j
takes output word j & 3 = w, U = ((w >> 9) + 0.5) 2^-23, G = -log(-log U).  `philox4x32_10` states the generator in numpy
(uint64 products of 32-bit factors are exact); `philox4x32_10_torch` is the same in int64 torch arithmetic, so that the
GPU tests can build the noise of their largest cases (1000 x 100003) where sinkhorn_ref's restatement already runs them,
on the device; the host tests hold the two against each other and against the known answer.

dtype=torch.float64 is the reference, dtype=torch.float32 on the same inputs the yardstick, as in sinkhorn_ref.py, whose
helpers (clouds, solves, plans) are imported, not restated.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

import sinkhorn_ref as ref  # noqa: F401  (re-exported: the tests take clouds and solves from it)

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on numpy arrays (or ints) of 32-bit counter words under the key (k0, k1): the four output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def _mulhilo_torch(m, c):
    """(high, low) 32 bits of m * c for 0 <= c < 2^32 in int64 arithmetic: the product is taken in two 16-bit halves of
    c, each below 2^48."""
    a, b = m * (c >> 16), m * (c & 0xFFFF)
    return (a + (b >> 16)) >> 16, ((a << 16) + b) & MASK


def philox4x32_10_torch(c0, c1, c2, c3, k0, k1):
    """philox4x32_10 on int64 torch tensors holding 32-bit words (any device)."""
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    for _ in range(10):
        hi0, lo0 = _mulhilo_torch(M0, c0)
        hi1, lo1 = _mulhilo_torch(M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def _split64(v):
    v = int(v) & ((1 << 64) - 1)
    return v & MASK, v >> 32


def words(seed, streams, Ny):
    """numpy: the 32-bit word of every (stream, key j < Ny), uint64 [n, Ny]."""
    k0, k1 = _split64(seed)
    streams = np.asarray([int(s) & ((1 << 64) - 1) for s in np.asarray(streams).reshape(-1).tolist()], dtype=np.uint64)
    ctr = np.arange((Ny + 3) // 4, dtype=np.uint64)[None, :]
    lo, hi = (streams & np.uint64(MASK))[:, None], (streams >> np.uint64(32))[:, None]
    out = philox4x32_10(ctr + 0 * lo, lo + 0 * ctr, hi + 0 * ctr, 0 * (ctr + lo), k0, k1)
    return np.stack(out, axis=2).reshape(len(streams), -1)[:, :Ny]


def uniforms(w):
    """numpy: U = ((w >> 9) + 0.5) 2^-23 in f64 (exactly representable in f32 too)."""
    return ((w >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel_numpy(seed, streams, Ny, dtype=np.float64):
    u = uniforms(words(seed, streams, Ny)).astype(dtype)
    return -np.log(-np.log(u))


def gumbel(seed, stream0, n, Ny, dtype, device=None):
    """torch [n, Ny]: G of the streams stream0 .. stream0 + n - 1, evaluated in `dtype` from the exact U."""
    k0, k1 = _split64(seed)
    s = [_split64(stream0 + i) for i in range(n)]
    lo = torch.tensor([v[0] for v in s], dtype=torch.int64, device=device)[:, None]
    hi = torch.tensor([v[1] for v in s], dtype=torch.int64, device=device)[:, None]
    ctr = torch.arange((Ny + 3) // 4, dtype=torch.int64, device=device)[None, :]
    z = torch.zeros_like(ctr + lo)
    out = philox4x32_10_torch(ctr + z, lo + z, hi + z, z, k0, k1)
    w = torch.stack(out, dim=2).reshape(n, -1)[:, :Ny]
    u = (((w >> 9) * 2 + 1).double() * 2.0 ** -24).to(dtype)            # exact in both types
    return -torch.log(-torch.log(u))


def logits(x, y, scale, bias, seed, stream0, dtype):
    """z [n, Ny] in `dtype` on the inputs' device: row k is stream stream0 + k."""
    x, y = x.to(dtype), y.to(dtype)
    z = scale * (x @ y.T)
    if bias is not None:
        z = z + bias.to(dtype)[None, :]
    return z + gumbel(seed, stream0, x.shape[0], y.shape[0], dtype, x.device)


def draw(x, y, scale, bias=None, seed=0, stream0=0, dtype=torch.float64, rows=128):
    """The draws of rows x (stream stream0 + row) in chunks: idx [n] (the first arg max), score [n] (its z) and gap [n],
    the distance from the best to the second best z (inf with a single key)."""
    idx, score, gap = [], [], []
    for i in range(0, x.shape[0], rows):
        z = logits(x[i:i + rows], y, scale, bias, seed, stream0 + i, dtype)
        top = torch.topk(z, min(2, z.shape[1]), dim=1)
        best = top.values[:, 0]
        # the lowest index among equal maxima, as the kernel's merge rule has it
        keys = torch.arange(z.shape[1], device=z.device)[None, :]
        first = torch.where(z == best[:, None], keys, z.shape[1]).amin(dim=1)
        idx.append(first)
        score.append(best)
        gap.append(best - top.values[:, 1] if z.shape[1] > 1 else torch.full_like(best, float("inf")))
    return SimpleNamespace(idx=torch.cat(idx), score=torch.cat(score), gap=torch.cat(gap))


def values_at(x, y, scale, bias, seed, streams, keys, dtype=torch.float64):
    """(z[row, key], max_j z[row, j]) for a few rows given one by one with their stream ids: what a disputed draw is
    judged by."""
    got, best = [], []
    for k in range(x.shape[0]):
        z = logits(x[k:k + 1], y, scale, bias, seed, int(streams[k]), dtype)[0]
        got.append(z[int(keys[k])])
        best.append(z.max())
    return torch.stack(got), torch.stack(best)


def chi_square(counts, probs):
    """Pearson's statistic of observed counts against expected probabilities (numpy, one row)."""
    counts, probs = np.asarray(counts, dtype=np.float64), np.asarray(probs, dtype=np.float64)
    e = counts.sum() * probs
    return float(((counts - e) ** 2 / e).sum())


def statistics_problem():
    """(x, y, eps, rows, seed) of the statistical check: 37 x 63 x 12, every row drawn 2000 times (draw k is stream k)."""
    x, y = ref.unit_clouds(37, 63, 12, 17)
    return x, y, 0.5, torch.arange(37).repeat(2000), 4242


def check_statistics(j, rows, y, r64):
    """The draws j [74000] (CPU, one per entry of rows) against the f64 plan r64 of statistics_problem(): the column
    counts against the plan's column marginal by Pearson's chi-square (62 degrees of freedom: mean 62, sd sqrt(124);
    threshold mean + 5 sd = 118), and the per-row mean of y[j] against the barycentric map within 5 standard errors of a
    mean of 2000 draws from the row's conditional.  Returns the two figures."""
    p = ref.plan(r64)
    cond = p / p.sum(1, keepdim=True)
    chi = chi_square(np.bincount(j.numpy(), minlength=63), (p.sum(0) / p.sum()).numpy())
    yy = y.double()
    bary = ref.barycentric_map(r64)
    sd = ((cond @ (yy * yy)) - bary * bary).clamp_min(0).sqrt()
    mean = torch.zeros(37, 12, dtype=torch.float64).index_add_(0, rows, yy[j]) / 2000
    worst = float(((mean - bary).abs() / (sd / math.sqrt(2000))).max())
    print(f"columns: chi-square {chi:.1f} at 62 degrees of freedom (threshold 118); per-row means: at most {worst:.2f} "
          f"standard errors from the barycentric map (threshold 5)")
    assert chi < 118 and worst < 5
    return chi, worst
