"""Plain f64 yardstick of the fused similarity + cross-entropy kernels (csrc/simce.hip, simce_tiled.hip, simce_hard.hip
and the headers they share), the seeded input families their tests use, the per-element error bounds they allow and a
Python restatement of the two split plans.  Pure torch on the CPU, on materialised logits; no kernel knowledge beyond
index arithmetic.  The class-aware and hard-negative definitions are tests/class_aware_ref.py and
tests/hard_negative_ref.py as they are.

tests/test_simce_ref_host.py pins this file against torch.autograd, holds a numpy-f32 stand-in inside every bound and
shows that every seeded fault falls outside them; tests/test_gpu_simce.py compares the HIP kernels with it.

The gradient is formed from the f32 lse_x / lse_y (cnt, coef) vectors it is handed, as the kernels form it, so a
comparison isolates the gradient kernel's own arithmetic.

Bounds (derived, none taken from GPU output).  u = 2^-24, keys K = [y | cache], D = x K^T, S = scale D.
  * bound_S[i,j] = (P + 2) u |scale| sum_p |x_ip| |K_jp|: an f32 fma chain of length P (the exact-f32 matrix pipe) plus
    the scale product.
  * bound_lse[i] = max_{j in the row's denominator} bound_S[i,j] + (C_EXP + C_LOG + 2) u (1 + |lse_i|): an LSE moves by
    at most the largest error of its exponents; then expf, the sum's and the final add's roundings, logf.
  * bound_pos = bound_S at the label.
  * With per direction d (row: w_row, lse_x; column: w_col, lse_y, batch keys only) E_d = [j in D] exp(s - lse_d), T_d its
    target and g = sum_d w_d (E_d - T_d) the gradient before inv_bg (and upstream) = ibg:
        err_g[i,j]  = sum_d w_d E_d (bound_S + C_EXP u (1 + |s - lse_d|))
        bound_dX[i,:] = |scale| ibg [ err_g |K| + (Nk + 2) u |g| |K| ] + u |dX|
        bound_dscale[i] = ibg [ sum_j err_g |D| + (Nk + 2) u sum_j |g| |D| + sum_j |g| bound_S / |scale| ] + u |dscale_i|
    (the exponent's error and its subtraction's rounding, expf; Nk accumulation steps and the factors; d scale
    multiplies g by the unscaled dot product, whose own error is bound_S / |scale|).
  * Class-aware target, tgt = (1 - eps) q + eps sd / n with sd = sum_{D} S (n terms), q = S[label] ("mask") or
    ss / c, ss = sum_{same} S (c terms): bound_sum(set) = sum_set bound_S + (#set + 2) u sum_set |S|,
        bound_tgt = (1 - eps) bound_q + eps bound_sum(D) / n + 3 u (|(1 - eps) q| + |eps sd / n|).
    cnt is a sum of ones below 2^24: exact.
  * ce_combine of n rows: (n + 4) u (w_row sum |lse_r - pos_r| + w_col sum |lse_c - pos_c|) / bg against the f64 value
    of the f32 vectors it was handed.
  * C_EXP = C_LOG = 2: ulp allowances for the device's expf / logf.  ASSUMPTION: the ROCm install this was written
    against carries no HIP math accuracy table.
  * Hard-negative: pos has bound_S.  The gradient is formed from the f32 coefficients (q, k1, k2) it is handed, and
    given them its bound closes like the plain one (hard_grad); the coefficients themselves are compared with the f64
    ones.  For lse_h and the coefficients q, k1, k2 the chain through A, C, log Ng (simce_hard.hip) is not closed
    here; hard_tol gives the tolerance tests/test_gpu_hard_negative_loss.py already uses for lse_h, 2e-5 (1 + 2 beta),
    scaled by max |S| / 14.2849: the error is in units of the logit's ulp.  The scaling is never below 1, so on the
    generic family the existing bar stands as it is.  An ASSUMPTION of the same kind, not a derivation.

The existing bars of the project stay as caps on the generic family (scale 14.2849): atol 2e-5 on lse / pos / tgt,
rtol 1e-4 with atol 1e-7 on dX; cap_stat and cap_dx take the smaller of the derived bound and the bar.
"""
import torch

import class_aware_ref as CA
import hard_negative_ref as HN

F64 = torch.float64
U = 2.0 ** -24
C_EXP = 2.0
C_LOG = 2.0
SCALE_A, SCALE_B, SCALE_C = 14.2849, 100.0, 16.0
BAR_STAT, BAR_DX_RTOL, BAR_DX_ATOL = 2e-5, 1e-4, 1e-7
TRI_PAIRS = ((0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1))


# ---------------------------------------------------------------------------------------------- split plans
def _cdiv(a, b):
    return -(-a // b)


def _splits(nqb, ntiles, problems=1):
    ks = max(1, min(_cdiv(512, nqb * max(problems, 1)), ntiles))
    tps = _cdiv(ntiles, ks)
    return tps, _cdiv(ntiles, tps)


def tiled_plan(Mx, Nk, problems=1):
    """csrc/cloud_tile.h: key_split_plan(Mx, Nk, 64, problems) -> (nqb, ntiles, tiles_per_split, ksplit)."""
    nqb, ntiles = _cdiv(Mx, 64), _cdiv(Nk, 64)
    return (nqb, ntiles) + _splits(nqb, ntiles, problems)


def first_gen_plan(Mx, Nk, P):
    """csrc/simce.hip: make_plan -> (nqb, ntiles, tiles_per_split, ksplit, NW, Pw), or None where it refuses (P % 4,
    P > 1024, or more than 160 KiB of LDS: NW = 8 waves with a 128-column slice each, P > 960)."""
    if Mx <= 0 or Nk <= 0 or P <= 0 or P % 4 or P > 1024:
        return None
    nw = 1
    while nw < 8 and _cdiv(P, nw) > 128:
        nw *= 2
    pw = (_cdiv(P, nw) + 7) & ~7
    if nw * 32 * (pw + 4) * 4 + nw * 1024 * 4 > 160 * 1024:
        return None
    nqb, ntiles = _cdiv(Mx, 32), _cdiv(Nk, 32)
    return (nqb, ntiles) + _splits(nqb, ntiles) + (nw, pw)


def grad_takes_tiled(Mx, Nk, P, mode):
    """csrc/simce.hip: use_tiled_grad under option simce_kernel = mode (0: default), for a P the first plan accepts."""
    if P > 512:
        return False
    if first_gen_plan(Mx, Nk, P)[5] % 32:
        return True
    return mode == 2 or (mode == 0 and Mx >= 64 and Nk >= 64)


def lse_takes_tiled(Mx, Nk, mode):
    return mode == 2 or (mode == 0 and Mx >= 64 and Nk >= 64)


# ---------------------------------------------------------------------------------------------- inputs
def unit_rows(n, P, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, P, generator=g, dtype=F64), dim=-1).float()


def eighths(n, P, seed):
    """Family C: entries from {-1, 0, 1} / 8.  With scale 16 every logit is a multiple of 1/4 below 2^7 in magnitude: an
    exact f32 in whatever order it is summed."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-1, 2, (n, P), generator=g).float() / 8.0).contiguous()


def plant_keys(Mx, Ny, Nc, off, tps):
    """Family B: (query row, key) pairs, so that the row's dominant key arrives at every level of the merge of the tiled
    pass with tps tiles per split: the diagonal; the first, second (third) tile of a split other than the diagonal's;
    key-wave 1 and lane half 1 of a tile; the cache segment; the last key of the list.  Rows are spread over both query
    halves of a block and several blocks; rows and keys are distinct and in range (a tiny shape keeps what fits)."""
    Nk = Ny + Nc
    rows = [r for r in (0, 5, 37, 63, 64, 101, Mx // 2, Mx - 2, Mx - 1, Mx // 3, 2 * Mx // 3, 17) if 0 <= r < Mx]
    rows = list(dict.fromkeys(rows))
    nsplit = _cdiv(_cdiv(Nk, 64), tps)

    def other_split(row, k):                                    # the k-th split that is not the row's diagonal's
        ds = (off + row) // (64 * tps)
        return [s for s in range(nsplit) if s != ds][k % max(1, nsplit - 1)] if nsplit > 1 else 0
    want = [lambda r: off + r,                                                       # the diagonal
            lambda r: other_split(r, 1) * tps * 64 + 3,                              # first tile of a split
            lambda r: (other_split(r, 2) * tps + 1) * 64 + 9,                        # second tile: rescale by ~e^-60
            lambda r: (other_split(r, 3) * tps + tps - 1) * 64 + 18,                 # last tile of a split
            lambda r: other_split(r, 0) * tps * 64 + 37,                             # key-wave 1, lane half 1
            lambda r: (other_split(r, 4) * tps + 1) * 64 + 60,                       # both, in a later tile
            lambda r: Ny + Nc // 2,                                                  # the cache segment
            lambda r: Nk - 1,                                                        # the last key (ragged tile)
            lambda r: off + r,                                                       # a second diagonal row
            lambda r: other_split(r, 5) * tps * 64 + 4]                              # lane half 1, key-wave 0
    out, used = [], set()
    for r, f in zip(rows, want):
        j = f(r)
        if 0 <= j < Nk and j not in used and (j < Ny or Nc > 0):
            used.add(j)
            out.append((r, j))
    return out


def pair_batch(family, Mx, Ny, Nc, off, P, seed, tps=1):
    """(a_g [max(Ny, off + Mx), P], b_g [Ny, P], cache [Nc, P] or None, scale): the row problem is a_g[off:off+Mx] against
    [b_g | cache], the column problem b_g against a_g.  B: a bitwise copy of the query in the key of plant_keys - the
    column problem's query b_g[j] then has its dominant key at off + row."""
    if family == "C":
        a, b = eighths(max(Ny, off + Mx), P, seed), eighths(Ny, P, seed + 1)
        return a, b, (eighths(Nc, P, seed + 2) if Nc else None), SCALE_C
    a, b = unit_rows(max(Ny, off + Mx), P, seed), unit_rows(Ny, P, seed + 1)
    cache = unit_rows(Nc, P, seed + 2) if Nc else None
    if family == "A":
        return a, b, cache, SCALE_A
    for r, j in plant_keys(Mx, Ny, Nc, off, tps):
        if j < Ny:
            b[j] = a[off + r]
        else:
            cache[j - Ny] = a[off + r]
    return a, b, cache, SCALE_B


def class_ids(pattern, n, seed=0):
    """None; "runs": runs of 300 from 0 (a whole key split of one class); "random"; "distinct"."""
    g = torch.Generator().manual_seed(seed)
    if pattern is None:
        return None
    if pattern == "runs":
        return (torch.arange(n) // 300).to(torch.int64)
    if pattern == "random":
        return torch.randint(0, max(1, n // 4), (n,), generator=g).to(torch.int64)
    return (torch.randperm(n, generator=g) * 7 - 3 * n).to(torch.int64)


# ---------------------------------------------------------------------------------------------- logits
def _d(t):
    return None if t is None else t.detach().cpu().to(F64)


class Logits:
    """D = x K^T, S = scale D, bS = bound_S, all f64 [Mx, Ny + Nc]."""

    def __init__(self, x, y, cache, scale):
        self.x, y, cache = _d(x), _d(y), _d(cache)
        self.K = y if cache is None else torch.cat([y, cache])
        self.scale = float(scale)
        self.Mx, self.P = self.x.shape
        self.Ny, self.Nk = y.shape[0], self.K.shape[0]
        self.D = self.x @ self.K.t()
        self.S = self.scale * self.D
        self.bS = (self.P + 2) * U * abs(self.scale) * (self.x.abs() @ self.K.abs().t())

    def diag(self, off):
        return CA.masks(self.Mx, self.Ny, self.Nk - self.Ny, off, None, None, "mask", "cpu")[1]


def bound_lse(L, lse, in_d=None):
    b = L.bS if in_d is None else L.bS.masked_fill(~in_d, 0.0)
    return b.max(1).values + (C_EXP + C_LOG + 2) * U * (1 + lse.abs())


def cap_stat(bound):
    return torch.clamp(bound, max=BAR_STAT)


def cap_dx(bound, ref):
    return torch.minimum(bound, BAR_DX_ATOL + BAR_DX_RTOL * ref.abs())


# ---------------------------------------------------------------------------------------------- plain
def plain_stats(L, off):
    """(lse, pos, bound_lse, bound_pos) of rows i with label off + i."""
    lse = torch.logsumexp(L.S, 1)
    dg = L.diag(off)
    return lse, (L.S * dg).sum(1), bound_lse(L, lse), (L.bS * dg).sum(1)


def _grad(L, ibg, parts):
    """parts: per direction (w, E, A, T), [Mx, Nk] each - E = [j in D] exp(s - lse), A = |s - lse| there (0 elsewhere), T
    the target.  -> (dX, dscale rows, bound_dX, bound_dscale)."""
    g = sum(w * (E - T) for w, E, A, T in parts)
    err = sum(w * E * (L.bS + C_EXP * U * (1 + A)) for w, E, A, T in parts)
    return _products(L, ibg, g, err)


def _products(L, ibg, g, err):
    """dX = scale ibg g K and the d scale rows ibg sum_j g D of a gradient g with per-entry error err, and their bounds."""
    dX = L.scale * ibg * (g @ L.K)
    dsc = ibg * (g * L.D).sum(1)
    ibg, sc, n = abs(ibg), abs(L.scale), L.Nk + 2
    Ka, Da = L.K.abs(), L.D.abs()
    b_dX = sc * ibg * (err @ Ka + n * U * (g.abs() @ Ka)) + U * dX.abs()
    b_dsc = ibg * ((err * Da).sum(1) + n * U * (g.abs() * Da).sum(1) + (g.abs() * L.bS).sum(1) / sc) + U * dsc.abs()
    return dX, dsc, b_dX, b_dsc


def _direction(L, w, lse, in_d, T, rows):
    """One direction's part; rows: lse belongs to the rows (else to the batch keys: cache columns take no part)."""
    z = L.S - (_d(lse)[:, None] if rows else torch.nn.functional.pad(_d(lse), (0, L.Nk - L.Ny))[None, :])
    m = in_d if rows else in_d & (torch.arange(L.Nk) < L.Ny)[None, :]
    z = z.masked_fill(~m, float("-inf"))
    Tm = T if rows else T * (torch.arange(L.Nk) < L.Ny)[None, :].to(F64)
    return w, torch.exp(z), z.abs().masked_fill(~m, 0.0), Tm


def _ibg(inv_bg, upstream):
    return inv_bg if upstream is None else inv_bg * float(upstream)


def plain_grad(L, off, lse_x, lse_y, w_row, w_col, inv_bg, upstream=None):
    """include/clipk.h: clipk_simce_grad[_scaled] -> (dX, dscale rows, bound_dX, bound_dscale)."""
    every = torch.ones_like(L.S, dtype=torch.bool)
    T = L.diag(off).to(F64)
    parts = [_direction(L, w_row, lse_x, every, T, True)]
    if w_col != 0.0:
        parts.append(_direction(L, w_col, lse_y, every, T, False))
    return _grad(L, _ibg(inv_bg, upstream), parts)


def simce_ref(x, y, cache, scale, label_offset, lse_x=None, lse_y=None, w_row=0.5, w_col=0.5, inv_bg=1.0, upstream=None):
    """The plain statistics and, where lse_x (and lse_y) are given, the gradient formed from them: a dict with lse, pos,
    dX, dscale (per-row partials) and their bounds b_lse, b_pos, b_dX, b_dscale, S and b_S."""
    L = Logits(x, y, cache, scale)
    lse, pos, b_lse, b_pos = plain_stats(L, label_offset)
    out = dict(L=L, S=L.S, b_S=L.bS, lse=lse, pos=pos, b_lse=b_lse, b_pos=b_pos)
    if lse_x is not None:
        out["dX"], out["dscale"], out["b_dX"], out["b_dscale"] = plain_grad(L, label_offset, lse_x, lse_y, w_row, w_col,
                                                                            inv_bg, upstream)
    return out


# ---------------------------------------------------------------------------------------------- class-aware
def _sum_bound(L, m):
    f = m.to(F64)
    return (L.bS * f).sum(1) + (f.sum(1) + 2) * U * (L.S.abs() * f).sum(1)


def cls_stats(L, off, cls_x, cls_y, same_class, eps):
    """class_aware_ref.stats plus bounds: dict lse, tgt, cnt, b_lse, b_tgt (cnt is exact)."""
    lse, tgt, cnt, T, in_d = CA.stats(L.S, L.Ny, off, cls_x, cls_y, same_class, eps)
    same, diag, _ = CA.masks(L.Mx, L.Ny, L.Nk - L.Ny, off, cls_x, cls_y, same_class, "cpu")
    n = in_d.sum(1).to(F64)
    sd = (L.S * in_d.to(F64)).sum(1)
    if same_class == "positive":
        q, b_q = (L.S * same.to(F64)).sum(1) / cnt, _sum_bound(L, same) / cnt
    else:
        q, b_q = (L.S * diag.to(F64)).sum(1), (L.bS * diag.to(F64)).sum(1)
    b_tgt = (1 - eps) * b_q + eps * _sum_bound(L, in_d) / n + 3 * U * (((1 - eps) * q).abs() + (eps * sd / n).abs())
    return dict(lse=lse, tgt=tgt, cnt=cnt, b_lse=bound_lse(L, lse, in_d), b_tgt=b_tgt)


def cls_grad(L, off, lse_x, lse_y, cnt_x, cnt_y, cls_x, cls_y, same_class, eps, nkeys_y, w_row, w_col, inv_bg,
             upstream=None):
    """include/clipk.h: clipk_simce_grad_cls (the arithmetic of class_aware_ref.simce_grad_cls, with bounds)."""
    same, diag, in_d = CA.masks(L.Mx, L.Ny, L.Nk - L.Ny, off, cls_x, cls_y, same_class, "cpu")
    pos = same_class == "positive"
    f = lambda m: m.to(F64)
    parts = []
    if w_row != 0.0:
        cx = _d(cnt_x)[:, None]
        nx = float(L.Nk) if pos else L.Nk - (cx - 1.0)
        T = (1.0 - eps) * (f(same) / cx if pos else f(diag)) + eps / nx * f(in_d)
        parts.append(_direction(L, w_row, lse_x, in_d, T, True))
    if w_col != 0.0:
        cy = torch.nn.functional.pad(_d(cnt_y), (0, L.Nk - L.Ny), value=1.0)[None, :]
        ny = float(nkeys_y) if pos else nkeys_y - (cy - 1.0)
        T = (1.0 - eps) * (f(same) / cy if pos else f(diag)) + eps / ny * f(in_d)
        parts.append(_direction(L, w_col, lse_y, in_d, T, False))
    return _grad(L, _ibg(inv_bg, upstream), parts)


# ---------------------------------------------------------------------------------------------- hard-negative
def hard_factor(L):
    return max(1.0, L.S.abs().max().item() / SCALE_A)


def hard_tol(L, beta, what, ref):
    """The tolerance of tests/test_gpu_hard_negative_loss.py for `what`, scaled by max |S| / 14.2849 (module docstring)."""
    f = hard_factor(L)
    assert what in ("lse_h", "q", "k1", "k2")
    return torch.full_like(ref, BAR_STAT * (1 + 2 * beta) * f)


def hard_cap_dx(bound, ref, beta):
    """The bar of tests/test_gpu_hard_negative_loss.py on dX (generic family): the smaller of it and the derived bound."""
    return torch.minimum(bound, 1e-6 * (1 + beta) + BAR_DX_RTOL * ref.abs())


def hard_stats(L, off, cls_x, cls_y, beta):
    """hard_negative_ref.stats / coefficients: dict lse_h, pos, coef [3, Mx], b_pos."""
    st = HN.stats(L.S, L.Ny, off, cls_x, cls_y, beta)
    return dict(lse_h=st["lse_h"], pos=st["pos"], coef=HN.coefficients(st, beta), b_pos=(L.bS * L.diag(off).to(F64)).sum(1))


def hard_grad(L, off, coef_x, coef_y, cls_x, cls_y, beta, w_row, w_col, inv_bg, upstream=None):
    """include/clipk.h: clipk_simce_grad_hard from the f32 coefficients (q, k1, k2) it is handed - the arithmetic of
    hard_negative_ref.simce_grad_hard - with bounds: given the coefficients the derivation closes as for the plain pass.
    Per direction g = [neg] (e1 - e2) - q [diag], e1 = exp((1 + beta) s + k1), e2 = exp(beta s + k2); an exponent
    c s + k is one fma of the rounded logit: its error is c bound_S + u |c s + k|, then expf and the subtraction:
        err_g = sum_d w_d (e1 ((1 + beta) bound_S + u |z1| + (C_EXP + 1) u) + e2 (beta bound_S + u |z2| + (C_EXP + 1) u)
                           + u q [diag])
    -> (dX, dscale rows, bound_dX, bound_dscale)."""
    neg, diag = HN.neg_mask(L.Mx, L.Ny, L.Nk - L.Ny, off, cls_x, cls_y, "cpu")
    batch = (torch.arange(L.Nk) < L.Ny)[None, :]
    g, err = torch.zeros_like(L.S), torch.zeros_like(L.S)
    for w, coef, rows in ((w_row, _d(coef_x), True), (w_col, _d(coef_y), False)):
        if w == 0.0:
            continue
        q, k1, k2 = (c[:, None] if rows else torch.nn.functional.pad(c, (0, L.Nk - L.Ny))[None, :] for c in coef)
        m = neg if rows else neg & batch
        T = q * (diag if rows else diag & batch).to(F64)
        g -= w * T
        err += w * U * T
        for c, k in ((1.0 + beta, k1), (beta, k2)):
            if c == 0.0:
                continue
            z = (c * L.S + k).masked_fill(~m | torch.isinf(k), float("-inf"))
            e = torch.exp(z)
            g += (w if c > beta else -w) * e
            err += w * e * (c * L.bS + U * z.abs().masked_fill(torch.isinf(z), 0.0) + (C_EXP + 1) * U)
    return _products(L, _ibg(inv_bg, upstream), g, err)


# ---------------------------------------------------------------------------------------------- ce_combine
def combine(lse_r, pos_r, lse_c, pos_c, w_row, w_col, bg):
    """(value, bound) of include/clipk.h: clipk_ce_combine on the f32 vectors handed in."""
    dr = _d(lse_r) - _d(pos_r)
    v, a = w_row * dr.sum(), abs(w_row) * dr.abs().sum()
    if lse_c is not None:
        dc = _d(lse_c) - _d(pos_c)
        v, a = v + w_col * dc.sum(), a + abs(w_col) * dc.abs().sum()
    return v / bg, (dr.numel() + 4) * U * a / bg


# ---------------------------------------------------------------------------------------------- shapes
# name -> (Mx, Ny, Nc, label_offset): the smallest shapes that reach each branch of the tiled (64 x 64) and the
# first-generation (32 x 32) passes; tests/test_simce_ref_host.py pins their plan numbers.
SHAPES = {"two-tile": (1500, 1510, 60, 10), "three-tile": (2048, 2100, 0, 52), "many-splits": (70, 4200, 30, 4000),
          "sweep": (65, 104, 50, 3)}
SHAPE_P = {"two-tile": (36, 32), "three-tile": (20,), "many-splits": (12, 32)}
TINY = ((1, 1, 0, 0), (1, 65, 0, 64), (65, 65, 1, 0), (63, 64, 0, 0), (64, 63, 0, 0))     # the last: plain entries only
BATCHED_B, BATCHED_P = 600, (36, 160, 512)           # six problems on the tiled batched passes
BATCHED_PLAIN_B, BATCHED_PLAIN_P = 770, 32           # six problems on the first-generation batched passes
SWEEP_P_TILED = (4, 132, 260, 388, 508, 512)
SWEEP_P_FIRST_LSE = (4, 132, 260, 516, 956, 960)     # 1020 and 1024 are refused: first_gen_plan
SWEEP_P_FIRST_GRAD = (32, 96, 192, 384, 768)         # 1024 is refused: first_gen_plan
