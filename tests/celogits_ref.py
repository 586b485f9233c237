"""Yardstick for the cross-entropy kernels on MATERIALISED logits (csrc/celogits.hip), plain torch on the CPU.

The contract (celogits.hip's header, include/clipk.h):

    rows:     lse[i] = logsumexp_j [S | S2][i, j]        pos[i] = S[i, i + off]   (0 when i + off is no column of S)
    columns:  lse[j] = logsumexp_i S[i, j]               pos[j] = S[j + off, j]   (0 when j + off is no row of S)
    backward: dS[i, j]  = g (wr (exp(S_ij - lse_r[i]) - [j == i + off_r]) + wc (exp(S_ij - lse_c[j]) - [i == j + off_c]))
              dS2[i, j] = g wr exp(S2_ij - lse_r[i])     (0 without lse_r); a NULL lse switches its direction off
    a -inf logit is a zero term; a row / column with no finite logit has lse = -inf (torch.logsumexp's answer)

`lse_rows`, `lse_cols`, `bwd`: the f64 reference, a few lines each, nothing shared with the restatement below.  The backward
    is a function of the lse it is HANDED (the kernels' f32 lse values, read as f64), so the forward's rounding is not
    charged to it.  exp(-inf - -inf) is NaN: the gradient of a row / column without a finite logit is NaN in the reference,
    and NaN entries of the reference are left out of every comparison.

`restate(case, inp, dt, mutant)`: the same formulas in the kernels' ORDER - 64 lanes that each run the online (m, l) update
    over every 64th column of S and then of S2, the xor-butterfly merge of the 64 pairs; 64 columns x 4 row slices merged
    one after the other - in dtype `dt` with torch's accurate exp / log.  dt = f32 is the restatement the tolerance rule
    measures; dt = f64 with a mutant gives that mistake's exact effect.

`check(got, ref, restated, what)`: the project's rule (attention_ref.check): max-norm deviation from f64
    <= max(8 x the restatement's deviation, FLOOR x magnitude), FLOOR = 64 x 2^-24.  8 is the margin for "the same
    arithmetic in another summation order".  Infinities must sit where the reference has them, bit for bit.

    The kernels use __expf / __logf where the restatement uses exp / log.  __expf(x) is exp2(x log2(e)) on the
    transcendental unit: the product x log2(e) is rounded to f32 (relative 2^-24), which moves the result by the relative
    amount |x| log2(e) 2^-24 ln 2 = |x| 2^-24, next to the unit's own 1 ulp.  Where does that go?
      lse: every term exp(x_j - m) has x_j - m <= 0 and weight p_j = exp(x_j - lse); the error of l is at most
           sum_j p_j |x_j - m| 2^-24 relative, and sum_j p_j |x_j - m| <= log(n) + 1 for n terms (the entropy bound), so
           below 8 x 2^-24 = 4.8e-7 for n <= 1000; log adds 1 ulp of log2(l) <= 10: 2^-20 = 9.5e-7.  FLOOR x |lse| is
           3.8e-6 |lse|, and the largest |lse| of a case is ~10 (generic, holes) or ~70 (peaked); onehot is exact.  No
           extra term is needed.
      dS:  |x| exp(x) <= 1 / e for x <= 0, so the argument rounding moves exp(S - lse) by at most 2^-24 / e absolute, its
           magnitude being up to 1: far below FLOOR.  No extra term either.
    So the rule stands as attention_ref states it; the GPU file's header records the measured kernel / bound ratios.

MUTANTS: one deliberate mistake each, applied to the restatement.  tests/test_celogits_ref_host.py shows that `check`
    rejects each of them at every case it applies to.  A mutant APPLIES to a case when the case has the structure it needs
    (`structural`) and its exact effect - the same mistake in f64 against the f64 reference - is larger than twice the
    bound (`applies`): dropping a column that holds 1e-9 of a row's mass is no mistake any f32 test could see.  Both are
    computed from the inputs and the reference alone, never from a kernel's output.

CASES: the one table of shapes, offsets, strides and input families both test files walk.
"""
import math
from types import SimpleNamespace

import torch

F32, F64 = torch.float32, torch.float64
INF = float("inf")
FLOOR = 64 * 2.0 ** -24
MARGIN = 8.0
G = 1.7                                  # upstream gradient of every backward case
PAD = 5                                  # extra elements of a padded row stride
TINY = 2.0 ** -126                       # an effect below the smallest normal f32 is none in f32 (exp(-130) next to a 0)


# ------------------------------------------------------------------------------------------------ f64 reference
def _lse(x, dim):
    """logsumexp in f64 from its definition; -inf where there is no finite entry."""
    m = x.max(dim).values
    safe = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    return torch.where(m == -INF, m, safe + torch.log(torch.exp(x - safe.unsqueeze(dim)).sum(dim)))


def _diag(S, off, columns):
    """rows: S[i, i + off]; columns: S[j + off, j]; 0 where that is outside S."""
    M, N = S.shape
    k = torch.arange(N if columns else M)
    lab = k + off
    ok = (lab >= 0) & (lab < (M if columns else N))
    pos = torch.zeros(k.numel(), dtype=S.dtype)
    pos[ok] = S[lab[ok], k[ok]] if columns else S[k[ok], lab[ok]]
    return pos


def lse_rows(S, S2, label_offset):
    S = S.to(F64)
    full = S if S2 is None or S2.shape[1] == 0 else torch.cat([S, S2.to(F64)], 1)
    return _lse(full, 1), _diag(S, label_offset, False)


def lse_cols(S, label_offset):
    S = S.to(F64)
    return _lse(S, 0), _diag(S, label_offset, True)


def _onehot(M, N, off, columns, dt=F64):
    """rows: [j == i + off]; columns: [i == j + off]."""
    i, j = torch.arange(M)[:, None], torch.arange(N)[None, :]
    return ((i == j + off) if columns else (j == i + off)).to(dt)


def bwd(S, S2, lse_r, lse_c, wr, wc, off_r, off_c, g):
    S = S.to(F64)
    M, N = S.shape
    d = torch.zeros(M, N, dtype=F64)
    if lse_r is not None:
        d = d + wr * (torch.exp(S - lse_r.to(F64)[:, None]) - _onehot(M, N, off_r, False))
    if lse_c is not None:
        d = d + wc * (torch.exp(S - lse_c.to(F64)[None, :]) - _onehot(M, N, off_c, True))
    dS2 = None
    if S2 is not None and S2.shape[1] > 0:
        dS2 = g * wr * torch.exp(S2.to(F64) - lse_r.to(F64)[:, None]) if lse_r is not None else torch.zeros(S2.shape, dtype=F64)
    return g * d, dS2


# ------------------------------------------------------------------------------------------------ restatement and mutants
MUTANTS = {
    "merge_unscaled": "1. two (m, l) pairs merged without rescaling: l = l1 + l2",
    "no_cache": "2. the cache columns S2 left out of the row LSE",
    "pos_no_offset": "3. pos ignores label_offset",
    "col_pos_transposed": "4. the column pos reads S[j, j + off]",
    "onehot_minus": "5. the backward's row one-hot at j == row - off",
    "ds2_col_term": "6. dS2 also gets the column term",
    "g_dropped": "7. the upstream gradient g dropped",
    "stride_n": "8. the row stride taken as N (N2 for S2 and dS2)",
    "ragged_cols": "9. the last N % 64 columns dropped",
    "ragged_rows": "10. the last M % 4 rows dropped",
    "three_slices": "11. three of the four row slices merged in the column LSE",
    "d1": "12. the online update without the -inf guard: l += exp(v - m) at v = m = -inf (the code before this fix)",
}


def _online(vals, live, dt, guarded):
    """The lane-local update of ce_lse_{row,col}_kernel over vals[t] (t = 0, 1, ...), elementwise over the other dims;
    live[t] False: no element there."""
    m = torch.full(vals.shape[1:], -INF, dtype=dt)
    l = torch.zeros(vals.shape[1:], dtype=dt)
    for v, on in zip(vals, live):
        up = v > m
        grown = l * torch.exp(m - v) + 1.0
        added = l + torch.exp(v - m)
        if guarded:
            added = torch.where(v != -INF, added, l)
        l = torch.where(on, torch.where(up, grown, added), l)
        m = torch.where(on & up, v, m)
    return m, l


def _merge(m, l, m2, l2, unscaled):
    mn = torch.maximum(m, m2)
    if unscaled:
        return mn, l + l2
    a = torch.where(m == -INF, torch.zeros_like(l), l * torch.exp(m - mn))
    b = torch.where(m2 == -INF, torch.zeros_like(l2), l2 * torch.exp(m2 - mn))
    return mn, a + b


def _lanes(x, dt):
    """[M, n] -> values [ceil(n / 64), M, 64] (lane = column % 64) and the mask of real elements."""
    M, n = x.shape
    steps = (n + 63) // 64
    v = torch.zeros(M, steps * 64, dtype=dt)
    on = torch.zeros(M, steps * 64, dtype=torch.bool)
    v[:, :n], on[:, :n] = x.to(dt), True
    return v.view(M, steps, 64).permute(1, 0, 2), on.view(M, steps, 64).permute(1, 0, 2)


def restate_rows(S, S2, off, dt=F32, mutant=None):
    M, N = S.shape
    Sx = S[:, :N - N % 64] if mutant == "ragged_cols" else S
    parts = [_lanes(Sx, dt)] if Sx.shape[1] else []
    if S2 is not None and S2.shape[1] > 0 and mutant != "no_cache":
        parts.append(_lanes(S2, dt))
    if parts:
        m, l = _online(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), dt, mutant != "d1")
    else:
        m, l = torch.full((M, 64), -INF, dtype=dt), torch.zeros(M, 64, dtype=dt)
    o = 32
    while o:
        idx = torch.arange(64) ^ o
        m, l = _merge(m, l, m[:, idx], l[:, idx], mutant == "merge_unscaled")
        o >>= 1
    lse = m[:, 0] + torch.log(l[:, 0])
    pos = _diag(S.to(dt), 0 if mutant == "pos_no_offset" else off, False)
    if mutant == "ragged_rows" and M % 4:
        lse[M - M % 4:], pos[M - M % 4:] = math.nan, math.nan           # never written
    return {"lse": lse, "pos": pos}


def restate_cols(S, off, dt=F32, mutant=None):
    M, N = S.shape
    Mx = M - M % 4 if mutant == "ragged_rows" else M
    steps = (M + 3) // 4
    v = torch.zeros(steps * 4, N, dtype=dt)
    on = torch.zeros(steps * 4, N, dtype=torch.bool)
    v[:Mx], on[:Mx] = S[:Mx].to(dt), True
    m, l = _online(v.view(steps, 4, N), on.view(steps, 4, N), dt, mutant != "d1")     # [4 slices, N]
    mm, ll = m[0], l[0]
    for k in range(1, 3 if mutant == "three_slices" else 4):
        mm, ll = _merge(mm, ll, m[k], l[k], mutant == "merge_unscaled")
    lse = mm + torch.log(ll)
    if mutant == "col_pos_transposed":
        k = torch.arange(N)
        ok = (k < M) & (k + off >= 0) & (k + off < N)
        pos = torch.zeros(N, dtype=dt)
        pos[ok] = S.to(dt)[k[ok], k[ok] + off]
    else:
        pos = _diag(S.to(dt), 0 if mutant == "pos_no_offset" else off, True)
    if mutant == "ragged_cols" and N % 64:
        lse[N - N % 64:], pos[N - N % 64:] = math.nan, math.nan
    return {"lse": lse, "pos": pos}


def restate_bwd(S, S2, lse_r, lse_c, wr, wc, off_r, off_c, g, dt=F32, mutant=None):
    """Every product in dtype dt, in the kernel's order: d = 0; d += wr (..); d += wc (..); g * d."""
    M, N = S.shape
    t = lambda x: torch.tensor(x, dtype=dt)                                 # noqa: E731  (scalars rounded as the ABI's floats)
    wr, wc, gv = t(wr), t(wc), t(1.0 if mutant == "g_dropped" else g)
    S = S.to(dt)
    d = torch.zeros(M, N, dtype=dt)
    if lse_r is not None:
        d = d + wr * (torch.exp(S - lse_r.to(dt)[:, None]) - _onehot(M, N, -off_r if mutant == "onehot_minus" else off_r, False, dt))
    if lse_c is not None:
        d = d + wc * (torch.exp(S - lse_c.to(dt)[None, :]) - _onehot(M, N, off_c, True, dt))
    dS = gv * d
    dS2 = None
    if S2 is not None and S2.shape[1] > 0:
        N2 = S2.shape[1]
        dS2 = gv * wr * torch.exp(S2.to(dt) - lse_r.to(dt)[:, None]) if lse_r is not None else torch.zeros(M, N2, dtype=dt)
        if mutant == "ds2_col_term" and lse_c is not None:
            lc = lse_c.to(dt)[torch.arange(N2).clamp(max=N - 1)]
            dS2 = dS2 + gv * wc * torch.exp(S2.to(dt) - lc[None, :])
    if mutant == "ragged_cols" and N % 64:
        dS[:, N - N % 64:] = math.nan
    if mutant == "ragged_rows" and M % 4:
        dS[M - M % 4:] = math.nan
        if dS2 is not None:
            dS2[M - M % 4:] = math.nan
    return {"dS": dS, "dS2": dS2}


# ------------------------------------------------------------------------------------------------ the tolerance rule
def deviation(got, ref, restated, what):
    """(ok, kernel deviation, bound).  NaN entries of the reference are not compared; its infinities must be matched."""
    got, ref, restated = (torch.as_tensor(x).detach().double().cpu() for x in (got, ref, restated))
    assert got.shape == ref.shape == restated.shape, (what, got.shape, ref.shape, restated.shape)
    cmp = ~torch.isnan(ref)
    fin = torch.isfinite(ref)
    inf = cmp & ~fin
    assert torch.equal(restated[inf], ref[inf]) and torch.isfinite(restated[fin]).all(), what
    if not (torch.equal(got[inf], ref[inf]) and torch.isfinite(got[fin]).all()):
        return False, INF, 0.0
    if not fin.any():
        return True, 0.0, 0.0
    dev_k = float((got[fin] - ref[fin]).abs().max())
    dev_r = float((restated[fin] - ref[fin]).abs().max())
    bound = max(MARGIN * dev_r, FLOOR * float(ref[fin].abs().max()))
    return dev_k <= bound, dev_k, bound


def check(got, ref, restated, what):
    """Assert the rule; -> deviation / bound (0 when both are 0)."""
    ok, dev_k, bound = deviation(got, ref, restated, what)
    assert ok, (what, dev_k, bound)
    return dev_k / bound if bound else 0.0


def bit_equal(a, b):
    """Same f32 bit patterns (NaN payloads and the sign of zero included)."""
    a, b = torch.as_tensor(a).detach().cpu(), torch.as_tensor(b).detach().cpu()
    return a.dtype == b.dtype == F32 and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                                                            b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ the cases
FAMILIES = ("generic", "peaked", "holes", "onehot")
OFFSETS = (0, 3, -3, "N")
WEIGHTS = {"row": (1.0, 0.0), "both": (0.5, 0.5), "col": (0.0, 0.5)}      # row: lse_col = NULL; col: lse_row = NULL
ROW_SHAPES = [(M, N, N2) for M in (1, 3, 4, 5, 9) for N in (1, 2, 63, 64, 65, 129, 200) for N2 in (0, 1, 63, 64, 130)]
COL_SHAPES = [(M, N) for N in (1, 63, 64, 65, 130) for M in (1, 2, 3, 4, 5, 9, 67)]
BWD_SHAPES = [(N, N2) for N in (1, 255, 256, 257, 513) for N2 in (0, 1, 300, 600)]
# the offsets, crossed on rectangular shapes of their own (every other shape takes one offset in turn)
OFFSET_SHAPES = [(5, 9, 0), (9, 5, 3), (4, 70, 0), (70, 4, 0)]


def _off(o, N):
    return N if o == "N" else o


def _mk(kind, family, k, M, N, N2, off, off_c=0, weights=None):
    """pad: every stride is the row length + 5 (every other case); joint: S and S2 are views of one [M, N + N2] buffer."""
    name = f"{kind}-{family}-M{M}-N{N}-N2{N2}-off{off}" + (f"-offc{off_c}-{weights}" if kind == "bwd" else "")
    return SimpleNamespace(name=name, kind=kind, family=family, M=M, N=N, N2=N2, off=off, off_c=off_c, weights=weights,
                           pad=bool(k & 1), joint=bool(N2 > 0 and k % 3 == 2), seed=1000 + 7 * k)


def _cases():
    out = []
    for fam in FAMILIES:
        for k, (M, N, N2) in enumerate(ROW_SHAPES):
            out.append(_mk("row", fam, k, M, N, N2, _off(OFFSETS[k % 4], N)))
        for k, (M, N) in enumerate(COL_SHAPES):
            out.append(_mk("col", fam, k, M, N, 0, _off(OFFSETS[k % 4], N)))
        k = 0
        for N, N2 in BWD_SHAPES:
            for w in WEIGHTS:
                if fam == "onehot" and w == "both":
                    continue             # one finite logit per row OR per column: the family defines one direction's lse
                M = (1, 3, 5, 6)[k % 4]
                out.append(_mk("bwd", fam, k, M, N, N2, _off(OFFSETS[k % 4], N), _off(OFFSETS[(k + 1) % 4], N), w))
                k += 1
        for k, (M, N, N2) in enumerate(OFFSET_SHAPES):
            for o in OFFSETS:
                out.append(_mk("row", fam, k, M, N, N2, _off(o, N)))
                if N2 == 0:
                    out.append(_mk("col", fam, k + 1, M, N, 0, _off(o, N)))
                for oc in OFFSETS:
                    if fam != "onehot":
                        out.append(_mk("bwd", fam, k, M, N, N2, _off(o, N), _off(oc, N), "both"))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


def by_columns(case):
    """onehot: one finite logit per column (the column direction's family) instead of one per row."""
    return case.kind == "col" or (case.kind == "bwd" and case.weights == "col")


def inputs(case):
    """S [M, N], S2 [M, N2] or None: seeded on the CPU, built in f64, rounded to f32."""
    M, N, N2, W = case.M, case.N, case.N2, case.N + case.N2
    g = torch.Generator().manual_seed(case.seed)
    x = torch.randn(M, W, generator=g, dtype=F64) * 4
    u = torch.rand(M + W, generator=g, dtype=F64)
    if case.family == "peaked":
        # background -60; one +60 .. +80 logit per row of [S | S2] and per column of S, at the places where a lane, a
        # merge or a slice begins or ends: lane 0, lane 63, the last (ragged) column, inside S2, the last row slice
        x = -60 + x / 8
        cols = [c for c in (0, 63, N - 1, N + N2 // 2 if N2 else N - 1, 64, W - 1) if c < W]
        rows = [r for r in (0, M - 1, (M // 4) * 4 - 1 if M >= 4 else M - 1, 1) if 0 <= r < M]
        for i in range(M):
            x[i, cols[i % len(cols)]] = 60 + 20 * u[i]
        for j in range(N):
            x[rows[j % len(rows)], j] = 60 + 20 * u[M + j]
    elif case.family == "holes":
        # -inf: column 0 of the odd rows (a lane's, a slice's first element), a whole lane stride of two rows in three,
        # all of S2 in the even rows, the diagonal, the last row and the last column altogether
        x[1::2, 0] = -INF
        for i in range(M):
            if i % 3 != 2:
                x[i, 5:N:64] = -INF
        x[0::2, N:] = -INF
        k = torch.arange(min(M, N))
        x[k, k] = -INF
        x[M - 1, :] = -INF
        x[:, N - 1] = -INF
    elif case.family == "onehot":
        y = torch.full((M, W), -INF, dtype=F64)
        if by_columns(case):
            for j in range(N):                                           # column j: row 3, M - 1, then every row in turn
                r = (3 % M, M - 1)[j] if j < 2 else (5 * j + 3) % M
                y[r, j] = x[r, j]
        else:
            for i in range(M):                                           # row i: over S and S2, lane 0 and the last column
                c = (W - 1, 0)[i] if i < 2 else (7 * i + N - 1) % W
                y[i, c] = x[i, c]
        x = y
    x = x.to(F32)
    return x[:, :N].contiguous(), (x[:, N:].contiguous() if N2 else None)


def lse_inputs(case, S, S2):
    """The lse vectors a backward case is handed: the f64 reference's, rounded to f32 (None: direction off)."""
    wr, wc = WEIGHTS[case.weights]
    lr = lse_rows(S, S2, 0)[0].to(F32) if case.weights != "col" else None
    lc = lse_cols(S, 0)[0].to(F32) if case.weights != "row" else None
    return lr, lc, wr, wc


def reference(case, S, S2):
    if case.kind == "row":
        lse, pos = lse_rows(S, S2, case.off)
        return {"lse": lse, "pos": pos}
    if case.kind == "col":
        lse, pos = lse_cols(S, case.off)
        return {"lse": lse, "pos": pos}
    lr, lc, wr, wc = lse_inputs(case, S, S2)
    dS, dS2 = bwd(S, S2, lr, lc, wr, wc, case.off, case.off_c, G)
    return {"dS": dS, "dS2": dS2}


def layout(case, S, S2, guard=0):
    """The buffers as the kernels get them, NaN in every pad and in `guard` elements behind each buffer:
    -> (flat buffers, S view, S2 view or None, ld, ld2).  pad: each row stride is the row length + 5; joint: S and S2 are
    the two column blocks of one [M, N + N2] buffer."""
    M, N, N2 = case.M, case.N, case.N2
    extra = PAD if case.pad else 0
    if case.joint:
        ld = ld2 = N + N2 + extra
        flat = torch.full((M * ld + guard,), math.nan, dtype=F32)
        rows = flat[:M * ld].view(M, ld)
        rows[:, :N], rows[:, N:N + N2] = S, S2
        return [flat], rows[:, :N], rows[:, N:N + N2], ld, ld2
    ld, ld2 = N + extra, (N2 + extra if N2 else 0)
    flat = torch.full((M * ld + guard,), math.nan, dtype=F32)
    flat[:M * ld].view(M, ld)[:, :N] = S
    if not N2:
        return [flat], flat[:M * ld].view(M, ld)[:, :N], None, ld, 0
    flat2 = torch.full((M * ld2 + guard,), math.nan, dtype=F32)
    flat2[:M * ld2].view(M, ld2)[:, :N2] = S2
    return [flat, flat2], flat[:M * ld].view(M, ld)[:, :N], flat2[:M * ld2].view(M, ld2)[:, :N2], ld, ld2


def restate(case, S, S2, dt=F32, mutant=None):
    """The restatement (or one mutant of it) of the case's kernel."""
    assert mutant is None or mutant in MUTANTS, mutant
    if mutant == "stride_n":
        # the kernels' buffers read from the same base pointers with the row length as the stride
        flats, Sv, S2v, ld, ld2 = layout(case, S, S2, guard=case.M * (case.N + case.N2))
        S = flats[0][:case.M * case.N].view(case.M, case.N)
        if S2 is not None:
            base = flats[0][case.N:] if case.joint else flats[1]
            S2 = base[:case.M * case.N2].view(case.M, case.N2)
    if case.kind == "row":
        return restate_rows(S, S2, case.off, dt, mutant)
    if case.kind == "col":
        return restate_cols(S, case.off, dt, mutant)
    S0, S20 = inputs(case)
    lr, lc, wr, wc = lse_inputs(case, S0, S20)
    return restate_bwd(S, S2, lr, lc, wr, wc, case.off, case.off_c, G, dt, mutant)


def structural(mutant, case):
    """Does the case have what the mistake needs to show at all?"""
    k, M, N, N2 = case.kind, case.M, case.N, case.N2
    return {
        "merge_unscaled": k != "bwd" and (M > 1 if k == "col" else N + N2 > 1),
        "no_cache": k == "row" and N2 > 0,
        "pos_no_offset": k != "bwd" and case.off != 0,
        "col_pos_transposed": k == "col" and case.off != 0,
        "onehot_minus": k == "bwd" and case.weights != "col" and case.off != 0,
        "ds2_col_term": k == "bwd" and N2 > 0 and case.weights != "row",
        "g_dropped": k == "bwd",
        "stride_n": M > 1 and (case.pad or case.joint),
        "ragged_cols": N % 64 != 0,
        "ragged_rows": M % 4 != 0,
        "three_slices": k == "col" and M >= 4,
        "d1": k != "bwd" and case.family in ("holes", "onehot"),
    }[mutant]


def d1_trigger(case, S, S2):
    """Does mutant 12 reach an output?  exp(-inf + inf) = NaN enters a lane's (a row slice's) l at a -inf met while its m is
    still -inf, and the cross-lane merge drops the l of a pair with m = -inf: the NaN survives where a FINITE logit
    follows in the same lane - column 0 masked and column 64 not, or S masked in a lane whose S2 column is not."""
    if case.kind == "row":
        parts = [_lanes(S, F64)] + ([_lanes(S2, F64)] if S2 is not None else [])
        v, on = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    else:
        steps = (case.M + 3) // 4
        v, on = torch.zeros(steps * 4, case.N, dtype=F64), torch.zeros(steps * 4, case.N, dtype=torch.bool)
        v[:case.M], on[:case.M] = S.to(F64), True
        v, on = v.view(steps, 4, case.N), on.view(steps, 4, case.N)
    hole = on & (v == -INF)
    before = torch.cumsum(hole, 0) - hole.long() > 0
    return bool((on & torch.isfinite(v) & before).any())


def rejected(got, ref, restated, what):
    """names of the outputs on which `check` rejects `got`."""
    return [nm for nm in ref if ref[nm] is not None and not deviation(got[nm], ref[nm], restated[nm], f"{what} {nm}")[0]]


def applies(mutant, case, S, S2, ref, restated):
    """structural, and the mistake's exact effect (the mutant in f64 against the f64 reference) exceeds twice the bound
    (and the smallest normal f32) on some output, or puts a non-finite value where the reference has a finite one."""
    if not structural(mutant, case):
        return False
    exact = restate(case, S, S2, F64, mutant)
    for nm, r in ref.items():
        if r is None:
            continue
        ok, dev, _ = deviation(exact[nm], r, restated[nm], f"{case.name} [{mutant} f64] {nm}")
        bound = deviation(restated[nm], r, restated[nm], nm)[2]
        if not ok and (dev == INF or dev > max(2 * bound, TINY)):
            return True
    return False


CASES = _cases()
