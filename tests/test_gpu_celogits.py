"""GPU: the cross-entropy kernels on materialised logits (csrc/celogits.hip: ce_lse_row_kernel, ce_lse_col_kernel,
ce_bwd_kernel) against the f64 reference of tests/celogits_ref.py, through the C entry points clipk_ce_logits_lse and
clipk_ce_logits_bwd, branch by branch.  The case table (celogits_ref.CASES) is the one tests/test_celogits_ref_host.py walks
on the CPU: every M x N x N2 around the 4 rows of a block and the 64 lanes of a wave (N < 64 with N2 > 0: some lanes first see
a value in S2), every N x M around the 64 columns x 4 row slices of the column kernel (M < 4: empty slices), N and N2 around
the backward's 256-column blocks with the wider side on either operand, the three weightings (row only with lse_col = NULL,
both, column only with lse_row = NULL and dS2 = 0), label offsets 0 / +3 / -3 / +N on rectangular S (a label outside S: pos = 0
and no one-hot), and four input families - generic, peaked (-60 background, +60 .. +80 at the lane / slice edges), holes (-inf
in column 0, over a lane stride, in all of S2, on the diagonal, a whole row and a whole column) and onehot (one finite logit
per row or column).

Every buffer is the test's own: inputs with NaN between the rows (every other case has row strides of the row length + 5; one
case in three takes S and S2, dS and dS2 as the two column blocks of one buffer), outputs pre-filled with NaN between two
fences.  After the call every element outside the outputs proper still holds its NaN pattern.  Every case runs twice: same
bits.

lse, dS and dS2 are held to celogits_ref.check: max-norm deviation from f64 <= max(8 x the f32 restatement's deviation,
64 x 2^-24 x magnitude); the host test shows that this rule rejects twelve mutant restatements, the code before the -inf fix
among them.  pos is a copy: bit for bit.  onehot: lse IS the one finite logit, dS is 0 or g w: bit for bit.  Gradient rows /
columns whose lse is -inf (no finite logit) are NaN in the reference and not compared.

Worst kernel deviation / bound per kernel and family, measured on an MI355X (1.0 = the bound, 0.125 = as far from f64 as the
f32 restatement; the file prints the table at the end of a run with -s):
                 generic        peaked         holes          onehot
  row lse        0.015 (191)    0.013 (191)    0.016 (191)    0 (191)
  column lse     0.076 (47)     0.013 (47)     0.015 (47)     0 (47)
  backward dS    0.053 (124)    0.030 (124)    0.033 (124)    0.007 (40)
  backward dS2   0.189 (61)     0.231 (61)     0.162 (61)     0.007 (30)
(comparisons in brackets; pos, compared in bits, comes with every lse).  The lse figures sit below 0.125 because the bound's
floor, 64 x 2^-24 |lse|, is what counts there: the f32 restatement is closer still.  dS2 is the largest: its magnitude is
small (the cache columns hold no label), so the floor is, and __expf's argument rounding shows.  test_more_rows_than_grid_y
and the cross_entropy_diag tests apply the same rule; they are not in the table.
Against the library of the commit before the -inf fix the holes and onehot walks fail with NaN in lse at 128 and 142 of 191
row cases and 12 and 20 of 47 column cases - the cases celogits_ref.d1_trigger predicts, no other - and
test_cross_entropy_diag[holes] returns a NaN loss.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import celogits_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BAD_ARG, UNSUPPORTED = -1, -2           # include/clipk.h
GUARD = 16
NAN_BITS = 0x7fc00abc                   # the prefill: a NaN no kernel produces
_WORST = {}                             # (kind, family, output) -> [comparisons, worst ratio]


def _ops():
    from clip_dplm_amd import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\nworst kernel deviation / bound (comparisons):")
    for key in sorted(_WORST):
        print(f"  {key[0]:4s} {key[1]:8s} {key[2]:4s} {_WORST[key][1]:.3f} ({_WORST[key][0]})")


def _note(case, nm, ratio):
    w = _WORST.setdefault((case.kind, case.family, nm), [0, 0.0])
    w[0] += 1
    w[1] = max(w[1], ratio)


class _Out:
    """n f32 between two GUARD-element fences on the device, every element the NaN pattern to begin with."""
    def __init__(self, n, dev):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def read(self):
        return self.buf.cpu()[GUARD:GUARD + self.n].clone()

    def untouched_outside(self, written):
        """written: bool [n], the elements the call may write; everything else must still hold the pattern."""
        got = self.buf.cpu().view(torch.int32)
        keep = torch.ones(self.n + 2 * GUARD, dtype=torch.bool)
        keep[GUARD:GUARD + self.n] = ~written
        return bool((got[keep] == NAN_BITS).all())


def _rows_mask(M, ld, col0, n):
    """bool [M * ld]: columns [col0, col0 + n) of every row."""
    m = torch.zeros(M, ld, dtype=torch.bool)
    m[:, col0:col0 + n] = True
    return m.view(-1)


def _inputs_on_device(case, S, S2, dev):
    """-> (keep-alive list, S pointer, ld, S2 pointer or None, ld2)."""
    flats, _, _, ld, ld2 = R.layout(case, S, S2, guard=GUARD)
    d = [f.to(dev) for f in flats]
    p2 = None
    if S2 is not None:
        p2 = d[0].data_ptr() + 4 * case.N if case.joint else d[1].data_ptr()
    return d, d[0].data_ptr(), ld, p2, ld2


def _lse_call(case, S, S2, dev):
    ops = _ops()
    keep, pS, ld, pS2, ld2 = _inputs_on_device(case, S, S2, dev)
    n = case.N if case.kind == "col" else case.M
    lse, pos = _Out(n, dev), _Out(n, dev)
    rc = ops._lib().clipk_ce_logits_lse(pS, ld, case.M, case.N, pS2, ld2, case.N2, int(case.kind == "col"), case.off,
                                        lse.ptr, pos.ptr, ops._stream())
    assert rc == 0, (case.name, rc)
    torch.cuda.synchronize()
    every = torch.ones(n, dtype=torch.bool)
    assert lse.untouched_outside(every) and pos.untouched_outside(every), f"{case.name}: a fence was written"
    return {"lse": lse.read(), "pos": pos.read()}


def _bwd_call(case, S, S2, dev):
    ops = _ops()
    M, N, N2 = case.M, case.N, case.N2
    keep, pS, ld, pS2, ld2 = _inputs_on_device(case, S, S2, dev)
    lr, lc, wr, wc = R.lse_inputs(case, S, S2)
    lrd, lcd = (None if lr is None else lr.to(dev)), (None if lc is None else lc.to(dev))
    g = torch.tensor([R.G], dtype=torch.float32, device=dev)
    extra = R.PAD if case.pad else 0
    if case.joint:
        ldd = ldd2 = N + N2 + extra
        o1 = _Out(M * ldd, dev)
        o2, p2 = o1, o1.ptr + 4 * N
        w1 = _rows_mask(M, ldd, 0, N) | _rows_mask(M, ldd, N, N2)
        w2 = w1
    else:
        ldd, ldd2 = N + extra, (N2 + extra if N2 else 0)
        o1 = _Out(M * ldd, dev)
        o2 = _Out(M * ldd2, dev) if N2 else None
        p2 = o2.ptr if N2 else None
        w1, w2 = _rows_mask(M, ldd, 0, N), (_rows_mask(M, ldd2, 0, N2) if N2 else None)
    rc = ops._lib().clipk_ce_logits_bwd(pS, ld, M, N, pS2, ld2, N2, ops.ptr(lrd), ops.ptr(lcd), wr, wc, case.off, case.off_c,
                                        g.data_ptr(), o1.ptr, ldd, p2, ldd2, ops._stream())
    assert rc == 0, (case.name, rc)
    torch.cuda.synchronize()
    assert o1.untouched_outside(w1) and (o2 is None or o2.untouched_outside(w2)), f"{case.name}: a pad or a fence was written"
    dS = o1.read().view(M, ldd)[:, :N].clone()
    dS2 = None
    if N2:
        dS2 = (o1.read().view(M, ldd)[:, N:N + N2] if case.joint else o2.read().view(M, ldd2)[:, :N2]).clone()
    return {"dS": dS, "dS2": dS2}


def _compare(case, ref, st, got, again):
    for nm, r in ref.items():
        if r is None:
            assert got[nm] is None
            continue
        cmp = ~torch.isnan(r)
        assert R.bit_equal(got[nm][cmp], again[nm][cmp]), f"{case.name} {nm}: two calls, different bits"
        if nm == "pos":
            assert R.bit_equal(got[nm], r.float()), f"{case.name}: pos is not the logit's bits"
            continue
        _note(case, nm, R.check(got[nm], r, st[nm], f"{case.name} {nm}"))
        if case.family == "onehot":
            assert torch.equal(got[nm][cmp], st[nm][cmp]), f"{case.name} {nm}: onehot is exact"
            if nm == "lse":
                assert R.bit_equal(got[nm], r.float()), f"{case.name}: lse of one finite logit is that logit"
    if case.kind == "bwd" and case.weights == "col" and case.N2:
        assert (got["dS2"] == 0).all(), f"{case.name}: dS2 without a row direction"


def _walk(dev, kind, family):
    """Every case of the kernel and family; the value failures are gathered and reported together."""
    call = _bwd_call if kind == "bwd" else _lse_call
    cases = [c for c in R.CASES if c.kind == kind and c.family == family]
    assert cases
    failed = []
    for case in cases:
        S, S2 = R.inputs(case)
        ref, st = R.reference(case, S, S2), R.restate(case, S, S2)
        got, again = call(case, S, S2, dev), call(case, S, S2, dev)
        try:
            _compare(case, ref, st, got, again)
        except AssertionError as e:
            nans = {nm: int(torch.isnan(t).sum()) for nm, t in got.items() if t is not None}
            failed.append(f"{case.name}: {e}"[:300] + f"  (NaN count {nans})")
    assert not failed, f"{len(failed)} of {len(cases)} cases:\n" + "\n".join(failed[:12])


@pytest.mark.parametrize("family", R.FAMILIES)
def test_row_lse(dev, family):
    """ce_lse_row_kernel: M in {1, 3, 4, 5, 9} x N in {1, 2, 63, 64, 65, 129, 200} x N2 in {0, 1, 63, 64, 130} and the offset
    shapes; holes and onehot are the -inf cases: NaN before the fix wherever a lane met -inf before a finite logit."""
    _walk(dev, "row", family)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_col_lse(dev, family):
    """ce_lse_col_kernel: N in {1, 63, 64, 65, 130} x M in {1, 2, 3, 4, 5, 9, 67} (M < 4: empty row slices; 67: 17 trips
    and a ragged last one) and the offset shapes."""
    _walk(dev, "col", family)


@pytest.mark.parametrize("family", R.FAMILIES)
def test_bwd(dev, family):
    """ce_bwd_kernel: N in {1, 255, 256, 257, 513} x N2 in {0, 1, 300, 600} (nmax from either side) x the three weightings,
    M in {1, 3, 5, 6}, and off_r x off_c in {0, 3, -3, N}^2 on rectangular S."""
    _walk(dev, "bwd", family)


# ------------------------------------------------------------------------------------------------ the autograd function
def _kf_inputs(kind, B, Nc):
    g = torch.Generator().manual_seed(40 + B)
    x = torch.randn(B, B + Nc, generator=g, dtype=torch.float64) * 4
    if kind == "peaked":
        x = -60 + x / 8
        k = torch.arange(B)
        x[k, (k * 7 + 63) % (B + Nc)] = 60 + 20 * torch.rand(B, generator=g, dtype=torch.float64)
        x[(k * 5 + 3) % B, k] = 60 + 20 * torch.rand(B, generator=g, dtype=torch.float64)
    else:
        # masked pairs off the diagonal (the loss stays finite): column 0 below the first row, lane 5 of every row but the
        # two whose label it is, all cache columns of the even rows
        x[1:, 0] = -R.INF
        for j in range(5, B, 64):
            x[torch.arange(B) != j, j] = -R.INF
        x[0::2, B:] = -R.INF
    return x.float()


@pytest.mark.parametrize("view", ["separate", "one_buffer"])
@pytest.mark.parametrize("kind", ["holes", "peaked"])
def test_cross_entropy_diag_matches_f64_autograd(dev, kind, view):
    """KF.cross_entropy_diag (CEDiagFn: row LSE over [S | cache], column LSE, fused backward; (0.5, 0.5) and (1, 0)) on
    masked and on peaked logits: loss and both gradients against f64 autograd of F.cross_entropy, by the rule, the f32
    autograd of the same on the CPU as the restatement.  one_buffer: logits and cache are the non-contiguous column blocks
    big[:, :B] and big[:, B:] of one matrix (row stride B + Nc, no copy)."""
    from clip_dplm_amd import functional as KF
    B, Nc = 70, 37
    x = _kf_inputs(kind, B, Nc)
    lab = torch.arange(B)
    for symmetric in (True, False):
        def torch_loss(dt):
            S, S2 = x[:, :B].to(dt).requires_grad_(True), x[:, B:].to(dt).requires_grad_(True)
            loss = F.cross_entropy(torch.cat([S, S2], 1), lab)
            if symmetric:
                loss = 0.5 * (loss + F.cross_entropy(S.t(), lab))
            gS, gS2 = torch.autograd.grad(loss * 1.7, [S, S2])
            return loss.detach(), gS, gS2
        ref, st = torch_loss(torch.float64), torch_loss(torch.float32)
        assert all(torch.isfinite(t).all() for t in ref)
        if view == "one_buffer":
            big = x.to(dev).requires_grad_(True)
            S, S2 = big[:, :B], big[:, B:]
            assert not S.is_contiguous() and S.stride(0) == B + Nc
        else:
            S, S2 = x[:, :B].contiguous().to(dev).requires_grad_(True), x[:, B:].contiguous().to(dev).requires_grad_(True)
        loss = KF.cross_entropy_diag(S, S2, symmetric=symmetric)
        (loss * 1.7).backward()
        gS, gS2 = (big.grad[:, :B], big.grad[:, B:]) if view == "one_buffer" else (S.grad, S2.grad)
        for nm, got, r, s in zip(("loss", "dS", "dS2"), (loss.detach(), gS, gS2), ref, st):
            R.check(got, r, s, f"cross_entropy_diag {kind} {view} symmetric={symmetric} {nm}")


# ------------------------------------------------------------------------------------------------ refusals, grid limit
def test_refusals_leave_the_outputs_alone(dev):
    """clipk_ce_logits_lse: NULL S / lse / pos, M or N <= 0, N2 < 0, N2 > 0 without S2 -> BAD_ARG; columns with N2 > 0 ->
    UNSUPPORTED.  clipk_ce_logits_bwd: NULL S / dS / g, bad dims, N2 > 0 without S2 or dS2 -> BAD_ARG.  Nothing written."""
    ops = _ops()
    lib, st = ops._lib(), ops._stream()
    M, N, N2 = 5, 7, 3
    S = torch.zeros(M, N, device=dev)
    S2 = torch.zeros(M, N2, device=dev)
    lr, g = torch.zeros(M, device=dev), torch.ones(1, device=dev)
    lse, pos, dS, dS2 = _Out(M, dev), _Out(M, dev), _Out(M * N, dev), _Out(M * N2, dev)
    p, p2 = S.data_ptr(), S2.data_ptr()
    calls = [
        (BAD_ARG, lambda: lib.clipk_ce_logits_lse(None, N, M, N, None, 0, 0, 0, 0, lse.ptr, pos.ptr, st)),
        (BAD_ARG, lambda: lib.clipk_ce_logits_lse(p, N, M, N, None, 0, 0, 0, 0, None, pos.ptr, st)),
        (BAD_ARG, lambda: lib.clipk_ce_logits_lse(p, N, M, N, None, 0, 0, 0, 0, lse.ptr, None, st)),
        (BAD_ARG, lambda: lib.clipk_ce_logits_lse(p, N, 0, N, None, 0, 0, 0, 0, lse.ptr, pos.ptr, st)),
        (BAD_ARG, lambda: lib.clipk_ce_logits_lse(p, N, M, 0, None, 0, 0, 0, 0, lse.ptr, pos.ptr, st)),
        (BAD_ARG, lambda: lib.clipk_ce_logits_lse(p, N, M, N, p2, N2, -1, 0, 0, lse.ptr, pos.ptr, st)),
        (BAD_ARG, lambda: lib.clipk_ce_logits_lse(p, N, M, N, None, N2, N2, 0, 0, lse.ptr, pos.ptr, st)),
        (UNSUPPORTED, lambda: lib.clipk_ce_logits_lse(p, N, M, N, p2, N2, N2, 1, 0, lse.ptr, pos.ptr, st)),
        (BAD_ARG, lambda: lib.clipk_ce_logits_bwd(None, N, M, N, None, 0, 0, lr.data_ptr(), None, 1.0, 0.0, 0, 0, g.data_ptr(),
                                                  dS.ptr, N, None, 0, st)),
        (BAD_ARG, lambda: lib.clipk_ce_logits_bwd(p, N, M, N, None, 0, 0, lr.data_ptr(), None, 1.0, 0.0, 0, 0, g.data_ptr(),
                                                  None, N, None, 0, st)),
        (BAD_ARG, lambda: lib.clipk_ce_logits_bwd(p, N, M, N, None, 0, 0, lr.data_ptr(), None, 1.0, 0.0, 0, 0, None,
                                                  dS.ptr, N, None, 0, st)),
        (BAD_ARG, lambda: lib.clipk_ce_logits_bwd(p, N, 0, N, None, 0, 0, lr.data_ptr(), None, 1.0, 0.0, 0, 0, g.data_ptr(),
                                                  dS.ptr, N, None, 0, st)),
        (BAD_ARG, lambda: lib.clipk_ce_logits_bwd(p, N, M, N, None, N2, N2, lr.data_ptr(), None, 1.0, 0.0, 0, 0, g.data_ptr(),
                                                  dS.ptr, N, dS2.ptr, N2, st)),
        (BAD_ARG, lambda: lib.clipk_ce_logits_bwd(p, N, M, N, p2, N2, N2, lr.data_ptr(), None, 1.0, 0.0, 0, 0, g.data_ptr(),
                                                  dS.ptr, N, None, N2, st)),
    ]
    for k, (want, fn) in enumerate(calls):
        assert fn() == want, f"call {k}"
    torch.cuda.synchronize()
    for o in (lse, pos, dS, dS2):
        assert o.untouched_outside(torch.zeros(o.n, dtype=torch.bool))


def test_more_rows_than_grid_y(dev):
    """M = 65 536, N = 1: one row more than grid y holds.  The backward walks its rows with a grid-stride loop (before: a
    launch error), so it accepts what the forward accepts: row LSE, column LSE (16 384 trips per row slice) and the
    backward with both directions, against f64, the plain f32 formulas on the CPU as the restatement."""
    ops = _ops()
    lib, st = ops._lib(), ops._stream()
    M = 65536
    g = torch.Generator().manual_seed(77)
    S = (torch.randn(M, 1, generator=g, dtype=torch.float64) * 4).float()
    Sd = S.to(dev)
    out = {}
    for columns in (0, 1):
        n = 1 if columns else M
        lse, pos = _Out(n, dev), _Out(n, dev)
        assert lib.clipk_ce_logits_lse(Sd.data_ptr(), 1, M, 1, None, 0, 0, columns, 0, lse.ptr, pos.ptr, st) == 0
        torch.cuda.synchronize()
        every = torch.ones(n, dtype=torch.bool)
        assert lse.untouched_outside(every) and pos.untouched_outside(every)
        rl, rp = R.lse_cols(S, 0) if columns else R.lse_rows(S, None, 0)
        restated = torch.logsumexp(S, 0) if columns else torch.logsumexp(S, 1)
        R.check(lse.read(), rl, restated, f"M = 65536 lse columns={columns}")
        assert R.bit_equal(pos.read(), rp.float())
        out[columns] = lse.buf[GUARD:GUARD + n]
    case = R._mk("bwd", "generic", 0, M, 1, 0, 0, 0, "both")
    lr, lc = out[0].cpu(), out[1].cpu()
    dS = _Out(M, dev)
    gd = torch.tensor([R.G], dtype=torch.float32, device=dev)
    assert lib.clipk_ce_logits_bwd(Sd.data_ptr(), 1, M, 1, None, 0, 0, out[0].data_ptr(), out[1].data_ptr(), 0.5, 0.5, 0, 0,
                                   gd.data_ptr(), dS.ptr, 1, None, 0, st) == 0
    torch.cuda.synchronize()
    assert dS.untouched_outside(torch.ones(M, dtype=torch.bool))
    ref, _ = R.bwd(S, None, lr, lc, 0.5, 0.5, 0, 0, R.G)
    R.check(dS.read().view(M, 1), ref, R.restate_bwd(S, None, lr, lc, 0.5, 0.5, 0, 0, R.G)["dS"], f"{case.name} dS")
    assert float(ref[M - 1].abs()) > 0                       # the row past the old limit has a gradient to get wrong
