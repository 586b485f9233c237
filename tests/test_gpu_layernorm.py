"""GPU: the LayerNorm family of csrc/rowwise.hip (forward with fused activation, first and second backward, LayerNorm + mean
pooling, the deferred parameter-gradient reduce) against the plain f64 references and the tolerances of
tests/layernorm_ref.py (pinned on the CPU by tests/test_layernorm_ref_host.py), branch by branch: every register width
(VPL 2 / 4 / 8 / 20) and both one-workgroup-per-row (NW = 4) instantiations on either side of each dispatch boundary, every accepted
(dy, x, dx_add) type triple, the second trip of every grid-stride loop, the dropout multiply, strides, refusals.  Every
input comes from a seeded CPU generator; each docstring names the branch the test exists for.  What the dispatch promises
exactly (bf16 = RNE of the f32 output, outputs independent of which are asked for, rows independent of the batch, the
dropout hash) is compared bit for bit.
"""
import numpy as np
import pytest
import torch

import elementwise_ref as E
import layernorm_ref as R
import ops_emulator as EMU

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF = torch.bfloat16
WIDTHS = [4, 8, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 5120]   # VPL 2 | 4 | 8 | wide (f32) or VPL 20, both sides of each
ROWS = [1, 3, 4, 5, 9]                  # 1: three idle waves; 4 | 5: one block | two; 9: three blocks, the last with one row
BAD_ARG, UNSUPPORTED = -1, -2           # include/clipk.h
GUARD = 16
# accepted (dy, x, dx_add) types -> the kernel instantiation at cols <= 2048 (beyond: ln_bwd_kernel<5, 4> for f32 / f32, VPL 20 else)
TRIPLES = [("f32", "f32", None), ("f32", "f32", "f32"),          # launch_ln_bwd<V, false, false>
           ("f32", "bf16", "f32"),                               # <V, false, true>
           ("bf16", "bf16", None), ("bf16", "bf16", "f32"),      # <V, true, true>
           ("bf16", "f32", "f32"),                               # <V, true, false>
           ("bf16", "f32", "bf16")]                              # <V, true, false, true> (ADD16): the res16 training path
DT = {"f32": torch.float32, "bf16": BF}


def _ops():
    from clip_dplm_amd import ops
    return ops


def _within(got, ref, tol, what=""):
    """|got - ref| <= tol per element (tol may be 0 where the reference is an exact 0), the worst ratio in the message."""
    got = got.detach().cpu().to(F64)
    err = (got - ref).abs()
    assert torch.isfinite(got).all(), what
    tol = tol * torch.ones_like(err)
    assert (err <= tol).all(), f"{what}: worst |err| / bound = {float((err / tol.clamp(min=1e-300)).max()):.3f}"


def _same(a, b):
    """Bitwise equality of two tensors of one dtype (NaN-safe, -0 != +0)."""
    if a.dtype == BF:
        return np.array_equal(E.bf16_bits(a), E.bf16_bits(b))
    return np.array_equal(E.f32_bits(a), E.f32_bits(b))


def _is_rne(x16, x32):
    return np.array_equal(E.bf16_bits(x16), E.bf16_rne_bits(E.f32_bits(x32)))


def _cast(t, kind, dev):
    """CPU f32 tensor -> device tensor of the named type (None stays None)."""
    return None if (t is None or kind is None) else t.to(DT[kind]).to(dev)


def _seen(t, kind):
    """The values the kernel sees: t rounded to bf16 where it is passed as bf16 (f32 CPU tensor)."""
    return None if (t is None or kind is None) else (t.to(BF).to(torch.float32) if kind == "bf16" else t)


def _acts(xbf16):
    combos = [(None, 1e-12), ("gelu", 1e-5)]
    if not xbf16:
        combos += [("celu", 1e-5), ("softplus", 1e-12)]
    return combos


# ------------------------------------------------------------------------------------------------ forward
def _check_fwd(dev, fam, rows, cols, xbf16, act, eps0, seed=50):
    ops = _ops()
    x, eps = R.family(fam, rows, cols, seed, eps0, xbf16)
    gamma, beta = R.params(cols, seed + 1)
    y32, y16, mean, rstd = ops.layernorm_fwd(_cast(x, "bf16" if xbf16 else "f32", dev), gamma.to(dev), beta.to(dev), eps,
                                             act=act, want_f32=True, want_bf16=True)
    yr, mr, rr = R.layernorm(x, gamma, beta, eps, act)
    b = R.bounds(x, gamma, beta, eps, act, fam=fam)
    tag = f"{fam} {rows}x{cols} bf16={xbf16} act={act} eps={eps}"
    _within(y32, yr, b["y"], "y " + tag)
    _within(mean, mr, b["mean"], "mean " + tag)
    _within(rstd, rr, b["rstd"], "rstd " + tag)
    assert _is_rne(y16, y32), "y16 != RNE(y32) " + tag
    return x, mean


@pytest.mark.parametrize("fam,xbf16", [(f, False) for f in R.FAMILIES] + [(f, True) for f in "abc"])
@pytest.mark.parametrize("cols", WIDTHS)
def test_forward_every_width_and_family(dev, cols, fam, xbf16):
    """ln_fwd_kernel<2 | 4 | 8, 1> and ln_fwd_kernel<5, 4> (cols 2052, 5120), f32 and bf16 x, on both sides of every dispatch
    boundary, rows 1 .. 9 (a lone row leaves three waves of its block idle), None / gelu (+ celu / softplus on f32), eps 1e-12
    and 1e-5: y32, mean, rstd within layernorm_ref.bounds of f64 on N(0, 4), offset 100 (|mean| >> std: the two-pass
    variance), std 1e-3 against eps 1e-5, and one constant row (finite outputs, mean within 2 ulp of the constant);
    y16 == RNE(y32) bit for bit."""
    for rows in ROWS:
        for act, eps0 in _acts(xbf16):
            x, mean = _check_fwd(dev, fam, rows, cols, xbf16, act, eps0)
            if fam == "d":
                c = np.float32(R.CONST)
                got = mean.cpu().numpy()[rows // 2]
                assert abs(float(got) - float(c)) <= 2.0 * float(np.spacing(c)), (rows, cols, float(got))


@pytest.mark.parametrize("xbf16", [False, True])
@pytest.mark.parametrize("rows,cols", [(8197, 8), (2053, 2052)])
def test_forward_second_grid_stride_trip(dev, rows, cols, xbf16):
    """The forward grids are capped at 2048 blocks: rows > 8192 send the first waves of ln_fwd_kernel<V, 1> round `row += row_step`
    again (rows 8192 .. 8196), rows > 2048 the first blocks of ln_fwd_kernel<5, 4> round it (row_step = gridDim.x).  Against f64, and
    the last row bit for bit against a 1-row call."""
    ops = _ops()
    _check_fwd(dev, "a", rows, cols, xbf16, None, 1e-5, seed=60)
    x, eps = R.family("a", rows, cols, 60, 1e-5, xbf16)
    gamma, beta = R.params(cols, 61)
    xd, g, b = _cast(x, "bf16" if xbf16 else "f32", dev), gamma.to(dev), beta.to(dev)
    full = ops.layernorm_fwd(xd, g, b, eps, want_bf16=True)
    for r in (0, rows - 5, rows - 1):
        one = ops.layernorm_fwd(xd[r:r + 1], g, b, eps, want_bf16=True)
        assert all(_same(f[r:r + 1], o) for f, o in zip(full, one)), r


@pytest.mark.parametrize("xbf16", [False, True])
@pytest.mark.parametrize("cols", WIDTHS)
def test_forward_outputs_do_not_depend_on_what_is_asked_for_or_on_the_batch(dev, cols, xbf16):
    """clipk_layernorm_fwd with y_f32 only, y_bf16 only, no statistics (the null-pointer branches of both forward kernels)
    gives the bits of the call asking for everything; row r of a 9-row call equals the 1-row call on that row (the
    dispatch comment: a row's arithmetic never depends on the batch)."""
    ops = _ops()
    x, eps = R.family("a", 9, cols, 70, 1e-5, xbf16)
    gamma, beta = R.params(cols, 71)
    xd, g, b = _cast(x, "bf16" if xbf16 else "f32", dev), gamma.to(dev), beta.to(dev)
    y32, y16, mean, rstd = ops.layernorm_fwd(xd, g, b, eps, act="gelu", want_f32=True, want_bf16=True)
    a32, a16, am, ar = ops.layernorm_fwd(xd, g, b, eps, act="gelu", want_f32=True, want_bf16=False, want_stats=False)
    assert a16 is None and am is None and ar is None and _same(a32, y32)
    b32, b16, bm, br = ops.layernorm_fwd(xd, g, b, eps, act="gelu", want_f32=False, want_bf16=True)
    assert b32 is None and _same(b16, y16) and _same(bm, mean) and _same(br, rstd)
    c32, c16, _, _ = ops.layernorm_fwd(xd, g, b, eps, act="gelu", want_f32=False, want_bf16=True, want_stats=False)
    assert _same(c16, y16)
    for r in range(9):
        o32, o16, om, orr = ops.layernorm_fwd(xd[r:r + 1], g, b, eps, act="gelu", want_f32=True, want_bf16=True)
        assert _same(o32, y32[r:r + 1]) and _same(o16, y16[r:r + 1]) and _same(om, mean[r:r + 1]) and _same(orr, rstd[r:r + 1]), r


# ------------------------------------------------------------------------------------------------ backward
def _bwd_case(dev, fam, rows, cols, triple, act, seed=80, eps0=1e-5):
    """Inputs of one backward case on the device + the values the kernel sees on the CPU."""
    ops = _ops()
    dyk, xk, addk = triple
    x, eps = R.family(fam, rows, cols, seed, eps0, xk == "bf16")
    gamma, beta = R.params(cols, seed + 1)
    dy = _seen(R.randn((rows, cols), seed + 2), dyk)
    add = _seen(R.randn((rows, cols), seed + 3), addk)
    dev_in = dict(dy=_cast(dy, dyk, dev), x=_cast(x, xk, dev), gamma=gamma.to(dev), beta=beta.to(dev), add=_cast(add, addk, dev))
    _, _, mean, rstd = ops.layernorm_fwd(dev_in["x"], dev_in["gamma"], dev_in["beta"], eps, act=act)
    dev_in.update(mean=mean, rstd=rstd)
    return dev_in, dict(dy=dy, x=x, gamma=gamma, beta=beta, add=add, eps=eps)


def _bwd(d, act, **kw):
    return _ops().layernorm_bwd(d["dy"], d["x"], d["gamma"], d["beta"], d["mean"], d["rstd"], act=act, dx_add=d["add"], **kw)


def _check_bwd(dev, fam, rows, cols, triple, act, seed=80):
    d, c = _bwd_case(dev, fam, rows, cols, triple, act, seed)
    dx32, dx16, dg, db = _bwd(d, act, want_f32=True, want_bf16=True)
    dxr, dgr, dbr = R.layernorm_bwd(c["dy"], c["x"], c["gamma"], c["beta"], c["eps"], act, dx_add=c["add"])
    b = R.bounds(c["x"], c["gamma"], c["beta"], c["eps"], act, dy=c["dy"], dx_add=c["add"], add_bf16=triple[2] == "bf16", fam=fam)
    tag = f"{fam} {rows}x{cols} {triple} act={act}"
    _within(dx32, dxr, b["dx"], "dx " + tag)
    _within(dg, dgr, b["dgamma"], "dgamma " + tag)
    _within(db, dbr, b["dbeta"], "dbeta " + tag)
    assert _is_rne(dx16, dx32), "dx16 != RNE(dx32) " + tag
    return d, c, (dx32, dx16, dg, db), (dxr, dgr, dbr, b)


@pytest.mark.parametrize("triple", TRIPLES, ids=lambda t: "-".join(str(k) for k in t))
@pytest.mark.parametrize("cols", WIDTHS)
def test_backward_every_type_triple_at_every_width(dev, cols, triple):
    """The four launch_ln_bwd type instantiations and ADD16 at VPL 2 / 4 / 8, ln_bwd_kernel<5, 4> for the f32 triples at
    cols 2052 / 5120 and VPL 20 (160 KiB of dynamic LDS at 5120) for the others; rows 1 .. 9; families (a) - (d) without an
    activation, gelu on (a) and (c) (layernorm_ref.ACT_BWD_FAMILIES).  dx32, dgamma, dbeta within layernorm_ref.bounds of
    the f64 closed form on the values the kernel sees, mean / rstd from the kernel's own forward; dx16 == RNE(dx32)."""
    fams = "abc" if triple[1] == "bf16" else "abcd"
    for rows in ROWS:
        for fam in fams:
            _check_bwd(dev, fam, rows, cols, triple, None)
            if fam in R.ACT_BWD_FAMILIES:
                _check_bwd(dev, fam, rows, cols, triple, "gelu")


@pytest.mark.parametrize("triple", [TRIPLES[1], TRIPLES[4], TRIPLES[6]], ids=lambda t: "-".join(str(k) for k in t))
@pytest.mark.parametrize("cols", WIDTHS)
def test_backward_call_forms_are_bitwise_consistent(dev, cols, triple):
    """clipk_layernorm_bwd's argument branches, narrow and wide: the accumulate form adds the same column sums to what
    dgamma / dbeta hold; want_param_grads=False skips the reduce and changes no dx bit; a bf16-only call (dx_f32 = NULL) and
    an f32-only call give the halves of the both-outputs call; a second call repeats every bit; row r of the 9-row call
    equals the 1-row call on that row."""
    ops = _ops()
    d, c = _bwd_case(dev, "a", 9, cols, triple, "gelu", seed=90)
    dx32, dx16, dg, db = _bwd(d, "gelu", want_f32=True, want_bf16=True)
    again = _bwd(d, "gelu", want_f32=True, want_bf16=True)
    assert all(_same(a, b) for a, b in zip(again, (dx32, dx16, dg, db)))
    dg0, db0 = R.randn((cols,), 95).to(dev), R.randn((cols,), 96).to(dev)
    dga, dba = dg0.clone(), db0.clone()
    _bwd(d, "gelu", dgamma=dga, dbeta=dba, accumulate=True)
    assert _same(dga, dg0 + dg) and _same(dba, db0 + db)
    dgw, dbw = dg0.clone(), db0.clone()
    _bwd(d, "gelu", dgamma=dgw, dbeta=dbw, accumulate=False)
    assert _same(dgw, dg) and _same(dbw, db)
    n32, n16, ng, nb = _bwd(d, "gelu", want_f32=True, want_bf16=True, want_param_grads=False)
    assert ng is None and nb is None and _same(n32, dx32) and _same(n16, dx16)
    h32, h16, _, _ = _bwd(d, "gelu", want_f32=False, want_bf16=True)
    assert h32 is None and _same(h16, dx16)
    f32_, f16, _, _ = _bwd(d, "gelu", want_f32=True, want_bf16=False)
    assert f16 is None and _same(f32_, dx32)
    for r in range(9):
        one = {k: (v[r:r + 1] if (v is not None and k not in ("gamma", "beta")) else v) for k, v in d.items()}
        o32, o16, _, _ = _bwd(one, "gelu", want_f32=True, want_bf16=True)
        assert _same(o32, dx32[r:r + 1]) and _same(o16, dx16[r:r + 1]), r


GRID_STRIDE_BWD = [(5125, 8, TRIPLES[1]),        # cols <= 512: 1280 blocks
                   (5125, 8, TRIPLES[6]),
                   (3077, 516, TRIPLES[6]),      # cols <= 1024: 768 blocks
                   (2053, 1028, TRIPLES[4]),     # beyond: 512 blocks
                   (2053, 2052, TRIPLES[1])]     # ln_bwd_kernel<5, 4>: row_step = gridDim.x


@pytest.mark.parametrize("rows,cols,triple", GRID_STRIDE_BWD, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_backward_second_grid_stride_trip_with_dropout(dev, rows, cols, triple):
    """The backward grids are capped at 1280 / 768 / 512 blocks: with rows just past four times the cap the first waves
    (blocks, in the wide kernel) take a second row, whose gradients join the same per-block dgamma / dbeta partials and whose
    dropout mask index is row * cols + col.  dx32 / dgamma / dbeta against f64; dx16 == RNE(dx32 * m) bit for bit with m
    from ops_emulator.drop_mult, dx32 unmasked; the last row bit for bit against a 1-row call (no dropout)."""
    d, c, (dx32, dx16, dg, db), _ = _check_bwd(dev, "a", rows, cols, triple, None, seed=100)
    _check_dropout(d, dx32, dg, db, rows, cols)
    one = {k: (v[rows - 1:] if (v is not None and k not in ("gamma", "beta")) else v) for k, v in d.items()}
    o32, o16, _, _ = _bwd(one, None, want_f32=True, want_bf16=True)
    assert _same(o32, dx32[rows - 1:]) and _same(o16, dx16[rows - 1:])


# ------------------------------------------------------------------------------------------------ dropout
P_DROP, SEED_DROP = 0.1, 99


def _drop_mask(rows, cols, p=P_DROP, seed=SEED_DROP):
    """keep * scale as f32 [rows, cols]: the emulator's hash at index row * cols + col; the scale is f32 1 / (1 - p) as
    clipk_layernorm_bwd computes it on the host."""
    keep = EMU.drop_mult(p, seed, torch.arange(rows * cols, dtype=torch.int64).view(rows, cols)) != 0
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return keep.to(torch.float32) * float(scale)


def _check_dropout(d, dx32, dg, db, rows, cols, act=None):
    m32, m16, mg, mb = _bwd(d, act, want_f32=True, want_bf16=True, dropout_bf16=(P_DROP, SEED_DROP))
    assert _same(m32, dx32) and _same(mg, dg) and _same(mb, db), "dropout touched the f32 output or the parameter gradients"
    want = E.bf16_rne_bits(E.f32_bits(dx32.cpu() * _drop_mask(rows, cols)))
    got = E.bf16_bits(m16)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} of {rows * cols} elements differ, first at {bad[0]}"
    kept = float((_drop_mask(rows, cols) != 0).to(F64).mean())
    assert rows * cols < 1000 or abs(kept - (1 - P_DROP)) < 0.02, kept


@pytest.mark.parametrize("rows,cols,triple", [(9, 4, TRIPLES[6]), (9, 516, TRIPLES[6]), (5, 1028, TRIPLES[3]), (9, 2052, TRIPLES[6]),
                                              (9, 2052, TRIPLES[1]), (5, 5120, TRIPLES[0])],
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_backward_dropout_mask_is_the_emulators_hash(dev, rows, cols, triple):
    """The dropout multiply on the bf16 output of ln_bwd_kernel<V, 1> (ADD16 path of encoders._post_layer_bwd among the cases) and
    of ln_bwd_kernel<5, 4>: dx16 == RNE(dx32 * m) bit for bit, m = ops_emulator.drop_mult(0.1, 99) at row * cols + col scaled
    by f32 1 / (1 - p); dx32, dgamma, dbeta unmasked; a bf16-only call gives the same bits; p = 0 is the no-dropout result."""
    d, c, (dx32, dx16, dg, db), _ = _check_bwd(dev, "a", rows, cols, triple, "gelu", seed=110)
    _check_dropout(d, dx32, dg, db, rows, cols, act="gelu")
    _, m16, _, _ = _bwd(d, "gelu", want_f32=True, want_bf16=True, dropout_bf16=(P_DROP, SEED_DROP))
    _, h16, _, _ = _bwd(d, "gelu", want_f32=False, want_bf16=True, dropout_bf16=(P_DROP, SEED_DROP))
    assert _same(h16, m16)
    _, z16, _, _ = _bwd(d, "gelu", want_f32=True, want_bf16=True, dropout_bf16=(0.0, SEED_DROP))
    assert _same(z16, dx16)


# ------------------------------------------------------------------------------------------------ strides
def _padded(t, pad, dev):
    """t [rows, cols] as a view of a [rows, cols + pad] device buffer whose padding holds NaN."""
    rows, cols = t.shape
    buf = torch.full((rows, cols + pad), float("nan"), dtype=t.dtype, device=dev)
    buf[:, :cols] = t.to(dev)
    return buf[:, :cols]


@pytest.mark.parametrize("triple", [TRIPLES[1], TRIPLES[4], TRIPLES[6]], ids=lambda t: "-".join(str(k) for k in t))
@pytest.mark.parametrize("cols", [4, 260, 1028, 2052])
def test_strided_inputs_through_ops(dev, cols, triple):
    """ldx / lddy > cols in every kernel: x and dy are views of buffers cols + 4 / cols + 8 wide whose padding holds NaN, so a
    read at row * cols (or past a row's end) poisons a row sum.  Same bits as the contiguous call, forward and backward."""
    ops = _ops()
    d, c = _bwd_case(dev, "a", 5, cols, triple, "gelu", seed=120)
    xs, dys = _padded(d["x"], 4, dev), _padded(d["dy"], 8, dev)
    assert xs.stride(0) == cols + 4 and dys.stride(0) == cols + 8
    want = ops.layernorm_fwd(d["x"], d["gamma"], d["beta"], c["eps"], act="gelu", want_bf16=True)
    got = ops.layernorm_fwd(xs, d["gamma"], d["beta"], c["eps"], act="gelu", want_bf16=True)
    assert all(_same(a, b) for a, b in zip(got, want))
    wantb = _bwd(d, "gelu", want_f32=True, want_bf16=True, dropout_bf16=(P_DROP, SEED_DROP))
    gotb = _bwd(dict(d, x=xs, dy=dys), "gelu", want_f32=True, want_bf16=True, dropout_bf16=(P_DROP, SEED_DROP))
    assert all(_same(a, b) for a, b in zip(gotb, wantb))


def _sentinel(rows, ld, dtype, dev):
    """(rows + 16) x ld buffer of a sentinel pattern (f32 0x5a5a5a5a, bf16 0x5a5a)."""
    if dtype == torch.float32:
        return torch.full((rows + GUARD, ld), 0x5a5a5a5a, dtype=torch.int32, device=dev).view(torch.float32)
    return torch.full((rows + GUARD, ld), 0x5a5a, dtype=torch.int16, device=dev).view(BF)


def _untouched(buf, rows, cols):
    raw = buf.view(torch.int32 if buf.dtype == torch.float32 else torch.int16).cpu()
    s = 0x5a5a5a5a if buf.dtype == torch.float32 else 0x5a5a
    return bool((raw[:rows, cols:] == s).all()) and bool((raw[rows:] == s).all())


@pytest.mark.parametrize("xk", ["f32", "bf16"])
@pytest.mark.parametrize("rows,cols", [(5, 4), (5, 260), (9, 1028), (5, 2052)])
def test_forward_output_stride_through_the_c_abi(dev, rows, cols, xk):
    """clipk_layernorm_fwd with ldy = cols + 4 into sentinel-filled buffers with 16 guard rows (ops always passes
    ldy = cols): the values are those of the contiguous call, the padding columns and the guard rows keep the sentinel -
    no write past a row's end or past the output, narrow and wide kernel."""
    ops = _ops()
    x, eps = R.family("a", rows, cols, 130, 1e-5, xk == "bf16")
    gamma, beta = R.params(cols, 131)
    xd, g, b = _cast(x, xk, dev), gamma.to(dev), beta.to(dev)
    y32, y16, mean, rstd = ops.layernorm_fwd(xd, g, b, eps, act="gelu", want_bf16=True)
    ld = cols + 4
    o32, o16 = _sentinel(rows, ld, torch.float32, dev), _sentinel(rows, ld, BF, dev)
    st = _sentinel(2, rows, torch.float32, dev)                 # row 0: mean, row 1: rstd, then 16 guard rows
    rc = ops._lib().clipk_layernorm_fwd(xd.data_ptr(), ops._dt(xd), cols, g.data_ptr(), b.data_ptr(), eps, ops.ACT["gelu"],
                                        o32.data_ptr(), o16.data_ptr(), ld, st[0].data_ptr(), st[1].data_ptr(), rows, cols,
                                        ops._stream())
    assert rc == 0
    assert _same(o32[:rows, :cols], y32) and _same(o16[:rows, :cols], y16)
    assert _same(st[0], mean) and _same(st[1], rstd)
    assert _untouched(o32, rows, cols) and _untouched(o16, rows, cols) and _untouched(st, 2, rows)


def _raw_bwd(ops, dy, x, gamma, beta, mean, rstd, act, add, dx32, dx16, lddx, dgamma, dbeta, rows, cols, drop=(0.0, 0),
             lddy=None, ldx=None, ws=None):
    if ws is None:
        ws = torch.empty(ops._lib().clipk_layernorm_bwd_workspace(rows, cols), dtype=torch.uint8, device=x.device)
    return ops._lib().clipk_layernorm_bwd(dy.data_ptr(), ops._dt(dy), cols if lddy is None else lddy, x.data_ptr(), ops._dt(x),
                                          cols if ldx is None else ldx, gamma.data_ptr(), ops.ptr(beta), mean.data_ptr(),
                                          rstd.data_ptr(), ops.ACT[act], ops.ptr(add), ops._dt(add) if add is not None else 1,
                                          ops.ptr(dx32), ops.ptr(dx16), lddx, ops.ptr(dgamma), ops.ptr(dbeta), 0, rows, cols,
                                          float(drop[0]), int(drop[1]), ws.data_ptr(), ws.numel(), ops._stream())


@pytest.mark.parametrize("rows,cols,triple", [(5, 4, TRIPLES[6]), (5, 260, TRIPLES[6]), (9, 1028, TRIPLES[4]), (5, 2052, TRIPLES[1]),
                                              (5, 2052, TRIPLES[6])],
                         ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_backward_output_stride_through_the_c_abi(dev, rows, cols, triple):
    """clipk_layernorm_bwd with lddx = cols + 4 (dx_add, dx_f32 and dx_bf16 share it) into sentinel-filled buffers with 16
    guard rows, with dropout: same bits as the contiguous call - so the dropout index stays row * cols + col, not
    row * lddx + col - and padding columns, guard rows and the dgamma / dbeta guards keep the sentinel."""
    ops = _ops()
    d, c = _bwd_case(dev, "a", rows, cols, triple, "gelu", seed=140)
    w32, w16, wg, wb = _bwd(d, "gelu", want_f32=True, want_bf16=True, dropout_bf16=(P_DROP, SEED_DROP))
    ld = cols + 4
    o32, o16 = _sentinel(rows, ld, torch.float32, dev), _sentinel(rows, ld, BF, dev)
    pg = _sentinel(2, cols, torch.float32, dev)
    add = torch.full((rows, ld), float("nan"), dtype=d["add"].dtype, device=dev)
    add[:, :cols] = d["add"]
    rc = _raw_bwd(ops, d["dy"], d["x"], d["gamma"], d["beta"], d["mean"], d["rstd"], "gelu", add, o32, o16, ld, pg[0], pg[1],
                  rows, cols, drop=(P_DROP, SEED_DROP))
    assert rc == 0
    assert _same(o32[:rows, :cols], w32) and _same(o16[:rows, :cols], w16)
    assert _same(pg[0], wg) and _same(pg[1], wb)
    assert _untouched(o32, rows, cols) and _untouched(o16, rows, cols) and _untouched(pg, 2, cols)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(dev):
    """Every shape or type the LayerNorm entry points refuse instead of launching: cols % 4 != 0 and cols > 5120 (forward
    and backward), a stride that is no multiple of 4, a bf16 dx_add with anything but bf16 dy / f32 x, second order beyond
    2048 columns or with exactly one of d_gamma / d_beta, mean pooling whose four LDS rows pass 64 KiB (cols 4096).  The
    outputs keep their sentinel."""
    ops = _ops()
    lib = ops._lib()
    rows, big = 3, 5124
    x32 = torch.zeros((rows, big + 8), device=dev)
    x16 = x32.to(BF)
    g, b = torch.ones(big, device=dev), torch.zeros(big, device=dev)
    mean, rstd = torch.zeros(rows, device=dev), torch.ones(rows, device=dev)
    out32, out16 = _sentinel(rows, big + 8, torch.float32, dev), _sentinel(rows, big + 8, BF, dev)
    ws = torch.empty(lib.clipk_layernorm_bwd_workspace(rows, big), dtype=torch.uint8, device=dev)

    def fwd(cols, ldx=None, ldy=None, x=x32):
        return lib.clipk_layernorm_fwd(x.data_ptr(), ops._dt(x), cols if ldx is None else ldx, g.data_ptr(), b.data_ptr(), 1e-5,
                                       0, out32.data_ptr(), out16.data_ptr(), cols if ldy is None else ldy, mean.data_ptr(),
                                       rstd.data_ptr(), rows, cols, ops._stream())

    def bwd(cols, dy=x32, x=x32, add=None, lddy=None, ldx=None, lddx=None):
        return _raw_bwd(ops, dy, x, g, b, mean, rstd, None, add, out32, out16, cols if lddx is None else lddx, None, None, rows,
                        cols, lddy=lddy, ldx=ldx, ws=ws)

    for cols in (6, 5124):
        assert fwd(cols) == UNSUPPORTED and fwd(cols, x=x16) == UNSUPPORTED, cols
        assert bwd(cols) == UNSUPPORTED and bwd(cols, dy=x16, x=x16) == UNSUPPORTED, cols
        assert bwd(cols, dy=x16, add=x16) == UNSUPPORTED, cols
    assert fwd(8, ldx=10) == UNSUPPORTED and fwd(8, ldy=10) == UNSUPPORTED
    assert bwd(8, lddy=10) == UNSUPPORTED and bwd(8, ldx=10) == UNSUPPORTED and bwd(8, lddx=10) == UNSUPPORTED
    for dy, x in ((x32, x32), (x32, x16), (x16, x16)):                       # ADD16 exists for bf16 dy / f32 x only
        assert bwd(8, dy=dy, x=x, add=x16) == UNSUPPORTED
    assert bwd(8, dy=x16, x=x32, add=x16) == 0 and fwd(8) == 0               # ... and the neighbours are accepted
    out32.view(torch.int32).fill_(0x5a5a5a5a)
    out16.view(torch.int16).fill_(0x5a5a)

    def bwd2(cols, d_gamma, d_beta):
        return lib.clipk_layernorm_bwd2(x32.data_ptr(), x32.data_ptr(), x32.data_ptr(), cols, g.data_ptr(), b.data_ptr(),
                                        mean.data_ptr(), rstd.data_ptr(), 0, out32.data_ptr(), out32.data_ptr(), ops.ptr(d_gamma),
                                        ops.ptr(d_beta), 0, rows, cols, ws.data_ptr(), ws.numel(), ops._stream())

    dgm, dbt = _sentinel(1, 2052, torch.float32, dev)[0], _sentinel(1, 2052, torch.float32, dev)[0]
    assert bwd2(2052, dgm, dbt) == UNSUPPORTED and bwd2(2052, None, None) == UNSUPPORTED
    assert bwd2(8, dgm, None) == BAD_ARG and bwd2(8, None, dbt) == BAD_ARG
    pooled = _sentinel(1, 4096, torch.float32, dev)
    wrow = torch.zeros(rows, device=dev)
    rc = lib.clipk_layernorm_meanpool_fwd(x32.data_ptr(), ops._dt(x32), 4096, g.data_ptr(), b.data_ptr(), 1e-5, None, 1, rows,
                                          4096, pooled.data_ptr(), mean.data_ptr(), rstd.data_ptr(), wrow.data_ptr(), ops._stream())
    assert rc == UNSUPPORTED and not ops.meanpool_fused_supported(4096) and ops.meanpool_fused_supported(4092)
    torch.cuda.synchronize()
    for buf, r, cc in ((out32, 0, 0), (out16, 0, 0), (pooled, 0, 0), (dgm.view(1, -1), 0, 0), (dbt.view(1, -1), 0, 0)):
        assert _untouched(buf, r, cc)


# ------------------------------------------------------------------------------------------------ deferred reduce
def test_deferred_parameter_gradients_against_f64(dev):
    """clipk_layernorm_bwd with part_out (dgamma = dbeta = NULL: the partial rows stay in the caller's buffer) +
    clipk_colreduce_batched over widths 4, 516, 2048 and 2052 in ONE launch (blockIdx.y = problem; blocks past a narrow
    problem's 2 cols columns return; narrow kernels and the wide kernel's per-wave partial rows): dgamma0 + dgamma against
    the f64 reference, not only against the immediate form - which stays as the bitwise companion."""
    ops = _ops()
    entries, checks = [], []
    for i, (rows, cols) in enumerate([(9, 4), (5, 516), (9, 2048), (9, 2052)]):
        d, c = _bwd_case(dev, "a", rows, cols, TRIPLES[1], None, seed=150 + 10 * i)
        dg0, db0 = R.randn((cols,), 155 + 10 * i), R.randn((cols,), 156 + 10 * i)
        dgi, dbi = dg0.to(dev), db0.to(dev)
        dxi = _bwd(d, None, dgamma=dgi, dbeta=dbi, accumulate=True)[0]
        blocks, nfloat = ops.layernorm_bwd_partial_shape(rows, cols)
        part = torch.empty(nfloat, device=dev)
        dxp, _, pg, pb = _bwd(d, None, part_out=part)
        assert pg is None and pb is None and _same(dxp, dxi)
        dgd, dbd = dg0.to(dev), db0.to(dev)
        entries.append((part, blocks, cols, dgd, dbd))
        checks.append((c, dg0, db0, dgi, dbi, dgd, dbd))
    ops.colreduce_entries(entries)
    for c, dg0, db0, dgi, dbi, dgd, dbd in checks:
        _, dgr, dbr = R.layernorm_bwd(c["dy"], c["x"], c["gamma"], c["beta"], c["eps"], None, dx_add=c["add"])
        b = R.bounds(c["x"], c["gamma"], c["beta"], c["eps"], None, dy=c["dy"], dx_add=c["add"])
        wg, wb = dg0.to(F64) + dgr, db0.to(F64) + dbr
        _within(dgd, wg, b["dgamma"] + R.U * wg.abs(), "deferred dgamma")      # + the rounding of the final add
        _within(dbd, wb, b["dbeta"] + R.U * wb.abs(), "deferred dbeta")
        assert _same(dgd, dgi) and _same(dbd, dbi)


# ------------------------------------------------------------------------------------------------ second order
@pytest.mark.parametrize("act", [None, "celu", "softplus"])
@pytest.mark.parametrize("cols", [4, 516, 1028, 2048])
def test_second_order_backward_every_register_width(dev, cols, act):
    """ln_bwd2_kernel<2 | 4 | 8> (VPL 8, cols 1028 .. 2048 with 64 KiB of dynamic LDS at 2048, was never launched), rows 1
    and 5 (idle waves; a second block): d_dy, d_a, d_gamma, d_beta within 2e-4 max(1, max|ref|) of f64 autograd over the
    closed-form first backward; the accumulate form adds the same column sums."""
    ops = _ops()
    for rows in (1, 5):
        a, dy, g = R.randn((rows, cols), 160, 1.5, 0.3), R.randn((rows, cols), 161), R.randn((rows, cols), 162)
        gamma, beta = R.params(cols, 163)
        ad, dyd, gd, gmd, btd = (t.to(dev) for t in (a, dy, g, gamma, beta))
        _, _, mean, rstd = ops.layernorm_fwd(ad, gmd, btd, 1e-5, act=act)
        got = ops.layernorm_bwd2(gd, dyd, ad, gmd, btd, mean, rstd, act=act)
        for name, o, ref in zip(("d_dy", "d_a", "d_gamma", "d_beta"), got, R.layernorm_bwd2(g, dy, a, gamma, beta, 1e-5, act)):
            err = float((o.cpu().to(F64) - ref).abs().max())
            assert torch.isfinite(o).all() and err <= R.bwd2_tol(ref), (name, rows, err, R.bwd2_tol(ref))
        dg0, db0 = R.randn((cols,), 164).to(dev), R.randn((cols,), 165).to(dev)
        dga, dba = dg0.clone(), db0.clone()
        ops.layernorm_bwd2(gd, dyd, ad, gmd, btd, mean, rstd, act=act, dgamma=dga, dbeta=dba, accumulate=True)
        assert _same(dga, dg0 + got[2]) and _same(dba, db0 + got[3])


# ------------------------------------------------------------------------------------------------ mean pooling
def _mask(kind, B, L):
    if kind == "none":
        return None
    g = torch.Generator().manual_seed(B * 16 + L)
    m = (torch.rand(B, L, generator=g) < 0.6).to(torch.uint8)
    m[:, 0] = 1
    if kind == "empty":
        m[B // 2] = 0                   # one sample without a valid row
    return m.view(-1)


@pytest.mark.parametrize("xk", ["f32", "bf16"])
@pytest.mark.parametrize("cols", [4, 516, 1028, 4092])
@pytest.mark.parametrize("B,L", [(1, 1), (3, 5), (2, 9)])
def test_meanpool_against_f64(dev, B, L, cols, xk):
    """ln_pool_fwd_kernel<2 | 4 | 8 | 20> and the POOL instantiation of ln_bwd_kernel, f32 and bf16 x, L below, just above and
    twice the four waves of a sample's workgroup, cols up to the last width whose four LDS rows fit 64 KiB; no mask, a
    ragged mask, and one sample without a valid row (pooled == 0, row_weight == 0, dx == 0 on its rows).  pooled,
    row_weight, dx, dgamma, dbeta against the f64 reference - not against layernorm_fwd + pool_fwd, which would share a
    statistics error; mean / rstd bitwise equal to layernorm_fwd's."""
    ops = _ops()
    x, eps = R.family("a", B * L, cols, 170, 1e-5, xk == "bf16")
    gamma, beta = R.params(cols, 171)
    dp = R.randn((B, cols), 172)
    xd, g, b, dpd = _cast(x, xk, dev), gamma.to(dev), beta.to(dev), dp.to(dev)
    _, _, mean0, rstd0 = ops.layernorm_fwd(xd, g, b, eps)
    for kind in ("none", "ragged", "empty"):
        mask = _mask(kind, B, L)
        pooled, mean, rstd, wrow = ops.layernorm_meanpool_fwd(xd, g, b, eps, B, L, None if mask is None else mask.to(dev))
        assert _same(mean, mean0) and _same(rstd, rstd0)
        pr, wr = R.meanpool(x, gamma, beta, eps, B, L, mask)
        bd = R.meanpool_bounds(x, gamma, beta, eps, B, L, mask, dp)
        tag = f"{kind} B={B} L={L} cols={cols} {xk}"
        _within(pooled, pr, bd["pooled"], "pooled " + tag)
        _within(wrow, wr, bd["row_weight"], "row_weight " + tag)
        dx32, dx16, dg, db = ops.layernorm_meanpool_bwd(dpd, wrow, xd, g, mean, rstd, B, L, want_f32=True, want_bf16=True)
        dxr, dgr, dbr = R.meanpool_bwd(dp, x, gamma, beta, eps, B, L, mask)
        _within(dx32, dxr, bd["dx"], "dx " + tag)
        _within(dg, dgr, bd["dgamma"], "dgamma " + tag)
        _within(db, dbr, bd["dbeta"], "dbeta " + tag)
        assert _is_rne(dx16, dx32)
        if kind == "empty":
            rows = slice((B // 2) * L, (B // 2 + 1) * L)
            assert float(pooled[B // 2].abs().max()) == 0.0 and float(wrow[rows].abs().max()) == 0.0
            assert float(dx32[rows].abs().max()) == 0.0
