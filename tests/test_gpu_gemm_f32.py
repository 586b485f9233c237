"""GPU: the exact-f32 GEMM (clipk_gemm_f32: csrc/gemm_f32.hip - gemm_f32_kernel<2, 2> and <4, 1>, gemm_f32_skinny_kernel
<MB = 1 / 2, TB> with its cross-workgroup split and gemm_f32_skinny_reduce_kernel) and its weight gradient
(clipk_gemm_wgrad_f32: wgrad_f32_small_kernel<MT = 1 / 2> and the many-rows branch of the C entry point) against the plain f64
references and the DERIVED bounds of tests/gemm_f32_ref.py (pinned on the CPU by tests/test_gemm_f32_ref_host.py), branch by
branch.  Inputs come from seeded CPU generators with full 24-bit mantissas; references are f64 on the CPU; nothing is masked
out or skipped.  Every call goes through the C entry point on buffers of the test's own: operand rows padded with NaN (no NaN
may reach the output: the pad is never read as data), NaN rows below the operands, the output inside a buffer with sentinel
columns right of N and GUARD sentinel rows below M (bit-unchanged afterwards), the skinny form's workspace followed by a NaN
fence.  A test id states the branch its shapes reach (`_route` restates the dispatch rule of clipk_gemm_f32 and is asserted
against the workspace the library asks for).

Families (a) N(0,1) x N(0,0.05^2), (b) rows scaled by 2^+-6, (d) addend offset 1000 are compared with the bound; family (c),
small integers with power-of-two alpha and addend_scale, EXACTLY, in every branch, summation order and split.

What the code promises exactly is compared bit for bit: two calls; leading dimensions; rows against the same rows of a larger
batch in the same kernel form; <2, 2> against <4, 1> (one k-ordered chain per element, gemm_f32.hip:8-9); the no-workspace
fallback against a forced single split; dW of the one-pass kernel against clipk_gemm_f32(transA, transB), with and without db.

Worst |error| / bound over this file, measured on an MI355X against the f64 reference (a ratio above 1 fails; the file prints
them at the end of a run with -s):
                        tiled <2, 2>   tiled <4, 1>   skinny MB = 1   skinny MB = 2
  product                  0.0484         0.0617         0.0016          0.0015
  with an epilogue         0.9434         0.9919         0.4627          0.5497
                        one-pass kernel   many rows (M > 64)   column reduce (dbias alone)
  dW, db                   0.4909            0.0245               0.8584 (plain and accumulated)
  accumulated              0.9973            0.9171
"product" is the bare product against gamma(K + 24) |A| |B|^T alone: the main loops use a few hundredths of it at the small K of
the tiled cases and about a thousandth at the K >= 256 of the skinny ones (the bound grows with K, a sum of random terms with its
square root).  That is expected, and why family (c) exists: it is exact, so it is what notices a wrong index; the bound is
derived, not fitted, and is not tightened to these figures.  The other rows sit near 1 by construction, not for want of
headroom: where one final rounding dominates (an f32 add of a bias, of an addend offset by 1000 or of a preloaded dW far larger
than the product or of a preloaded db) the bound IS that rounding's half ulp and a correctly rounded result reaches it.
"""
import functools
from types import SimpleNamespace

import pytest
import torch

import gemm_f32_ref as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
BAD_ARG, UNSUPPORTED = -1, -2           # include/clipk.h
GUARD = 8
SENTINEL = -12288.0
NAN = float("nan")
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]
LID = {(False, False): "nt", (False, True): "nn", (True, False): "tt", (True, True): "tn"}     # (trans_a, trans_b) -> BLAS-like name
RATIOS = {}


def _ops():
    from clip_dplm_amd import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    print("\nworst |error| / bound per kernel form: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(RATIOS.items())))


def _route(M, N, K, ta, tb):
    """The kernel form clipk_gemm_f32 picks (skinny_applies, gemm_f32.hip:356-358; the t128 rule, 474-480)."""
    if not ta and M <= 64 and K >= 256 and K % 4 == 0:
        return "skinnyMB1" if M <= 32 else "skinnyMB2"
    return "tiled4x1" if -(-M // 128) * -(-N // 64) >= 1024 else "tiled2x2"


def _within(got, ref, bound, key, what=""):
    got = got.detach().cpu().to(F64)
    assert torch.isfinite(got).all(), what + ": non-finite output"
    err = (got - ref).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max())
    print(f"{what}: worst |err| / bound = {ratio:.4f}")
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio if bool((err <= bound).all()) else max(ratio, 1.0001))
    assert (err <= bound).all(), f"{what}: worst |err| / bound = {ratio:.3f}"


def _exact(got, ref, what):
    got = got.detach().cpu().to(F64)
    assert torch.equal(got, ref), f"{what}: {int((got != ref).sum())} elements differ from the exact reference"


def _same(a, b):
    """Bitwise equality (NaN-safe, -0 != +0)."""
    a, b = a.detach().contiguous().cpu(), b.detach().contiguous().cpu()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ cases and buffers
def _case(fam, M, N, K):
    """CPU inputs of one (family, shape), the f64 product and |a| |b|^T, computed once and shared; device buffers are cached
    on the case.  (The few large cases have a cache of their own, so that the many small ones do not evict them.)"""
    return (_big_case if M * N > 1 << 20 else _small_case)(fam, M, N, K)


def _make_case(fam, M, N, K):
    a, b = R.operands(fam, M, N, K, 100)
    bias, addend, alpha, asc = R.epilogue_operands(fam, M, N, 200)
    return SimpleNamespace(fam=fam, M=M, N=N, K=K, a=a, b=b, bias=bias, addend=addend, alpha=alpha, asc=asc, product=R.product(a, b),
                           dev={})


_big_case = functools.lru_cache(maxsize=5)(_make_case)
_small_case = functools.lru_cache(maxsize=64)(_make_case)


def _padded(t, extra, dev, rows_extra=GUARD):
    """t [r, c] as the leading part of a NaN buffer [r + rows_extra, roundup4(c) + extra] on the device -> (buffer, ld)."""
    r, c = t.shape
    ld = (c + 3) // 4 * 4 + extra
    buf = torch.full((r + rows_extra, ld), NAN, dtype=torch.float32, device=dev)
    buf[:r, :c] = t.to(dev)
    return buf, ld


def _operand(c, which, trans, extra, dev):
    """Stored operand of a case: a [M, K] or, transposed, [K, M]; b [N, K] or [K, N] - in a NaN-padded buffer, made once."""
    key = (which, trans, extra)
    if key not in c.dev:
        t = getattr(c, which)
        c.dev[key] = _padded(t.t() if trans else t, extra, dev)
    return c.dev[key]


def _small(c, name, dev):
    if name not in c.dev:
        v = getattr(c, name)
        c.dev[name] = (torch.tensor([v], dtype=torch.float32) if isinstance(v, float) else v).to(dev)
    return c.dev[name]


# epilogue requests: which operands are present; alias: out IS the addend; wide: ldo = N + 8, ldadd = N + 16
def _epi(alpha=False, bias=False, addend=False, asc=False, alias=False, wide=False):
    return SimpleNamespace(alpha=alpha, bias=bias, addend=addend, asc=asc, alias=alias, wide=wide)


EPIS = {"none": _epi(), "alpha": _epi(alpha=True), "bias": _epi(bias=True), "addend": _epi(addend=True),
        "addend_scaled": _epi(addend=True, asc=True), "all": _epi(True, True, True, True),
        "alias": _epi(True, True, True, True, alias=True), "ld": _epi(True, True, True, True, wide=True)}


def _call(c, ta, tb, epi, dev, extra=0, ws="own", rows=None, expect=0):
    """clipk_gemm_f32 on the first `rows` rows of case c (all of them by default) -> the [rows, N] view of the guarded output.
    extra: additional padding columns of both operands.  ws: "own" (the bytes clipk_gemm_f32_workspace asks for, followed by a
    NaN fence; every byte asked for must be written, nothing behind), "none" (NULL), "small" (4 bytes short)."""
    ops = _ops()
    lib = ops._lib()
    q = EPIS[epi]
    M, N, K = (c.M if rows is None else rows), c.N, c.K
    (abuf, lda), (bbuf, ldb) = _operand(c, "a", ta, extra, dev), _operand(c, "b", tb, extra, dev)
    obuf = torch.full((M + GUARD, N + (8 if q.wide else 0)), SENTINEL, dtype=torch.float32, device=dev)
    out = obuf[:M, :N]
    add, ldadd = None, 0
    if q.addend:
        if q.alias:
            out.copy_(c.addend[:M].to(dev))
            add, ldadd = out, obuf.stride(0)
        else:
            addbuf = torch.full((M + GUARD, N + (16 if q.wide else 0)), NAN, dtype=torch.float32, device=dev)
            addbuf[:M, :N] = c.addend[:M].to(dev)
            add, ldadd = addbuf, addbuf.stride(0)
    need = lib.clipk_gemm_f32_workspace(M, N, K, int(ta), int(tb))
    assert (need > 0) <= _route(M, N, K, ta, tb).startswith("skinny")
    wbuf = torch.full((need // 4 + 4096,), NAN, dtype=torch.float32, device=dev)
    wptr, wbytes = {"own": (wbuf.data_ptr(), need), "none": (None, 0), "small": (wbuf.data_ptr(), max(need - 4, 0))}[ws]
    rc = lib.clipk_gemm_f32(abuf.data_ptr(), lda, int(ta), bbuf.data_ptr(), ldb, int(tb), M, N, K,
                            _small(c, "alpha", dev).data_ptr() if q.alpha else None, _small(c, "bias", dev).data_ptr() if q.bias else None,
                            None if add is None else add.data_ptr(), ldadd, _small(c, "asc", dev).data_ptr() if q.asc else None,
                            out.data_ptr(), obuf.stride(0), wptr, wbytes, ops._stream())
    assert rc == expect, rc
    torch.cuda.synchronize()
    assert bool((obuf[M:] == SENTINEL).all()) and bool((obuf[:M, N:] == SENTINEL).all()), "written outside the output"
    used = need // 4 if ws == "own" else 0
    assert bool(torch.isnan(wbuf[used:]).all()), "written outside the workspace"
    assert not bool(torch.isnan(wbuf[:used]).any()), "the workspace asked for is not the workspace used"
    return out


def _reference(c, epi, rows=None):
    q = EPIS[epi]
    m = c.M if rows is None else rows
    return R.gemm(c.a[:m], c.b, alpha=c.alpha if q.alpha else None, bias=c.bias if q.bias else None,
                  addend=c.addend[:m] if q.addend else None, addend_scale=c.asc if q.asc else None, want_bound=True,
                  product_=(c.product[0][:m], c.product[1][:m]))


def _check(c, ta, tb, epi, dev, **kw):
    """One call against gemm_f32_ref: exactly on family (c), the bound on the others -> the output."""
    out = _call(c, ta, tb, epi, dev, **kw)
    ref, e = _reference(c, epi, kw.get("rows"))
    form = _route(out.shape[0], c.N, c.K, ta, tb)
    what = f"{form} {LID[(ta, tb)]} {epi} ({c.fam}) {out.shape[0]}x{c.N}x{c.K}"
    if c.fam == "c":
        _exact(out, ref, what)
    else:
        _within(out, ref, e, f"{form} {'product' if epi == 'none' else 'epilogue'}", what)
    return out


# ------------------------------------------------------------------------------------------------ tiled <2, 2>
@pytest.mark.parametrize("K", [1, 3, 15, 16, 17, 33, 66])
@pytest.mark.parametrize("ta,tb", LAYOUTS, ids=[LID[l] for l in LAYOUTS])
def test_tiled_2x2_edges(dev, ta, tb, K):
    """gemm_f32_kernel<2, 2> (gemm_f32.hip:94-171), every layout: K = 1, 3 (one partial float4 of the staging, Stager::load
    52-56 / 64-68), 15, 16, 17 (the BK = 16 boundary), 33, 66 (3 and 5 steps: either LDS buffer is the last one read, 122, 146);
    M = 1, 63, 64, 65 and N = 1, 31, 33, 64, 65 (ragged and whole tiles, a second tile with one row / column, the `wn` halves
    with and without live columns: 158-159).  Bare product and the full epilogue, families (a) and (c); (b) and (d) at the
    two-tile shapes."""
    for M in (1, 63, 64, 65):
        for N in (1, 31, 33, 64, 65):
            assert _route(M, N, K, ta, tb) == "tiled2x2"
            for fam in ("a", "c") + (("b", "d") if (M, N) in ((65, 65), (63, 33)) else ()):
                c = _case(fam, M, N, K)
                _check(c, ta, tb, "none", dev)
                _check(c, ta, tb, "all", dev)


# ------------------------------------------------------------------------------------------------ tiled <4, 1>
TALL, SQUARE, BELOW = (130945, 37, 18), (4091, 2045, 18), (130944, 37, 18)


@pytest.mark.parametrize("shape", [TALL, SQUARE], ids=["tiled4x1-tall-1024x1", "tiled4x1-square-32x32"])
@pytest.mark.parametrize("ta,tb", LAYOUTS, ids=[LID[l] for l in LAYOUTS])
def test_tiled_4x1(dev, ta, tb, shape):
    """gemm_f32_kernel<4, 1> (t128 >= 1024, gemm_f32.hip:475-478): Stager<128> with two float4 per thread (40, 45), `wm` = the
    wave, both 32-column tiles per wave (NT = 2).  Tall: 1023 * 128 + 1 rows - 1024 row tiles, the last with one row.
    Square-ish: 32 x 32 tiles with a ragged last row (123 rows) and column (61 columns: the second 32-column tile has 29 live
    columns) - the tm / tn decomposition of blockIdx.x (102-104).  Exact on family (c), the bound on (a)."""
    assert _route(*shape, ta, tb) == "tiled4x1"
    _check(_case("c", *shape), ta, tb, "all", dev)
    _check(_case("a", *shape), ta, tb, "none", dev)


@pytest.mark.parametrize("ta,tb", LAYOUTS, ids=[LID[l] for l in LAYOUTS])
def test_tile_threshold_and_equal_bits_of_the_two_tiles(dev, ta, tb):
    """t128 = 1023 (M = 1023 * 128, N = 37) runs <2, 2>, one row more runs <4, 1> (gemm_f32.hip:477): both right, and the rows
    they share bit-identical - each element is one chain of fmaf over k in steps of the instruction's K = 2, whichever tile
    computes it (8-9; the fragment k map is the same in both: 128-144)."""
    assert _route(*BELOW, ta, tb) == "tiled2x2" and _route(*TALL, ta, tb) == "tiled4x1"
    c = _case("a", *TALL)
    tall = _check(c, ta, tb, "all", dev)
    below = _check(c, ta, tb, "all", dev, rows=BELOW[0])          # (the first M - 1 rows / stored columns of the same buffers)
    assert _same(tall[:BELOW[0]], below)
    _check(_case("c", *TALL), ta, tb, "all", dev, rows=BELOW[0])


# ------------------------------------------------------------------------------------------------ skinny
SK_N = [1, 31, 32, 33, 520]
SK_K = [256, 260, 272, 1284]


def _expected_ws(M, N, K, S):
    """Bytes a FORCED split asks for (skinny_splits 339-341, skinny_ws_bytes 351-355)."""
    mb = 1 if M <= 32 else 2
    nunit = -(-K // (32 if mb == 1 else 16))
    s = S if nunit // S >= 1 else 1
    return 0 if s <= 1 else s * -(-N // 32) * mb * 1024 * 4


@pytest.mark.parametrize("S", range(9), ids=lambda s: "Sauto" if s == 0 else f"S{s}")
@pytest.mark.parametrize("tb", [False, True], ids=["nt", "nn"])
@pytest.mark.parametrize("M", [1, 17, 32, 33, 64], ids=lambda m: f"skinnyMB{1 if m <= 32 else 2}-M{m}")
def test_skinny_every_split(dev, kopt, M, tb, S):
    """gemm_f32_skinny_kernel<MB, TB> + gemm_f32_skinny_reduce_kernel<MB> with option gemm_f32_splits = 0 (the auto rule) and
    forced 1 .. 8: N = 1, 31, 32, 33, 520 (one ragged column block, whole, a second with one column, 17 blocks), K = 256 (8 units
    of 32 at MB = 1: fewer than the 16 waves; 16 units of 16 at MB = 2), 260 (a partial unit), 272, 1284 (41 / 81 units: an odd
    run, the `uok` half idle on the last trip, gemm_f32.hip:226-228).  Forced splits that do not divide the unit count leave
    trailing workgroups with an empty run (MB = 1, K = 256, S = 5: g0 = 8 >= nunit, 203-206: their partial tile must be written
    as zeros); S = 8 at K = 256 is one unit per workgroup.  The workspace is the test's own: the bytes asked for are the bytes
    written.  Exact on family (c) whatever the split; the bound on (a)."""
    kopt("gemm_f32_splits", S)
    lib = _ops()._lib()
    for N in SK_N:
        for K in SK_K:
            assert _route(M, N, K, False, tb) == f"skinnyMB{1 if M <= 32 else 2}"
            need = lib.clipk_gemm_f32_workspace(M, N, K, 0, int(tb))
            if S:
                assert need == _expected_ws(M, N, K, S), (N, K, need)
            else:
                assert need % (-(-N // 32) * (1 if M <= 32 else 2) * 4096) == 0 and need // (-(-N // 32) * (1 if M <= 32 else 2) * 4096) <= 8
            for fam in ("c", "a"):
                _check(_case(fam, M, N, K), False, tb, "all", dev)


@pytest.mark.parametrize("ws", ["none", "small"])
@pytest.mark.parametrize("tb", [False, True], ids=["nt", "nn"])
@pytest.mark.parametrize("M", [17, 64], ids=["skinnyMB1-M17", "skinnyMB2-M64"])
def test_skinny_without_a_workspace(dev, kopt, M, tb, ws):
    """clipk_gemm_f32 without a workspace, or with one 4 bytes short (gemm_f32.hip:466-470): one workgroup per column block
    (S = 1), nothing parked anywhere - right, and the bits of a forced single split."""
    N, K = 520, 1284
    kopt("gemm_f32_splits", 4)
    assert _ops()._lib().clipk_gemm_f32_workspace(M, N, K, 0, int(tb)) == _expected_ws(M, N, K, 4) > 0
    got = {fam: _check(_case(fam, M, N, K), False, tb, "all", dev, ws=ws) for fam in ("c", "a", "d")}
    split = _check(_case("a", M, N, K), False, tb, "all", dev)
    kopt("gemm_f32_splits", 1)
    single = _check(_case("a", M, N, K), False, tb, "all", dev)
    assert _same(got["a"], single)
    assert not _same(split, single)          # (the forced 4-way split did run: another summation order)


@pytest.mark.parametrize("M,N,K,ta", [(65, 33, 256, False), (17, 33, 252, False), (17, 33, 258, False), (17, 33, 256, True),
                                      (64, 33, 255, False)],
                         ids=["tiled2x2-M65", "tiled2x2-K252", "tiled2x2-K258", "tiled2x2-transA", "tiled2x2-K255"])
@pytest.mark.parametrize("tb", [False, True], ids=["b_nk", "b_kn"])
def test_neighbours_of_the_skinny_form_go_tiled(dev, M, N, K, ta, tb):
    """skinny_applies (gemm_f32.hip:356-358): M = 65, K = 252 (< 256), K = 258 (% 4), a transposed A stay on the tiled kernel
    (no workspace asked for) and are right."""
    assert _route(M, N, K, ta, tb) == "tiled2x2"
    assert _ops()._lib().clipk_gemm_f32_workspace(M, N, K, int(ta), int(tb)) == 0
    for fam in ("c", "a"):
        _check(_case(fam, M, N, K), ta, tb, "all", dev)


# ------------------------------------------------------------------------------------------------ every form
# (M, N, K, layouts, forced split) of one representative per form
# (tiled4x1: 1024 row tiles of 3 columns - the smallest output that reaches the kernel)
FORMS = {"tiled2x2": (65, 65, 33, LAYOUTS, 0), "tiled4x1": (130945, 3, 5, LAYOUTS, 0), "skinnyMB1-S1": (17, 33, 260, LAYOUTS[:2], 1),
         "skinnyMB1-S3": (32, 520, 1284, LAYOUTS[:2], 3), "skinnyMB2-S1": (40, 33, 272, LAYOUTS[:2], 1),
         "skinnyMB2-S4": (64, 65, 1284, LAYOUTS[:2], 4)}


@pytest.mark.parametrize("form", list(FORMS))
def test_every_epilogue_in_every_form(dev, kopt, form):
    """The epilogue of each kernel (tiled: gemm_f32.hip:153-170; skinny single split: 290-299; reduce: 317-329): none, alpha,
    bias, addend, addend with addend_scale, all together, out aliasing the addend (each element read and written by one
    thread), ldo = N + 8 with ldadd = N + 16.  Every family; each call twice: same bits."""
    M, N, K, layouts, S = FORMS[form]
    kopt("gemm_f32_splits", S)
    for ta, tb in layouts:
        assert form.startswith(_route(M, N, K, ta, tb))
        for fam in R.FAMILIES:
            c = _case(fam, M, N, K)
            for epi in EPIS:
                out = _check(c, ta, tb, epi, dev)
                if epi in ("none", "all", "alias") and fam == "a":
                    assert _same(out, _call(c, ta, tb, epi, dev)), (form, epi, "not reproducible")


@pytest.mark.parametrize("form", list(FORMS))
def test_leading_dimensions_do_not_change_bits(dev, kopt, form):
    """lda, ldb 8 floats wider (NaN in every pad column and in the rows below the operands, as in every call of this file): the
    same bits, and no NaN in the output - Stager::load reads k < K and rows < nrows only (gemm_f32.hip:50-69), the skinny
    kernel masks clamped loads with bit masks (225, 252-255)."""
    M, N, K, layouts, S = FORMS[form]
    kopt("gemm_f32_splits", S)
    c = _case("a", M, N, K)
    for ta, tb in layouts:
        dense, wide = _call(c, ta, tb, "ld", dev), _call(c, ta, tb, "ld", dev, extra=8)
        assert torch.isfinite(wide).all() and _same(dense, wide), (form, ta, tb)


@pytest.mark.parametrize("form,rows", [("tiled2x2", 64), ("tiled2x2", 1), ("skinnyMB1-S1", 1), ("skinnyMB1-S3", 17), ("skinnyMB2-S1", 33),
                                       ("skinnyMB2-S4", 33), ("tiled4x1-square", 4000)])
def test_rows_do_not_depend_on_the_batch(dev, kopt, form, rows):
    """Family (b): the first m rows of the M-row call == the call on those m rows, bit for bit, both routed to the same kernel
    form: an element is a chain over k of its own row and column (MFMA lanes do not mix rows), tails are zero-filled
    (Stager::load) or masked (skinny: mok, 216-218, 255), only stores are predicated."""
    M, N, K, layouts, S = (SQUARE + (LAYOUTS, 0)) if form == "tiled4x1-square" else FORMS[form]
    kopt("gemm_f32_splits", S)
    c = _case("b", M, N, K)
    for ta, tb in layouts:
        assert _route(rows, N, K, ta, tb) == _route(M, N, K, ta, tb)
        full, part = _call(c, ta, tb, "all", dev), _call(c, ta, tb, "all", dev, rows=rows)
        assert _same(full[:rows], part), (form, ta, tb)
    _check(c, *layouts[-1], "all", dev)


@pytest.mark.parametrize("M,N,K", [(65, 65, 33), (17, 33, 260)], ids=["tiled2x2", "skinnyMB1"])
def test_refusals(dev, M, N, K):
    """clipk_gemm_f32's checks (gemm_f32.hip:456-457) return before any launch: a leading dimension that is no multiple of 4
    and a base pointer off a 16-byte boundary are UNSUPPORTED (float4 staging), a missing operand or an empty shape BAD_ARG; the
    output keeps its bits."""
    ops = _ops()
    lib = ops._lib()
    ld = (K + 3) // 4 * 4 + 4
    a = torch.zeros(M + 1, ld + 2, device=dev)
    b = torch.zeros(N + 1, ld + 2, device=dev)
    obuf = torch.full((M + GUARD, N), SENTINEL, device=dev)

    def refused(code, A=a, lda=ld, B=b, ldb=ld, m=M, out=obuf):
        rc = lib.clipk_gemm_f32(None if A is None else A.data_ptr(), lda, 0, B.data_ptr(), ldb, 0, m, N, K, None, None, None, 0, None,
                                None if out is None else out.data_ptr(), N, None, 0, ops._stream())
        assert rc == code, rc
        torch.cuda.synchronize()
        assert bool((obuf == SENTINEL).all())

    refused(UNSUPPORTED, lda=ld + 1)
    refused(UNSUPPORTED, ldb=ld + 1)
    refused(UNSUPPORTED, lda=ld + 2)
    refused(UNSUPPORTED, ldb=ld + 2)
    refused(UNSUPPORTED, A=a.view(-1)[1:])
    refused(UNSUPPORTED, B=b.view(-1)[2:])
    refused(BAD_ARG, A=None)
    refused(BAD_ARG, out=None)
    refused(BAD_ARG, m=0)
    ok = torch.full((M, N), SENTINEL, device=dev)                         # the same buffers with nothing wrong are accepted
    assert lib.clipk_gemm_f32(a.data_ptr(), ld, 0, b.data_ptr(), ld, 0, M, N, K, None, None, None, 0, None, ok.data_ptr(), N, None, 0,
                              ops._stream()) == 0
    torch.cuda.synchronize()
    assert bool((ok == 0).all())


# ------------------------------------------------------------------------------------------------ weight gradient
@functools.lru_cache(maxsize=8)
def _wcase(fam, M, N, K):
    dy, x = R.wgrad_operands(fam, M, N, K, 400)
    pre_w = R.randint((N, K), 500, -3, 3) if fam == "c" else R.randn((N, K), 500)
    pre_b = R.randint((N,), 501, -3, 3) if fam == "c" else R.randn((N,), 501)
    return SimpleNamespace(fam=fam, M=M, N=N, K=K, dy=dy, x=x, pre_w=pre_w, pre_b=pre_b, plain=R.wgrad(dy, x, want_bound=True),
                           acc=R.wgrad(dy, x, pre_w=pre_w, pre_b=pre_b, want_bound=True))


def _wgrad_raw(dyb, lddy, xb, ldx, dwv, lddw, dbv, M, N, K, acc):
    ops = _ops()
    rc = ops._lib().clipk_gemm_wgrad_f32(dyb.data_ptr(), lddy, xb.data_ptr(), ldx, None if dwv is None else dwv.data_ptr(), lddw,
                                         None if dbv is None else dbv.data_ptr(), M, N, K, int(acc), ops._stream())
    torch.cuda.synchronize()
    return rc


def _wgrad(c, dev, acc=False, want_w=True, want_b=True, extra=(4, 8, 12), dense_dy=False, expect=0):
    """clipk_gemm_wgrad_f32 on NaN-padded dY / X and a guarded dW [N + GUARD, K + extra] / db [N + GUARD] -> (dW, db) views."""
    M, N, K = c.M, c.N, c.K
    dyb, lddy = (c.dy.to(dev).contiguous(), N) if dense_dy else _padded(c.dy, extra[0], dev)
    xb, ldx = _padded(c.x, extra[1], dev)
    wbuf = torch.full((N + GUARD, K + extra[2]), SENTINEL, dtype=torch.float32, device=dev)
    bbuf = torch.full((N + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    if acc:
        wbuf[:N, :K], bbuf[:N] = c.pre_w.to(dev), c.pre_b.to(dev)
    before_w, before_b = wbuf.clone(), bbuf.clone()
    rc = _wgrad_raw(dyb, lddy, xb, ldx, wbuf if want_w else None, wbuf.stride(0), bbuf if want_b else None, M, N, K, acc)
    assert rc == expect, rc
    assert bool((wbuf[N:] == SENTINEL).all()) and bool((wbuf[:N, K:] == SENTINEL).all()) and bool((bbuf[N:] == SENTINEL).all())
    if not want_w or expect:
        assert _same(wbuf, before_w)
    if not want_b or expect:
        assert _same(bbuf, before_b)
    return wbuf[:N, :K], bbuf[:N], (dyb, lddy, xb, ldx)


def _wverify(c, dw, db, acc, key, what):
    rw, rb, e_w, e_b = c.acc if acc else c.plain
    if c.fam == "c":
        if dw is not None:
            _exact(dw, rw, what + " dW")
        if db is not None:
            _exact(db, rb, what + " db")
    else:
        if dw is not None:
            _within(dw, rw, e_w, key, what + " dW")
        if db is not None:
            _within(db, rb, e_b, key, what + " db")


def _gemm_tn(bufs, M, N, K, dev, addend=None):
    """clipk_gemm_f32(transA, transB) on the weight gradient's own buffers: dW[N, K] = dY^T X (+ addend)."""
    ops = _ops()
    dyb, lddy, xb, ldx = bufs
    out = torch.empty(N, K, device=dev)
    rc = ops._lib().clipk_gemm_f32(dyb.data_ptr(), lddy, 1, xb.data_ptr(), ldx, 1, N, K, M, None, None,
                                   None if addend is None else addend.data_ptr(), 0 if addend is None else addend.stride(0), None,
                                   out.data_ptr(), K, None, 0, ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("K", [1, 31, 127, 128, 129, 161])
@pytest.mark.parametrize("M", [1, 31, 32, 33, 64], ids=lambda m: f"onepassMT{1 if m <= 32 else 2}-M{m}")
def test_wgrad_one_pass_kernel(dev, M, K):
    """wgrad_f32_small_kernel<MT> (gemm_f32.hip:391-443): M = 1, 31, 32 (MT = 1), 33, 64 (MT = 2); N = 1, 31, 33, 65 (ragged row
    blocks; db comes from the waves of column block 0, 439-442); K = 1, 31 (one wave, three returning early, 396), 127, 128, 129
    (a second workgroup with one column), 161 (a partial second wave).  Strided lddy / ldx / lddw and dense; overwrite and
    accumulate; dbias = NULL (dW bit-identical); dW = NULL with dbias alone (the column reduce); dW bit-identical to
    clipk_gemm_f32(transA, transB) on the same buffers (same contraction order: 383-384), accumulation included."""
    for N in (1, 31, 33, 65):
        for fam in ("c", "a", "b"):
            c = _wcase(fam, M, N, K)
            what = f"one-pass ({fam}) {M}x{N}x{K}"
            dw, db, bufs = _wgrad(c, dev)
            _wverify(c, dw, db, False, "wgrad one-pass", what)
            assert torch.equal(dw, _gemm_tn(bufs, M, N, K, dev)), what + ": dW differs from clipk_gemm_f32(transA, transB)"
            dw0, _, _ = _wgrad(c, dev, want_b=False)
            assert _same(dw0, dw), what + ": dW depends on dbias"
            dwd, dbd, _ = _wgrad(c, dev, extra=(0, 0, 0))
            assert _same(dwd, dw) and _same(dbd, db), what + ": leading dimensions change bits"
            dw2, db2, _ = _wgrad(c, dev)
            assert _same(dw2, dw) and _same(db2, db), what + ": not reproducible"
            _, db1, _ = _wgrad(c, dev, want_w=False, dense_dy=True)
            _wverify(c, None, db1, False, "wgrad column reduce", what + " dbias alone")
            aw, ab, bufs = _wgrad(c, dev, acc=True)
            _wverify(c, aw, ab, True, "wgrad one-pass accumulated", what + " accumulated")
            assert torch.equal(aw, _gemm_tn(bufs, M, N, K, dev, addend=c.pre_w.to(dev)))
            _, ab1, _ = _wgrad(c, dev, acc=True, want_w=False, dense_dy=True)
            _wverify(c, None, ab1, True, "wgrad column reduce", what + " dbias alone accumulated")


@pytest.mark.parametrize("N,K", [(36, 33), (64, 70)])
@pytest.mark.parametrize("M", [65, 100], ids=lambda m: f"manyrows-M{m}")
def test_wgrad_many_rows_branch_of_the_entry_point(dev, M, N, K):
    """M > 64 inside clipk_gemm_wgrad_f32 (gemm_f32.hip:503-513; ops.gemm_wgrad_f32 takes this case itself and never gets here):
    dW through clipk_gemm_f32(transA, transB) with dW as its own addend when accumulating, db through the column reduce (dense
    dY rows: lddy = N).  Exact on (c), the bound on (a) and (b); dW bit-identical to the direct call and without dbias."""
    for fam in ("c", "a", "b"):
        c = _wcase(fam, M, N, K)
        what = f"many rows ({fam}) {M}x{N}x{K}"
        for acc in (False, True):
            dw, db, bufs = _wgrad(c, dev, acc=acc, dense_dy=True)
            _wverify(c, dw, db, acc, "wgrad many rows" + (" accumulated" if acc else ""), what)
            assert _same(dw, _gemm_tn(bufs, M, N, K, dev, addend=c.pre_w.to(dev) if acc else None)), what
            dw0, _, _ = _wgrad(c, dev, acc=acc, want_b=False)                 # strided dY is fine without dbias
            assert _same(dw0, dw), what + ": dW depends on dbias / lddy"
            _, db1, _ = _wgrad(c, dev, acc=acc, want_w=False, dense_dy=True)
            assert _same(db1, db)


@pytest.mark.parametrize("M", [33, 65, 100])
def test_wgrad_refuses_strided_dy_with_dbias_before_touching_dw(dev, M):
    """The column reduce takes dense rows: dbias != NULL with lddy != N is UNSUPPORTED in the many-rows branch (M > 64, or no dW
    at all) - and it is refused BEFORE the product is launched: dW and dbias keep their bits (the entry point used to write dW
    first and refuse afterwards; gemm_f32.hip:503-506).  M = 33 with a dW runs the one-pass kernel, which takes any lddy."""
    for acc in (False, True):
        c = _wcase("a", M, 36, 33)
        if M > 64:
            _wgrad(c, dev, acc=acc, expect=UNSUPPORTED)
        else:
            _wgrad(c, dev, acc=acc)
        _wgrad(c, dev, acc=acc, want_w=False, expect=UNSUPPORTED)
    z = torch.zeros(64, device=dev)
    assert _wgrad_raw(z, 4, z, 4, None, 4, None, 4, 4, 4, 0) == BAD_ARG
    assert _wgrad_raw(z, 4, z, 4, z, 4, z, 0, 4, 4, 0) == BAD_ARG
