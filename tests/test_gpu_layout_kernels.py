"""GPU: the layout kernels - transpose_scale_kernel (csrc/celogits.hip), cast_transpose_kernel / cast_transpose_batched_kernel
and pool_varlen_fwd_kernel / pool_varlen_bwd_kernel (csrc/elementwise.hip), rope_qk_kernel<D> (csrc/attention.hip) - through
their C entry points, at the sizes where their tiles, loops and instantiations change.  Every reference is computed on the CPU
by torch or by a few lines of f64 here (RoPE: the tables and the rotate-half convention of tests/attention_ref.py; bf16
rounding: tests/elementwise_ref.py); none is taken from another kernel.  Outputs live in buffers of the test's own between two
fences of a bit pattern no kernel writes; after every call the fences, the row pads and the outputs of refused calls still
hold it.

What is a copy or ONE rounding is compared bit for bit: the transpose with and without a scale, both bf16 copies of
cast_transpose under every interleave, position-0 pooling and its backward, the v third of a rotated qkv.  What sums or rounds
twice has a bound derived from the number formats, stated at the test: the mean pooling (rtol 1e-5 / atol 1e-6, the bound of
test_gpu_elementwise's pool_fwd test), its backward (two f32 roundings), RoPE (one multiply-add pair in f32, then one bf16
rounding).

Measured on an MI355X (the file prints these at the end of a run with -s):
  transpose_scale              2 236 189 elements, all bits equal (2 097 121 of them past grid y)
  cast_transpose               2 251 956 elements, all bits equal;  batched: 328 712
  pool_varlen, first row       56 sequences x d, all bits equal;  past grid y: 1 572 864 elements, all bits equal
  pool_varlen, mean            49 sequences x d, worst deviation / bound 0.038
  pool_varlen, mean backward   35 sequences x d, worst deviation / bound 0.847 (two roundings against a two-rounding bound)
  rope_qk D = 16 .. 128        133 056 elements inside the rounding interval; under 0.05 % are not the bf16 rounding of the f64 value itself
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_ref as A  # noqa: E402
import elementwise_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
BAD_ARG, UNSUPPORTED = -1, -2           # include/clipk.h
GUARD = 16                              # elements of each fence
PAT32, PAT16 = 0x7fc00abc, 0x5a5a       # fence patterns (f32: a NaN no kernel produces)
_STATS = {}                             # group -> [comparisons, worst deviation / bound]


def _ops():
    from clip_dplm_amd import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\ncomparisons and worst deviation / bound per group (bitwise groups: 0):")
    for key in sorted(_STATS):
        print(f"  {key:28s} {_STATS[key][0]:6d}  {_STATS[key][1]:.3f}")


def _note(group, ratio=0.0, n=1):
    s = _STATS.setdefault(group, [0, 0.0])
    s[0] += n
    s[1] = max(s[1], float(ratio))


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


class _Fenced:
    """n elements of int32 (f32) or int16 (bf16) between two fences, every element the pattern to begin with."""
    def __init__(self, n, dev, bits=32):
        self.n, self.bits = n, bits
        self.pat = PAT32 if bits == 32 else PAT16
        self.buf = torch.full((n + 2 * GUARD,), self.pat, dtype=torch.int32 if bits == 32 else torch.int16, device=dev)
        self.ptr = self.buf.data_ptr() + GUARD * (bits // 8)

    def fill(self, values):
        """values: a CPU tensor of n elements of the same width, copied in bit for bit."""
        self.buf[GUARD:GUARD + self.n] = values.contiguous().view(self.buf.dtype).view(-1).to(self.buf.device)
        return self

    def read(self):
        """The n elements as a CPU integer tensor."""
        return self.buf.cpu()[GUARD:GUARD + self.n].clone()

    def f32(self):
        return self.read().view(torch.float32)

    def untouched_outside(self, written=None):
        got = self.buf.cpu()
        keep = torch.ones(self.n + 2 * GUARD, dtype=torch.bool)
        if written is not None:
            keep[GUARD:GUARD + self.n] = ~written.view(-1)
        return bool((got[keep] == self.pat).all())


def _bits32(x):
    return x.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ transpose_scale
SPECIALS32 = np.array([0x80000000, 0x7f800000, 0xff800000, 0x7fc00123, 0xffc54321, 0x00000001, 0x807fffff], dtype=np.uint32)


def _transpose_input(Rr, C, seed):
    x = _randn((Rr, C), seed, 3.0)
    k = min(len(SPECIALS32), Rr * C - 1) if Rr * C > 1 else 0
    x.view(-1)[Rr * C - k:] = R.f32_from_bits(SPECIALS32[:k])          # -0, +-inf, two NaN payloads, subnormals
    return x


def _transpose(x, scale, dev):
    ops = _ops()
    Rr, C = x.shape
    out = _Fenced(Rr * C, dev)
    xd = x.to(dev)
    sd = None if scale is None else torch.tensor([scale], dtype=torch.float32, device=dev)
    rc = ops._lib().clipk_transpose_scale_f32(xd.data_ptr(), Rr, C, ops.ptr(sd), out.ptr, ops._stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("Rr,C", [(r, c) for r in (1, 31, 32, 33, 65) for c in (1, 31, 32, 33, 65)] + [(333, 130)])
def test_transpose_scale(dev, Rr, C):
    """transpose_scale_kernel: below, at and past the 32 x 32 tile on both axes.  No scale: x^T bit for bit, -0.0, +-inf,
    quiet NaN payloads and subnormals included (1.0f * x).  With a device scale: ONE f32 product, the bits of torch's own
    f32 multiply on the CPU (NaN stays NaN).  Nothing written outside out[C, R]."""
    x = _transpose_input(Rr, C, 10 + Rr * 7 + C)
    rc, out = _transpose(x, None, dev)
    assert rc == 0 and out.untouched_outside(torch.ones(Rr * C, dtype=torch.bool))
    assert torch.equal(out.read().view(C, Rr), _bits32(x.t().contiguous())), "x^T: not the same bits"
    s = 0.37
    rc, out = _transpose(x, s, dev)
    assert rc == 0 and out.untouched_outside(torch.ones(Rr * C, dtype=torch.bool))
    want = (x.t() * torch.tensor(s, dtype=torch.float32)).contiguous()
    got = out.f32().view(C, Rr)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(_bits32(got)[~nan], _bits32(want)[~nan]), "s x^T: not one f32 rounding"
    _note("transpose_scale", n=2 * Rr * C)


def test_transpose_scale_more_row_tiles_than_grid_y(dev):
    """2 097 121 x 1: 65 536 row tiles, one more than grid y holds; the kernel walks them with a grid-stride loop (before: a
    launch error).  x^T bit for bit, the last row included."""
    Rr = 2097121
    x = _randn((Rr, 1), 11)
    rc, out = _transpose(x, None, dev)
    assert rc == 0 and out.untouched_outside(torch.ones(Rr, dtype=torch.bool))
    assert torch.equal(out.read(), _bits32(x).view(-1))
    _note("transpose_scale", n=Rr)


def test_transpose_scale_refusals(dev):
    ops = _ops()
    lib, st = ops._lib(), ops._stream()
    x = torch.zeros(4, 4, device=dev)
    out = _Fenced(16, dev)
    assert lib.clipk_transpose_scale_f32(None, 4, 4, None, out.ptr, st) == BAD_ARG
    assert lib.clipk_transpose_scale_f32(x.data_ptr(), 4, 4, None, None, st) == BAD_ARG
    assert lib.clipk_transpose_scale_f32(x.data_ptr(), 0, 4, None, out.ptr, st) == BAD_ARG
    assert lib.clipk_transpose_scale_f32(x.data_ptr(), 4, -1, None, out.ptr, st) == BAD_ARG
    torch.cuda.synchronize()
    assert out.untouched_outside()


# ------------------------------------------------------------------------------------------------ cast_transpose
def _il_src(rows, hd, il_rows):
    """include/clipk.h: copy row 2 j (+ 1) of a head of hd rows holds W row j (+ hd / 2) of that head, rows < il_rows."""
    r = torch.arange(rows)
    if il_rows == 0:
        return r
    d = r % hd
    return torch.where(r < il_rows, (r - d) + d // 2 + (d % 2) * (hd // 2), r)


def _il_cases(rows):
    """none; il_hd 2 / 16 / 24 below `rows`; il_rows = rows; il_rows no multiple of 64 (a tile straddles the boundary)."""
    cand = [(0, 0), (2, rows - rows % 2), (2, 66), (16, 48), (16, 96), (16, rows if rows % 16 == 0 else 0), (24, 48), (24, 120)]
    return sorted({(hd, n) for hd, n in cand if n == 0 and hd == 0 or 0 < n <= rows})


def _weight(rows, cols, seed):
    w = _randn((rows, cols), seed, 2.0)
    tab = R.f32_from_bits(R.CAST_TABLE)                                  # ties, carry, overflow to inf, NaN, subnormals
    k = min(tab.numel(), rows * cols)
    idx = (torch.arange(k) * 7919) % (rows * cols) if rows * cols > k else torch.arange(k)
    w.view(-1)[idx] = tab[:k]
    return w


def _same_bf16(got_bits, want):
    """got: int16 bits [..]; want: bf16 tensor.  Equal bits; a NaN only has to be a NaN (elementwise_ref.bf16_rne_bits)."""
    g = got_bits.numpy().view(np.uint16).reshape(-1)
    w = R.bf16_bits(want).reshape(-1)
    nan = (w & 0x7fff) > 0x7f80
    return bool(np.array_equal(g[~nan], w[~nan])) and bool(((g[nan] & 0x7fff) > 0x7f80).all())


def _cast_reference(w, il):
    src = _il_src(w.shape[0], *il)
    wb = w[src].to(torch.bfloat16)
    return wb, wb.t().contiguous()


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 130])
def test_cast_transpose(dev, rows):
    """cast_transpose_kernel: rows and cols below, at and past the 64 x 64 tile; wb only, wt only, both; every interleave
    of _il_cases.  Both copies equal w[il source rows].to(bfloat16) - torch's CPU cast - and its transpose in bits, on
    the rounding table of elementwise_ref (ties, carry, overflow, NaN, subnormals) scattered over the matrix."""
    ops = _ops()
    lib, st = ops._lib(), ops._stream()
    for cols in (1, 63, 64, 65, 130):
        w = _weight(rows, cols, 20 + rows + 3 * cols)
        wd = w.to(dev)
        for il in _il_cases(rows):
            want_b, want_t = _cast_reference(w, il)
            for use_b, use_t in ((True, False), (False, True), (True, True)):
                ob, ot = _Fenced(rows * cols, dev, 16), _Fenced(rows * cols, dev, 16)
                rc = lib.clipk_cast_transpose(wd.data_ptr(), ob.ptr if use_b else None, ot.ptr if use_t else None, rows, cols,
                                              il[0], il[1], st)
                torch.cuda.synchronize()
                assert rc == 0, (rows, cols, il, rc)
                every = torch.ones(rows * cols, dtype=torch.bool)
                assert ob.untouched_outside(every if use_b else None) and ot.untouched_outside(every if use_t else None)
                if use_b:
                    assert _same_bf16(ob.read(), want_b), (rows, cols, il, "w_bf16")
                if use_t:
                    assert _same_bf16(ot.read(), want_t), (rows, cols, il, "wt_bf16")
                _note("cast_transpose", n=rows * cols * (use_b + use_t))


def test_cast_transpose_batched(dev):
    """cast_transpose_batched_kernel (32 blocks per tensor, striding over its tiles): n = 1; 65 x 1089 = 36 tiles, the second
    trip of the block-stride loop; tensors with fewer tiles than blocks; interleaved heads with a tile across il_rows; a
    descriptor without w_bf16 and one without wt_bf16.  Each copy against torch's CPU cast, never against the other kernel."""
    ops = _ops()
    specs = [((65, 1089), (0, 0), True, True), ((130, 65), (16, 96), True, True), ((1, 1), (0, 0), True, True),
             ((63, 130), (2, 62), False, True), ((192, 64), (24, 120), True, False), ((64, 64), (16, 64), True, True)]
    for group in ([specs[0]], specs):
        ws = [_weight(*sh, 30 + i) for i, (sh, _, _, _) in enumerate(group)]
        wds = [w.to(dev) for w in ws]
        outs = [(_Fenced(w.numel(), dev, 16), _Fenced(w.numel(), dev, 16)) for w in ws]
        desc = torch.tensor([(wd.data_ptr(), ob.ptr if ub else 0, ot.ptr if ut else 0, w.shape[0], w.shape[1], il[0] or 2, il[1])
                             for w, wd, (ob, ot), (_, il, ub, ut) in zip(ws, wds, outs, group)], dtype=torch.int64).to(dev)
        rc = ops._lib().clipk_cast_transpose_batched(desc.data_ptr(), len(group), ops._stream())
        torch.cuda.synchronize()
        assert rc == 0
        for w, (ob, ot), (sh, il, ub, ut) in zip(ws, outs, group):
            want_b, want_t = _cast_reference(w, il)
            every = torch.ones(w.numel(), dtype=torch.bool)
            assert ob.untouched_outside(every if ub else None) and ot.untouched_outside(every if ut else None), sh
            assert not ub or _same_bf16(ob.read(), want_b), (sh, il, "w_bf16")
            assert not ut or _same_bf16(ot.read(), want_t), (sh, il, "wt_bf16")
            _note("cast_transpose_batched", n=w.numel() * (ub + ut))


def test_cast_transpose_refusals(dev):
    """Odd il_hd, il_rows no multiple of il_hd, il_rows > rows, both outputs NULL, NULL w, bad dims: BAD_ARG; more row tiles
    than grid y holds: UNSUPPORTED.  Nothing written."""
    ops = _ops()
    lib, st = ops._lib(), ops._stream()
    rows, cols = 48, 8
    w = torch.zeros(rows, cols, device=dev)
    ob, ot = _Fenced(rows * cols, dev, 16), _Fenced(rows * cols, dev, 16)
    p = w.data_ptr()
    for args in ((p, ob.ptr, ot.ptr, rows, cols, 3, 6), (p, ob.ptr, ot.ptr, rows, cols, 16, 40), (p, ob.ptr, ot.ptr, rows, cols, 16, 64),
                 (p, None, None, rows, cols, 0, 0), (None, ob.ptr, ot.ptr, rows, cols, 0, 0), (p, ob.ptr, ot.ptr, 0, cols, 0, 0),
                 (p, ob.ptr, ot.ptr, rows, cols, 16, -16)):
        assert lib.clipk_cast_transpose(*args, st) == BAD_ARG, args[3:]
    # 64 * 65 535 + 1 rows: one row tile more than grid y holds - refused before the launch, as include/clipk.h says
    assert lib.clipk_cast_transpose(p, ob.ptr, ot.ptr, 64 * 65535 + 1, 1, 0, 0, st) == UNSUPPORTED
    assert lib.clipk_cast_transpose_batched(None, 1, st) == BAD_ARG
    assert lib.clipk_cast_transpose_batched(w.data_ptr(), 0, st) == BAD_ARG
    torch.cuda.synchronize()
    assert ob.untouched_outside() and ot.untouched_outside()


# ------------------------------------------------------------------------------------------------ pool_varlen
LENS = [1, 7, 0, 8, 9, 16, 17, 40]      # around the 8-way unrolled loop; one empty sequence
CU0 = 3                                 # rows before the first sequence and two behind the last belong to nobody


def _cu():
    return torch.tensor([CU0] + [CU0 + sum(LENS[:i + 1]) for i in range(len(LENS))], dtype=torch.int32)


def _pool_varlen_fwd(x, cu, d, mode, dev):
    ops = _ops()
    B = cu.numel() - 1
    y = _Fenced(B * d, dev)
    xd, cud = x.to(dev), cu.to(dev)
    rc = ops._lib().clipk_pool_varlen_fwd(xd.data_ptr(), cud.data_ptr(), y.ptr, B, d, mode, ops._stream())
    torch.cuda.synchronize()
    return rc, y


def _pool_varlen_bwd(dy, cu, T, d, mode, dev):
    ops = _ops()
    B = cu.numel() - 1
    dx = _Fenced(T * d, dev)
    dyd, cud = dy.to(dev), cu.to(dev)
    rc = ops._lib().clipk_pool_varlen_bwd(dyd.data_ptr(), cud.data_ptr(), dx.ptr, B, d, mode, ops._stream())
    torch.cuda.synchronize()
    return rc, dx


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("d", [1, 63, 4, 60, 64, 68, 256])
def test_pool_varlen(dev, d, mode):
    """pool_varlen_fwd_kernel / pool_varlen_bwd_kernel: lengths on both sides of the 8-way unrolled loop and an empty sequence
    (y = 0, no dx row), cu[0] = 3 and T = cu[B] + 2 (the rows outside [cu[0], cu[B]) of dx keep their fill), d below / at /
    past the 64-column block (d % 4 != 0: forward only), 40 x 256 / 4 = 2560 chunks: the second trip of the backward's
    grid-stride loop.  Mode 0 and its backward: bit for bit.  The mean: rtol 1e-5 + atol 1e-6 against f64 (sequential f32
    sum of <= 40 terms: 40 x 2^-24 = 2.4e-6 of sum |x|).  Its backward dy * (1 / n): two f32 roundings, 2^-23 |dy / n|."""
    cu = _cu()
    B, T = len(LENS), int(cu[-1]) + 2
    x, dy = _randn((T, d), 50 + d), _randn((B, d), 51 + d)
    rc, y = _pool_varlen_fwd(x, cu, d, mode, dev)
    assert rc == 0 and y.untouched_outside(torch.ones(B * d, dtype=torch.bool))
    got = y.f32().view(B, d)
    for b, n in enumerate(LENS):
        rows = x[int(cu[b]):int(cu[b + 1])]
        if n == 0:
            assert (got[b] == 0).all(), "empty sequence"
        elif mode == 0:
            assert torch.equal(_bits32(got[b]), _bits32(rows[0])), f"sequence {b}: not its first row's bits"
        else:
            ref = rows.to(F64).mean(0)
            err = (got[b].to(F64) - ref).abs()
            tol = 1e-6 + 1e-5 * ref.abs()
            assert (err <= tol).all(), (b, n, float((err - tol).max()))
            _note("pool_varlen mean", (err / tol).max())
    if mode == 0:
        _note("pool_varlen first row", n=B)
    if d % 4:
        return
    rc, dx = _pool_varlen_bwd(dy, cu, T, d, mode, dev)
    owned = torch.zeros(T, d, dtype=torch.bool)
    owned[CU0:int(cu[-1])] = True
    assert rc == 0 and dx.untouched_outside(owned), "a row outside [cu[0], cu[B]) was written"
    gdx = dx.f32().view(T, d)
    for b, n in enumerate(LENS):
        rows = gdx[int(cu[b]):int(cu[b + 1])]
        if n == 0:
            continue
        if mode == 0:
            assert torch.equal(_bits32(rows[0]), _bits32(dy[b])) and (rows[1:] == 0).all(), f"sequence {b}"
        else:
            ref = (dy[b].to(F64) / n).expand(n, d)
            err, tol = (rows.to(F64) - ref).abs(), 2.0 ** -23 * ref.abs()
            assert (err <= tol).all(), (b, n)
            _note("pool_varlen mean backward", (err / tol.clamp(min=1e-300)).max())


def test_pool_backwards_refuse_d_not_a_multiple_of_4_alike(dev):
    """d % 4 != 0 (the backwards write float4 rows): CLIPK_ERR_UNSUPPORTED - the code include/clipk.h documents for a shape the
    kernels do not tile - from clipk_pool_bwd and clipk_pool_varlen_bwd alike, nothing written."""
    ops = _ops()
    lib, st = ops._lib(), ops._stream()
    B, L, d = 3, 5, 6
    dy = torch.zeros(B, d, device=dev)
    cu = torch.tensor([0, 5, 10, 15], dtype=torch.int32, device=dev)
    dx = _Fenced(B * L * d, dev)
    assert lib.clipk_pool_bwd(dy.data_ptr(), None, dx.ptr, B, L, d, 1, st) == UNSUPPORTED
    assert lib.clipk_pool_varlen_bwd(dy.data_ptr(), cu.data_ptr(), dx.ptr, B, d, 1, st) == UNSUPPORTED
    assert lib.clipk_pool_varlen_bwd(dy.data_ptr(), None, dx.ptr, B, 8, 1, st) == BAD_ARG
    assert lib.clipk_pool_varlen_bwd(dy.data_ptr(), cu.data_ptr(), dx.ptr, 0, 8, 1, st) == BAD_ARG
    torch.cuda.synchronize()
    assert dx.untouched_outside()


def test_pools_with_more_sequences_than_grid_y(dev):
    """B = 65 536, L = 1, d = 4: one sequence more than grid y holds; the kernels walk the sequences with a grid-stride loop
    (before: a launch error).  One row per sequence: the mean, the first row and the mean's backward are the row itself."""
    ops = _ops()
    lib, st = ops._lib(), ops._stream()
    B, d = 65536, 4
    x = _randn((B, d), 60)
    xd = x.to(dev)
    cu = torch.arange(B + 1, dtype=torch.int32)
    for mode in (0, 1):
        y = _Fenced(B * d, dev)
        assert lib.clipk_pool_fwd(xd.data_ptr(), None, y.ptr, B, 1, d, mode, st) == 0
        torch.cuda.synchronize()
        assert y.untouched_outside(torch.ones(B * d, dtype=torch.bool))
        assert torch.equal(y.read(), _bits32(x).view(-1)), f"pool_fwd mode {mode}"
        rc, y = _pool_varlen_fwd(x, cu, d, mode, dev)
        assert rc == 0 and y.untouched_outside(torch.ones(B * d, dtype=torch.bool))
        assert torch.equal(y.read(), _bits32(x).view(-1)), f"pool_varlen_fwd mode {mode}"
        rc, dx = _pool_varlen_bwd(x, cu, B, d, mode, dev)
        assert rc == 0 and dx.untouched_outside(torch.ones(B * d, dtype=torch.bool))
        assert torch.equal(dx.read(), _bits32(x).view(-1)), f"pool_varlen_bwd mode {mode}"
        _note("pools past grid y", n=3 * B * d)


# ------------------------------------------------------------------------------------------------ rope_qk
def _rope_reference(qkv, B, L, H, D, cos, sin):
    """f64 rotate-half RoPE of the q and k thirds at position t % L (attention_ref's convention and tables) ->
    (reference [T, 3, H, D], slack): slack = 2^-23 (|x1 c| + |x2 s|), the f32 rounding of the product x2 s and of the fma."""
    T = B * L
    x = qkv.to(F64).view(T, 3, H, D)
    pos = torch.arange(T) % L
    c = torch.cat([cos, cos], -1).to(F64)[pos][:, None, None, :]
    s = torch.cat([sin, sin], -1).to(F64)[pos][:, None, None, :]
    ref = x.clone()
    ref[:, :2] = x[:, :2] * c + A._rot_half(x[:, :2]) * s
    slack = 2.0 ** -23 * ((x[:, :2] * c).abs() + (A._rot_half(x[:, :2]) * s).abs())
    return ref, slack


@pytest.mark.parametrize("L,H", [(5, 3), (37, 3)])
@pytest.mark.parametrize("D", [16, 24, 32, 64, 128])
def test_rope_qk(dev, D, L, H):
    """rope_qk_kernel<D>, every instantiation, B = 2 (the position wraps at t = L), 60 rows (one partial block) and 444 (one
    full block and a partial one).  Each element is the bf16 rounding of a value within `slack` of the f64 rotation:
    between round_bf16(ref - slack) and round_bf16(ref + slack).  The v third and the fence behind qkv: untouched bits."""
    ops = _ops()
    B = 2
    T = B * L
    qkv = _randn((T, 3 * H * D), 70 + D + L).to(torch.bfloat16)
    cos, sin = A.rope_tables(L, D)
    buf = _Fenced(qkv.numel(), dev, 16).fill(qkv)
    cd, sd = cos.to(dev), sin.to(dev)
    rc = ops._lib().clipk_rope_qk(buf.ptr, cd.data_ptr(), sd.data_ptr(), B, L, H, D, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0 and buf.untouched_outside(torch.ones(qkv.numel(), dtype=torch.bool))
    got = R.bf16_from_bits(buf.read().numpy().view(np.uint16)).view(T, 3, H, D)
    assert torch.equal(got[:, 2].view(torch.int16), qkv.view(T, 3, H, D)[:, 2].view(torch.int16)), "v was touched"
    ref, slack = _rope_reference(qkv, B, L, H, D, cos, sin)
    lo = R.round_f64_to_bf16(ref[:, :2] - slack)
    hi = R.round_f64_to_bf16(ref[:, :2] + slack)
    g = got[:, :2].to(F64)
    bad = (g < lo) | (g > hi)
    assert not bad.any(), f"{int(bad.sum())} elements outside the rounding interval, first at {bad.nonzero()[0].tolist()}"
    exact = R.round_f64_to_bf16(ref[:, :2])
    _note(f"rope_qk D={D}", float((g != exact).float().mean()), n=g.numel())
    assert (g != qkv.to(F64).view(T, 3, H, D)[:, :2]).any()


def test_rope_qk_refusals(dev):
    """D = 40 and D = 96 (no instantiation): UNSUPPORTED; missing tables or a pointer off 16 bytes: BAD_ARG; qkv unchanged."""
    ops = _ops()
    lib, st = ops._lib(), ops._stream()
    B, L, H = 2, 3, 2
    tab = torch.zeros(L, 64, device=dev)
    for D in (40, 96):
        buf = _Fenced(B * L * 3 * H * D, dev, 16)
        assert lib.clipk_rope_qk(buf.ptr, tab.data_ptr(), tab.data_ptr(), B, L, H, D, st) == UNSUPPORTED
        torch.cuda.synchronize()
        assert buf.untouched_outside()
    D = 16
    buf = _Fenced(B * L * 3 * H * D + 8, dev, 16)
    assert lib.clipk_rope_qk(buf.ptr, None, tab.data_ptr(), B, L, H, D, st) == BAD_ARG
    assert lib.clipk_rope_qk(buf.ptr, tab.data_ptr(), None, B, L, H, D, st) == BAD_ARG
    assert lib.clipk_rope_qk(buf.ptr + 2, tab.data_ptr(), tab.data_ptr(), B, L, H, D, st) == BAD_ARG
    assert lib.clipk_rope_qk(None, tab.data_ptr(), tab.data_ptr(), B, L, H, D, st) == BAD_ARG
    torch.cuda.synchronize()
    assert buf.untouched_outside()
