"""GPU: the small kernels of csrc/elementwise.hip and the column-sum / L2-norm kernels of csrc/rowwise.hip against the plain
f64 references of tests/elementwise_ref.py (pinned against torch's own f64 ops by tests/test_elementwise_ref_host.py), at
the sizes where their branches change: vector tails, the second trip of a grid-stride loop (the grid is capped at 2048 x
256 threads), the unrolled part of the reduce loops, the second MFMA accumulator, the LDS-table chunks, the clamp, the
device-scalar optimiser path.  Every input comes from a seeded CPU generator; each docstring names the branch the test
exists for.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise_ref as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
SIZES = [1, 7, 8, 9, 255, 257, 4099]
WRAP = 2 * 524288 + 37                  # per-element kernels: third trip of the grid-stride loop, ragged
WRAP_SUMSQ = 2097152 + 1027             # sumsq (4 per thread): second trip, 3-element tail
WRAP_CAST = 4194304 + 8 * 300 + 5       # casts / dact (8 per thread): second trip of the body, 5-element tail
UNSUPPORTED = -2                        # include/clipk.h CLIPK_ERR_UNSUPPORTED
GUARD = 16


def _ops():
    from clip_dplm_amd import ops
    return ops


def _randn(shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def _close(got, ref, rtol, atol):
    """|got - ref| <= atol + rtol |ref| against an f64 reference, with the worst excess in the message."""
    got = got.detach().cpu().to(F64)
    err = (got - ref).abs() - (atol + rtol * ref.abs())
    assert torch.isfinite(got).all() and (err <= 0).all(), f"worst excess {float(err.max()):.3e}"


def _within(got, ref, tol):
    got = got.detach().cpu().to(F64)
    err = (got - ref).abs() - tol
    assert torch.isfinite(got).all() and (err <= 0).all(), f"worst excess {float(err.max()):.3e}"


# ------------------------------------------------------------------------------------------------ casts
def _cast_to_bf16(x_cpu, dev):
    """clipk_cast_f32_to_bf16 into the first n elements of an n + 16 buffer -> (bf16 bits, guard untouched)."""
    ops = _ops()
    n = x_cpu.numel()
    x = x_cpu.to(dev)
    buf = torch.full((n + GUARD,), 0x5a5a, dtype=torch.int16, device=dev)
    ops.check(ops._lib().clipk_cast_f32_to_bf16(x.data_ptr(), buf.data_ptr(), n, ops._stream()), "clipk_cast_f32_to_bf16")
    out = buf.cpu()
    return out[:n].numpy().view(np.uint16), bool((out[n:] == 0x5a5a).all())


def _cast_to_f32(bits_cpu, dev):
    ops = _ops()
    n = bits_cpu.numel()
    x = bits_cpu.to(dev)
    buf = torch.full((n + GUARD,), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    ops.check(ops._lib().clipk_cast_bf16_to_f32(x.data_ptr(), buf.data_ptr(), n, ops._stream()), "clipk_cast_bf16_to_f32")
    out = buf.cpu()
    return out[:n].numpy().view(np.uint32), bool((out[n:] == 0x5a5a5a5a).all())


@pytest.mark.parametrize("n", SIZES + [WRAP_CAST])
def test_casts_bitwise_at_tail_and_wrap_sizes(dev, n):
    """cast_f32_bf16_kernel / cast_bf16_f32_kernel: the scalar tail (n % 8 != 0, and n < 8: no vector body at all), the
    second trip of the 8-per-thread body loop (n > 4 194 304) with a ragged tail behind it, and no byte written past n.
    Bitwise against the integer RNE of the reference and against torch."""
    x = _randn((n,), 100 + n % 97, 3.0)
    got, guard_ok = _cast_to_bf16(x, dev)
    assert guard_ok, "cast_f32_to_bf16 wrote past n"
    assert np.array_equal(got, R.bf16_rne_bits(R.f32_bits(x)))
    assert np.array_equal(got, R.bf16_bits(x.to(torch.bfloat16)))
    back, guard_ok = _cast_to_f32(torch.from_numpy(got.view(np.int16)), dev)
    assert guard_ok, "cast_bf16_to_f32 wrote past n"
    assert np.array_equal(back, got.astype(np.uint32) << 16)


def test_cast_to_f32_is_a_shift_for_every_bf16_pattern(dev):
    """cast_bf16_f32_kernel over all 65 536 bit patterns plus a 3-element tail: NaN payloads, infinities and subnormals
    come through as the pattern shifted by 16."""
    bits = np.concatenate([np.arange(65536, dtype=np.uint32), np.array([0x7fc1, 0x0001, 0xff80], dtype=np.uint32)])
    got, guard_ok = _cast_to_f32(torch.from_numpy(bits.astype(np.uint16).view(np.int16)), dev)
    assert guard_ok and np.array_equal(got, bits << 16)


def test_cast_to_bf16_rounding_table_in_the_vector_body_and_in_the_scalar_tail(dev):
    """f32 -> bf16 on ties (both directions), a carry into the exponent, overflow to inf, +-inf, quiet and signalling NaN,
    +-0, the smallest normal and subnormals, each placed at an index < 8 (n / 8) (pack_bf16x2, the vector body) and at
    one >= that (f32_to_bf16, the scalar tail): both paths give torch's bits (NaN: some NaN), so the same bits."""
    tab = R.CAST_TABLE
    nan = (tab & 0x7fffffff) > 0x7f800000
    want = R.bf16_rne_bits(tab)
    assert np.array_equal(want[~nan], R.bf16_bits(R.f32_from_bits(tab).to(torch.bfloat16))[~nan])
    body_n = 8 * ((len(tab) + 7) // 8)
    for k0 in range(0, len(tab), 7):                         # the tail holds 7 elements: the table goes through it in chunks
        sel = np.arange(k0, min(k0 + 7, len(tab)))
        bits = np.concatenate([tab, np.zeros(body_n - len(tab), dtype=np.uint32), tab[sel], np.zeros(7 - len(sel), np.uint32)])
        got, guard_ok = _cast_to_bf16(R.f32_from_bits(bits), dev)
        assert guard_ok
        body, tail = got[:len(tab)], got[body_n:body_n + len(sel)]
        for name, g, w, isnan, src in (("body", body, want, nan, tab), ("tail", tail, want[sel], nan[sel], tab[sel])):
            bad = np.nonzero((g != w) & ~isnan)[0]
            assert bad.size == 0, f"{name}: " + ", ".join(f"{src[i]:#010x} -> {g[i]:#06x} (want {w[i]:#06x})" for i in bad)
            assert ((g[isnan] & 0x7fff) > 0x7f80).all(), f"{name}: a NaN did not stay NaN"
        assert np.array_equal(body[sel][~nan[sel]], tail[~nan[sel]])


# ------------------------------------------------------------------------------------------------ activations
def _act_inputs(n, seed):
    return _randn((n,), seed, 3.0), _randn((n,), seed + 1)


@pytest.mark.parametrize("name", R.ACTS)
@pytest.mark.parametrize("n", SIZES + [WRAP])
def test_act_fwd_bwd_sizes(dev, n, name):
    """act_fwd_kernel / act_bwd_kernel: one thread per element, so n = 1 .. 4099 are a partial block, a partial last block
    and 17 blocks; n = 2 * 524 288 + 37 takes the grid-stride loop through a second and a ragged third trip.  Tolerance:
    the activation's own (elementwise_ref.act_tol) times |dy|, plus 2^-23 |ref| for the f32 product of the backward."""
    ops = _ops()
    x, dy = _act_inputs(n, 200 + n % 89)
    ref = R.act(x, name)
    _within(ops.act_fwd(x.to(dev), name), ref, R.act_tol(x, name, False, ref))
    g = R.act_grad(x, name)
    refb = dy.to(F64) * g
    _within(ops.act_bwd(dy.to(dev), x.to(dev), name), refb, dy.to(F64).abs() * R.act_tol(x, name, True, g) + 2.0 ** -23 * refb.abs())


@pytest.mark.parametrize("name", ["relu", "celu", "softplus"])
def test_act_grid_relu_celu_softplus(dev, name):
    """The branch points of common.h act_apply / act_grad (x > 0, x > 20 and its two f32 neighbours, +-0) and the tails
    (+-88, -104: expf / expm1f / log1pf at their limits) on a dense grid over [-30, 30]: rtol 1e-6, atol 1e-7 against
    f64, forward and gradient (dy = 1)."""
    ops = _ops()
    x = R.act_grid()
    _close(ops.act_fwd(x.to(dev), name), R.act(x, name), 1e-6, 1e-7)
    _close(ops.act_bwd(torch.ones_like(x).to(dev), x.to(dev), name), R.act_grad(x, name), 1e-6, 1e-7)


def test_act_grid_gelu_within_the_measured_tolerance(dev):
    """common.h gelu_erf / gelu_erf_grad (Abramowitz-Stegun 7.1.26 on v_rcp_f32 / v_exp_f32) before any bf16 rounding.
    The same formula in numpy float32 over this grid is off the f64 erf-GELU by at most E max(1, |x|) with E = 1.43e-7
    (recorded 1.5e-7) for GELU and 2.15e-7 (recorded 2.2e-7) for GELU'; the kernel is allowed 4 E max(1, |x|) =
    6.0e-7 max(1, |x|) and 8.8e-7 max(1, |x|): the factor 4 covers the two 1-ulp hardware approximations."""
    ops = _ops()
    x = R.act_grid()
    for grad in (False, True):
        got = ops.act_bwd(torch.ones_like(x).to(dev), x.to(dev), "gelu") if grad else ops.act_fwd(x.to(dev), "gelu")
        ref = R.act_grad(x, "gelu") if grad else R.act(x, "gelu")
        err = ((got.cpu().to(F64) - ref).abs() / x.to(F64).abs().clamp(min=1.0)).max()
        print(f"gelu grad={grad}: max |err| / max(1, |x|) = {float(err):.3e}")
        _within(got, ref, R.act_tol(x, "gelu", grad, ref))


def _dact(dy_cpu, aux_cpu, name, dev):
    """clipk_dact into the first n elements of an n + 16 buffer -> (bf16 bits, guard untouched)."""
    ops = _ops()
    n = aux_cpu.numel()
    dy, aux = dy_cpu.to(dev), aux_cpu.to(dev)
    buf = torch.full((n + GUARD,), 0x5a5a, dtype=torch.int16, device=dev)
    ops.check(ops._lib().clipk_dact(dy.data_ptr(), ops._dt(dy), aux.data_ptr(), ops.ACT[name], buf.data_ptr(), n,
                                    ops._stream()), "clipk_dact")
    out = buf.cpu()
    return out[:n].numpy().view(np.uint16), bool((out[n:] == 0x5a5a).all())


@pytest.mark.parametrize("dy_bf16", [False, True])
@pytest.mark.parametrize("name", R.ACTS)
def test_dact_grid(dev, name, dy_bf16):
    """dact_kernel<DYBF16> on the activation grid, in bf16 bits against bf16(f64 product of the bf16-rounded inputs): equal,
    or one bf16 step away only where the f64 product lies within the activation's tolerance of a rounding boundary, such
    elements capped at 0.1 % of the grid (elementwise_ref.dact_check).

    GELU below x = -4 is the branch this exists for: dact_kernel leaves the A&S erf there (gelu_grad_tail), whose absolute
    error is per cents of a GELU' that small; the numpy float32 emulation of the kernel differs in 4 / 9 of 60 009
    elements (test_elementwise_ref_host), the cap is 60.
    The test prints the three counts before it asserts."""
    x = R.act_grid()
    aux = x.to(torch.bfloat16)
    dy = _randn((x.numel(),), 5)
    bits, guard_ok = _dact(dy.to(torch.bfloat16) if dy_bf16 else dy, aux, name, dev)
    outside, differ, far = R.dact_check(bits, dy, aux, name, dy_bf16)
    print(f"dact {name} dy_bf16={dy_bf16}: outside {outside}, differ {differ}, more than one step {far} of {x.numel()}")
    assert guard_ok
    assert outside == 0
    assert far == 0
    assert differ <= 0.001 * x.numel()


@pytest.mark.parametrize("dy_bf16", [False, True])
@pytest.mark.parametrize("n", SIZES + [WRAP_CAST])
def test_dact_sizes(dev, n, dy_bf16):
    """dact_kernel<DYBF16>: the scalar tail (n % 8, n < 8), the second trip of the 8-per-thread body (n > 4 194 304) and
    no write past n, for both dy dtypes.  Normal inputs (|x| < 6): every result is the bf16 rounding of a value within
    the activation's tolerance of the f64 product; at the large size at most 0.1 % differ from the reference's bits."""
    aux = _randn((n,), 300 + n % 83).to(torch.bfloat16)
    dy = _randn((n,), 301 + n % 83)
    for name in (R.ACTS if n < WRAP_CAST else ("gelu",)):
        bits, guard_ok = _dact(dy.to(torch.bfloat16) if dy_bf16 else dy, aux, name, dev)
        outside, differ, far = R.dact_check(bits, dy, aux, name, dy_bf16)
        assert guard_ok, f"{name}: wrote past n"
        assert outside == 0, f"{name}: {outside} results outside the tolerance interval"
        if n >= WRAP_CAST:
            assert differ <= 0.001 * n, f"{name}: {differ} of {n} differ"


@pytest.mark.parametrize("with_a", [True, False])
@pytest.mark.parametrize("n", SIZES + [WRAP])
def test_axpby_dev(dev, n, with_a):
    """axpby_dev_kernel: y = a + s b with s read from device memory, and the a == NULL form y = s b (the layer-scale
    skip); partial blocks and the second / third grid-stride trip.  Two f32 roundings: 2^-23 (|a| + |s b|)."""
    ops = _ops()
    a, b = _randn((n,), 400 + n % 79), _randn((n,), 401 + n % 79)
    s = torch.tensor([0.37], dtype=torch.float32)
    ref = R.axpby(a if with_a else None, b, float(s))
    scale = (a.to(F64).abs() if with_a else 0.0) + (float(s) * b.to(F64)).abs()
    got = ops.axpby_dev(a.to(dev) if with_a else None, b.to(dev), s.to(dev))
    _within(got, ref, 2.0 ** -23 * scale)


@pytest.mark.parametrize("with_addend", [True, False])
@pytest.mark.parametrize("n", SIZES + [WRAP])
def test_dropout_f32(dev, n, with_addend):
    """dropout_f32_kernel: the mask index is the element index, also on the later grid-stride trips (n = 2 * 524 288 +
    37): bit-equal to the emulator's counter-based mask, with and without the residual addend; p = 0 returns x
    (+ addend) exactly."""
    import ops_emulator as E
    ops = _ops()
    x, a = _randn((n,), 500 + n % 73), (_randn((n,), 501 + n % 73) if with_addend else None)
    ad = a.to(dev) if with_addend else None
    y = ops.dropout_f32(x.to(dev), (0.1, 99), addend=ad)
    assert torch.equal(y.cpu(), E.dropout_f32(x, (0.1, 99), addend=a))
    y0 = ops.dropout_f32(x.to(dev), (0.0, 99), addend=ad)
    assert torch.equal(y0.cpu(), x + a if with_addend else x)


# ------------------------------------------------------------------------------------------------ column sum
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 112, 113, 129, 1000, 4099])
def test_colsum_f32(dev, rows):
    """colreduce_kernel through clipk_colsum_f32 (the bias gradient of every f32 Linear): fewer rows than the 16 row
    groups, the remainder loop alone (rows <= 112), the first trip of the 8-way unrolled loop (s + 7 * 16 < rows: 113
    rows), several trips with a remainder (1000, 4099); columns below / at / past the 16-column block.  Write and
    accumulate forms, 4e-7 sum |x| + 1e-6 per column, bitwise repeatable, nothing written past out[:cols]."""
    ops = _ops()
    for cols in (1, 15, 16, 17, 130, 1280):
        x = _randn((rows, cols), 600 + cols)
        ref, scale = R.colsum(x)
        xd = x.to(dev)
        out = ops.colsum_f32(xd)
        _within(out, ref, 4e-7 * scale + 1e-6)
        assert torch.equal(out, ops.colsum_f32(xd))
        pre = _randn((cols + GUARD,), 601 + cols)
        buf = pre.to(dev)
        ops.colsum_f32(xd, out=buf[:cols], accumulate=True)
        _within(buf[:cols], pre[:cols].to(F64) + ref, 4e-7 * (scale + pre[:cols].to(F64).abs()) + 1e-6)
        assert torch.equal(buf[cols:].cpu(), pre[cols:]), "accumulate wrote past out[:cols]"
        buf2 = pre.to(dev)
        ops.colsum_f32(xd, out=buf2[:cols], accumulate=False)
        assert torch.equal(buf2[:cols], out) and torch.equal(buf2[cols:].cpu(), pre[cols:])


# ------------------------------------------------------------------------------------------------ embedding
def _ids(B, L, V, seed):
    return torch.randint(0, V, (B, L), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("d", [4, 132, 480])
@pytest.mark.parametrize("B,L", [(1, 1), (3, 7), (8, 7300)])
def test_embed_fwd_exact(dev, B, L, d):
    """embed_fwd_kernel: one float4 chunk per row (d = 4), a chunk count that is no power of two, and B L d / 4 past
    524 288 (the grid-stride loop's later trips) at (8, 7300); plain, and with row_scale, mask and mask_token_id.
    Exactly table[id] * scale as one f32 product."""
    ops = _ops()
    V = 33
    ids, table = _ids(B, L, V, 700 + d), _randn((V, d), 701)
    rs = 0.75 + 0.5 * torch.rand(B, generator=torch.Generator().manual_seed(702))
    mask = (torch.rand(B, L, generator=torch.Generator().manual_seed(703)) > 0.2).to(torch.uint8)
    idd, td = ids.to(dev), table.to(dev)
    assert torch.equal(ops.embed_fwd(idd, td).cpu().view(B, L, d), R.embed_fwd(ids, table))
    got = ops.embed_fwd(idd, td, row_scale=rs.to(dev), mask=mask.to(dev).view(-1), mask_token_id=32)
    assert torch.equal(got.cpu().view(B, L, d), R.embed_fwd(ids, table, rs, mask, 32))


def _embed_bwd_case(dev, ids, dx, V, pre, rs=None, mask=None, mask_token_id=-1):
    ops = _ops()
    dt = pre.to(dev)
    ops.embed_bwd(ids.to(dev), dx.to(dev), dt, row_scale=None if rs is None else rs.to(dev),
                  mask=None if mask is None else mask.to(dev).view(-1), mask_token_id=mask_token_id)
    ref, scale = R.embed_bwd(ids, dx, V, rs, mask, mask_token_id)
    p = pre.to(F64)
    _within(dt, p + ref, 4e-7 * (scale + p.abs()) + 1e-6)
    return dt


@pytest.mark.parametrize("d", [4, 132, 480])
@pytest.mark.parametrize("B,L", [(1, 1), (1, 7), (3, 11), (3, 171), (8, 7300)])
def test_embed_bwd_mfma(dev, B, L, d):
    """embed_bwd_mfma_kernel + embed_bwd_reduce_kernel (V <= 64, d % 4 == 0): ids over the whole vocabulary with
    mask_token_id = -1, so that rows 32 .. V-1 - the second accumulator (V > 32) - are non-zero; a lone token (the odd
    half of a token pair is padding), 2 slices (513 tokens) and 115 slices (58 400 tokens: the first trip of the reduce
    kernel's 8-way unrolled loop plus its remainder); one column group with dead lanes (d = 4), two (132: 4 live
    columns in the second) and four (480).  dtable is pre-filled (the kernel adds); 4e-7 sum |terms| + 1e-6 per entry;
    no atomics: two runs give equal bits."""
    T = B * L
    dx = _randn((T, d), 710 + d)
    rs = 0.75 + 0.5 * torch.rand(B, generator=torch.Generator().manual_seed(711))
    mask = (torch.rand(B, L, generator=torch.Generator().manual_seed(712)) > 0.1).to(torch.uint8) if T in (33, 513) else None
    for V in (33, 40, 64):
        ids = _ids(B, L, V, 713 + V)
        if T >= 33:
            assert (ids >= 32).any()
        pre = _randn((V, d), 714)
        a = _embed_bwd_case(dev, ids, dx, V, pre, rs, mask)
        b = _embed_bwd_case(dev, ids, dx, V, pre, rs, mask)
        assert torch.equal(a, b), "the MFMA embedding gradient is not bitwise reproducible"


@pytest.mark.parametrize("B,L", [(3, 171), (16, 1000)])
@pytest.mark.parametrize("V,d", [(65, 100), (300, 100), (33, 30)])
def test_embed_bwd_lds_table(dev, V, d, B, L):
    """embed_bwd_kernel (V > 64, or d % 4 != 0): one 100-column chunk (V = 65), chunks of 40, 40 and a ragged 20
    (V = 300), d = 30 (no float4 path); 16 000 tokens give every wave several tokens.  LDS and global atomics: same
    bound as the MFMA path, no bit equality."""
    dx = _randn((B * L, d), 720 + d)
    rs = 0.75 + 0.5 * torch.rand(B, generator=torch.Generator().manual_seed(721))
    mask = (torch.rand(B, L, generator=torch.Generator().manual_seed(722)) > 0.1).to(torch.uint8)
    _embed_bwd_case(dev, _ids(B, L, V, 723), dx, V, _randn((V, d), 724), rs, mask, mask_token_id=V - 1)


@pytest.mark.parametrize("V,d", [(40, 132), (65, 100), (33, 30)])
def test_embed_bwd_out_of_range_id_contributes_nothing(dev, V, d):
    """Both backward kernels (MFMA: V = 40; LDS table: V = 65 and d = 30): tokens with id -1, V and 2^32 + 3 (which
    narrows to the valid id 3) among valid ones add nothing - dtable is the gradient over the valid tokens only - and
    the entries around dtable are untouched.  The id is tested as int64, before narrowing."""
    ops = _ops()
    B, L = 3, 171
    ids = _ids(B, L, V, 730)
    for k, bad in enumerate((-1, V, 2 ** 32 + 3)):
        ids.view(-1)[5 + 40 * k] = bad
        ids.view(-1)[300 + 7 * k] = bad
    dx = _randn((B * L, d), 731)
    pre = _randn((V + 2, d), 732)
    buf = pre.to(dev)
    ops.embed_bwd(ids.to(dev), dx.to(dev), buf[1:V + 1], mask_token_id=5)
    ref, scale = R.embed_bwd(ids, dx, V, mask_token_id=5)
    valid = (ids >= 0) & (ids < V)
    clean = torch.where(valid, ids, torch.full_like(ids, 5))           # the same tokens dropped as the mask token
    assert torch.equal(ref, R.embed_bwd(clean, dx, V, mask_token_id=5)[0])
    p = pre[1:V + 1].to(F64)
    _within(buf[1:V + 1], p + ref, 4e-7 * (scale + p.abs()) + 1e-6)
    assert torch.equal(buf[0].cpu(), pre[0]) and torch.equal(buf[V + 1].cpu(), pre[V + 1])


# ------------------------------------------------------------------------------------------------ pooling
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("mode", [0, 1])
def test_pool_fwd_bwd(dev, mode, masked):
    """pool_fwd_kernel / pool_bwd_kernel: L below, at and past the 8-way unrolled loop (1, 7, 8, 9, 50), d below / at /
    past the 64-column block (4, 60, 64, 68, 480); no mask at all, and a mask with one fully masked sequence (output 0,
    gradient 0, everything finite).  rtol 1e-5, atol 1e-6 against f64."""
    ops = _ops()
    B = 4
    for L in (1, 7, 8, 9, 50):
        mask = None
        if masked:
            lens = torch.tensor([L, (L + 1) // 2, 0, 1])
            mask = (torch.arange(L)[None] < lens[:, None]).to(torch.uint8).contiguous()
        md = None if mask is None else mask.to(dev).view(-1)
        for d in (4, 60, 64, 68, 480):
            x, dy = _randn((B * L, d), 800 + d), _randn((B, d), 801 + d)
            y = ops.pool_fwd(x.to(dev), B, L, mask=md, mode=mode)
            _close(y, R.pool_fwd(x, B, L, mask, mode), 1e-5, 1e-6)
            dx = ops.pool_bwd(dy.to(dev), B, L, mask=md, mode=mode).view(B, L, d)
            _close(dx, R.pool_bwd(dy, B, L, mask, mode), 1e-5, 1e-6)
            if masked and mode == 1:
                assert (y[2] == 0).all() and (dx[2] == 0).all()


# ------------------------------------------------------------------------------------------------ L2 normalise
@pytest.mark.parametrize("rows", [1, 5, 257])
@pytest.mark.parametrize("cols", [4, 512, 516, 2048])
def test_l2norm_fwd_bwd_with_clamped_rows(dev, rows, cols):
    """l2norm_fwd_kernel / l2norm_bwd_kernel: one float4 in one lane (cols = 4), the VPL = 2 kernel at its limit (512),
    the VPL = 8 kernel just past the switch (516) and at its limit (2048); a partial block of rows (1, 5) and 65 blocks.
    Every batch holds an all-zero row and a row of norm 1e-13 < eps (the one-row batches: one of each kind in turn): the
    clamped branch, y = x / eps and dx = dy / eps; the other rows against f64 autograd of F.normalize."""
    ops = _ops()
    eps = 1e-12
    for kind in (("plain", "zero", "tiny") if rows == 1 else ("mixed",)):
        x = _randn((rows, cols), 900 + cols)
        clamped = []
        if kind == "mixed":
            clamped = [1, 2]
            x[1] = 0.0
            x[2] *= 1e-13 / x[2].to(F64).norm()
        elif kind == "zero":
            clamped, x[0] = [0], 0.0
        elif kind == "tiny":
            clamped = [0]
            x[0] *= 1e-13 / x[0].to(F64).norm()
        free = [r for r in range(rows) if r not in clamped]
        dy = _randn((rows, cols), 901 + cols)
        y, n = ops.l2norm_fwd(x.to(dev), eps)
        dx = ops.l2norm_bwd(dy.to(dev), y, n, eps)
        ry, rn, rdx = R.l2norm(x, dy, eps)
        _close(y, ry, 1e-5, 1e-6)
        _close(n, rn, 1e-5, 0.0)
        if clamped:
            assert (rn[clamped] < eps).all()
            _close(dx[clamped], dy[clamped].to(F64) / eps, 1e-6, 0.0)
        if free:
            xa = x[free].to(F64).requires_grad_(True)
            ya = F.normalize(xa, dim=-1, eps=eps)
            (ga,) = torch.autograd.grad((ya * dy[free].to(F64)).sum(), xa)
            _close(y[free], ya.detach(), 1e-5, 1e-6)
            _close(dx[free], ga, 1e-5, 1e-6)


@pytest.mark.parametrize("cols", [6, 2052])
def test_l2norm_refuses_what_it_cannot_tile(dev, cols):
    """cols % 4 != 0 and cols > 2048 (past VPL = 8): CLIPK_ERR_UNSUPPORTED from both entry points, nothing written."""
    ops = _ops()
    rows = 3
    x = _randn((rows, cols), 910).to(dev)
    y = torch.full((rows, cols), 7.0, device=dev)
    n = torch.full((rows,), 7.0, device=dev)
    lib = ops._lib()
    assert lib.clipk_l2norm_fwd(x.data_ptr(), y.data_ptr(), n.data_ptr(), rows, cols, 1e-12, ops._stream()) == UNSUPPORTED
    assert lib.clipk_l2norm_bwd(x.data_ptr(), x.data_ptr(), n.data_ptr(), y.data_ptr(), rows, cols, 1e-12,
                                ops._stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    assert (y == 7.0).all() and (n == 7.0).all()


# ------------------------------------------------------------------------------------------------ optimiser
@pytest.mark.parametrize("n", SIZES + [6, 4098, WRAP, WRAP_SUMSQ])
def test_sumsq(dev, n):
    """sumsq_partial_kernel / sumsq_final_kernel: float4 body with a scalar tail of 1 (9, 257), 2 (6, 4098) and 3 (7,
    255, 4099, 2 097 152 + 1027) elements, n < 4 (no body), and the second trip of the 4-per-thread loop (n > 2 097 152).
    Relative 1e-5 against f64; fixed summation order: two runs give equal bits."""
    ops = _ops()
    g = _randn((n,), 1000 + n % 71, 3.0)
    gd = g.to(dev)
    a, b = ops.sumsq(gd).clone(), ops.sumsq(gd).clone()
    assert torch.equal(a, b)
    ref = R.sumsq(g)
    assert abs(a.item() - ref) <= 1e-5 * ref


# beta1 / beta2 as the C ABI carries them (f32): 1 - f32(0.999) is 1.3e-5 away from 0.001, which the second moment shows
HP = dict(lr=1e-3, beta1=ctypes.c_float(0.9).value, beta2=ctypes.c_float(0.999).value, eps=1e-8, weight_decay=0.01)


def _adamw_inputs(n, seed, gnorm):
    w, g = _randn((n,), seed), _randn((n,), seed + 1)
    if n > 8:
        g[:3] = 0.0                                          # g = 0 and v = 0: the denominator is eps alone
    if float(g.norm()) > 0:
        g = (g.to(F64) * (gnorm / g.to(F64).norm())).float()
    return w, g


def _adamw_run(dev, w, g, max_norm, grad_scale, with_norm=True, with_bf16=False, steps=(1, 2, 3)):
    """Three steps of the kernel next to three of the f64 reference; w at rtol 1e-5 / atol 1e-6 (test_adamw_clip's
    numbers), m and v at rtol 1e-5 (a handful of f32 roundings per step; they carry the clipping coefficient, which
    Adam's normalised update hides from w)."""
    ops = _ops()
    wk, gd = w.to(dev), g.to(dev)
    mk, vk = torch.zeros_like(wk), torch.zeros_like(wk)
    wb = torch.zeros(w.numel(), dtype=torch.bfloat16, device=dev) if with_bf16 else None
    rw, rm, rv = w.to(F64), torch.zeros(w.numel(), dtype=F64), torch.zeros(w.numel(), dtype=F64)
    for step in steps:
        nsq = ops.sumsq(gd) if with_norm else None
        ops.adamw_step(wk, gd, mk, vk, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["weight_decay"], step,
                       grad_norm_sq=nsq, max_norm=max_norm, grad_scale=grad_scale, w_bf16=wb)
        rw, rm, rv = R.adamw_step(rw, g, rm, rv, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["weight_decay"], step,
                                  max_norm=max_norm if with_norm else None, grad_scale=grad_scale)
        _close(wk, rw, 1e-5, 1e-6)
        _close(mk, rm, 1e-5, 1e-12)
        _close(vk, rv, 1e-5, 1e-14)
        if with_bf16:
            assert torch.equal(wb, wk.to(torch.bfloat16)), "fused w_bf16 != bf16(w)"
    return wk, mk, vk


@pytest.mark.parametrize("n", SIZES + [WRAP])
def test_adamw_clipped_sizes(dev, n):
    """adamw_kernel with clip_grad_norm_ active (coef < 1): partial blocks, and the second / third grid-stride trip at
    n = 2 * 524 288 + 37 (case f); entries with g = 0 and v = 0 (case g): denominator eps, no NaN."""
    w, g = _adamw_inputs(n, 1100 + n % 67, 30.0)
    _adamw_run(dev, w, g, max_norm=1.0, grad_scale=1.0)


def test_adamw_coefficient_clamps_to_one(dev):
    """(a) the coef >= 1 branch: |g| = 0.5 under max_norm = 1 is not clipped (and not scaled up)."""
    w, g = _adamw_inputs(4099, 1110, 0.5)
    assert R.clip_coef(g, 1.0) == 1.0
    _adamw_run(dev, w, g, max_norm=1.0, grad_scale=1.0)


def test_adamw_grad_scale_clips_the_scaled_norm(dev):
    """(b) grad_scale = 1/8: |g| = 4 is 0.5 after scaling - not clipped, although the unscaled norm is above max_norm -
    and |g| = 40 is 5 after scaling, clipped by 1 / 5 and not by 1 / 40 (m and v show the coefficient)."""
    for gnorm in (4.0, 40.0):
        w, g = _adamw_inputs(4099, 1120, gnorm)
        _adamw_run(dev, w, g, max_norm=1.0, grad_scale=0.125)


def test_adamw_without_a_norm_and_with_the_fused_bf16_copy(dev):
    """(c) grad_norm_sq == NULL: no clipping, grad_scale alone; (d) w_bf16 supplied: bit-equal to bf16(w) after every
    step, with and without clipping."""
    w, g = _adamw_inputs(4099, 1130, 30.0)
    _adamw_run(dev, w, g, max_norm=1.0, grad_scale=0.5, with_norm=False)
    _adamw_run(dev, w, g, max_norm=1.0, grad_scale=0.5, with_norm=False, with_bf16=True)
    _adamw_run(dev, w, g, max_norm=1.0, grad_scale=1.0, with_bf16=True)


def test_adamw_hyper_device_scalars_equal_the_host_scalars(dev):
    """(e) the `hyper` path of graph replay: {lr, 1 - beta1^t, sqrt(1 - beta2^t)} read from device memory, rounded to f32
    from double as the launcher rounds its own, with step = 0 and a wrong host lr: w, m, v bit-equal to the host-scalar
    call of the same step."""
    ops = _ops()
    w, g = _adamw_inputs(4099, 1140, 30.0)
    state = {}
    for path in ("host", "hyper"):
        wk, gd = w.to(dev), g.to(dev)
        mk, vk = torch.zeros_like(wk), torch.zeros_like(wk)
        nsq = ops.sumsq(gd).clone()
        for t in (1, 2, 3):
            if path == "host":
                ops.adamw_step(wk, gd, mk, vk, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["weight_decay"], t,
                               grad_norm_sq=nsq, max_norm=1.0)
            else:
                hyper = torch.tensor([ctypes.c_float(HP["lr"]).value, ctypes.c_float(1.0 - HP["beta1"] ** t).value,
                                      ctypes.c_float(math.sqrt(1.0 - HP["beta2"] ** t)).value], dtype=torch.float32).to(dev)
                ops.adamw_step(wk, gd, mk, vk, 123.0, HP["beta1"], HP["beta2"], HP["eps"], HP["weight_decay"], 0,
                               grad_norm_sq=nsq, max_norm=1.0, hyper=hyper)
        state[path] = (wk, mk, vk)
    for a, b, name in zip(state["host"], state["hyper"], "wmv"):
        assert torch.equal(a, b), f"{name}: hyper path != host scalars"
