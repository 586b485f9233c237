"""CPU: tests/gemm_ref.py - the yardstick tests/test_gpu_gemm.py compares the Linear and weight-gradient kernels with -
pinned against torch's own f64 ops, a plain numpy-f32 stand-in (this file's own code: a sequential sum over k in 32-wide
blocks, RNE casts, the epilogue in the documented order) held inside every bound on every input family, and every seeded
fault shown to fall OUTSIDE the bound or to fail the exact check of family (c): the bounds can discriminate."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import elementwise_ref as E  # noqa: E402
import gemm_ref as R  # noqa: E402

F64 = torch.float64
f32 = np.float32
# (M, N, K) of the GPU suite's small forward cases: ragged M / N, K % 64 == 32, one and several K-steps
SHAPES = [(1, 8, 32), (15, 136, 64), (77, 136, 120), (129, 264, 160), (300, 136, 96)]
WSHAPES = [(7, 8, 120), (65, 136, 128), (513, 120, 264), (1100, 264, 136)]


# ---------------------------------------------------------------------------------------------- the f32 stand-in
def _to_bf16_np(x, truncate=False):
    """f32 array -> the bf16 value as f32: RNE (elementwise_ref.bf16_rne_bits), or truncation (the seeded fault)."""
    bits = np.ascontiguousarray(x, dtype=f32).view(np.uint32)
    if truncate:
        return (bits & np.uint32(0xFFFF0000)).view(f32)
    return (E.bf16_rne_bits(bits).astype(np.uint32) << np.uint32(16)).view(f32).reshape(x.shape)


def _matmul_f32(a, b, skip_last_half=False, drop=None):
    """sum over k of a[m, k] b[n, k] in f32: 32-wide blocks (each block's 32 exact products summed in f64 and rounded
    once, like one matrix instruction), blocks added sequentially in f32.  skip_last_half: the last 32-wide block is
    left out.  drop = (m, n, k): that one product is left out."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    K = a.shape[1]
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=f32)
    blocks = list(range(0, K, 32))
    if skip_last_half:
        blocks = blocks[:-1]
    for k0 in blocks:
        blk = a64[:, k0:k0 + 32] @ b64[:, k0:k0 + 32].T
        if drop is not None and k0 <= drop[2] < k0 + 32:
            blk[drop[0], drop[1]] -= a64[drop[0], drop[2]] * b64[drop[1], drop[2]]
        acc = (acc + blk.astype(f32)).astype(f32)
    return acc


def _act_np(v, name):
    if name == "relu":
        return np.maximum(v, f32(0))
    if name == "gelu":
        return E.gelu_as_f32(torch.from_numpy(v)).numpy()
    return v


def _act_grad_np(x, name):
    if name == "relu":
        return (x > 0).astype(f32)
    return E.gelu_grad_as_f32(torch.from_numpy(np.ascontiguousarray(x, dtype=f32))).numpy()


def emulate(a, b, bias=None, act=None, alpha=1.0, residual=None, dact_aux=None, dact=None, keep=None, out_bf16=False,
            fault=None):
    """The Linear in numpy float32, one correctly rounded operation per fused step; fault: one of FAULTS."""
    a, b = a.numpy(), b.numpy()
    M, N = a.shape[0], b.shape[0]
    drop = None
    if fault == "product_dropped":                       # the largest product of the middle element
        m, n = M // 2, N // 2
        drop = (m, n, int(np.argmax(np.abs(a[m] * b[n]))))
    v = _matmul_f32(a, b, skip_last_half=(fault == "half_step_skipped"), drop=drop)
    if alpha != 1.0 and fault != "alpha_ignored":
        v = (v * f32(alpha)).astype(f32)
    if bias is not None:
        bv = bias.numpy()
        if fault == "bias_shifted":
            bv = np.roll(bv, 1)
        v = (v + bv[None, :]).astype(f32)
    if residual is not None and fault == "residual_before_act":
        v = (v + residual.numpy()).astype(f32)
    pre = v
    v = _act_np(v, act)
    if keep is not None:
        v = (v * (keep[0].numpy().astype(f32) * f32(keep[1]))).astype(f32)
    if dact_aux is not None:
        v = (v * _act_grad_np(dact_aux.numpy(), dact)).astype(f32)
    if residual is not None and fault != "residual_before_act":
        v = (v + residual.numpy()).astype(f32)
    if fault == "row_duplicated" and M >= 2:
        v = v.copy()
        v[M - 2] = v[M - 1]
    if out_bf16:
        v = _to_bf16_np(v, truncate=(fault == "truncation"))
    return torch.from_numpy(np.ascontiguousarray(v)), torch.from_numpy(np.ascontiguousarray(pre))


def emulate_wgrad(dy, x, splits=1, dropped_split=None):
    """dY^T X and colsum dY in numpy f32: 64-row steps summed sequentially inside each split, the splits' partial sums
    added in order; dropped_split: that split's partial sum is left out (the seeded fault)."""
    dy, x = dy.numpy(), x.numpy()
    M = dy.shape[0]
    mps = -(-M // splits)
    mps = -(-mps // 64) * 64                             # whole 64-row steps per split
    dw = np.zeros((dy.shape[1], x.shape[1]), dtype=f32)
    db = np.zeros((dy.shape[1],), dtype=f32)
    for s, m0 in enumerate(range(0, M, mps)):
        pw, pb = np.zeros_like(dw), np.zeros_like(db)
        for r0 in range(m0, min(m0 + mps, M), 64):
            r1 = min(r0 + 64, m0 + mps, M)
            pw = (pw + (dy[r0:r1].astype(np.float64).T @ x[r0:r1].astype(np.float64)).astype(f32)).astype(f32)
            pb = (pb + dy[r0:r1].astype(np.float64).sum(0).astype(f32)).astype(f32)
        if s != dropped_split:
            dw, db = (dw + pw).astype(f32), (db + pb).astype(f32)
    return torch.from_numpy(dw), torch.from_numpy(db)


# the epilogue requests the stand-in is run through (the GPU suite's, minus the 8-bit codes)
def _requests(fam, M, N):
    bias, res, aux = R.epilogue_operands(fam, M, N, 20)
    g = torch.Generator().manual_seed(5)
    keep = ((torch.rand(M, N, generator=g) >= 0.5).to(torch.float32), f32(1.0) / (f32(1.0) - f32(0.5)))
    return {
        "plain_nb": dict(),
        "plain": dict(bias=bias),
        "res32": dict(bias=bias, residual=res),
        "pres16": dict(residual=R.bf16(res)),
        "gelu": dict(bias=bias, act="gelu"),
        "dgelu": dict(dact_aux=aux, dact="gelu"),
        "drelu": dict(dact_aux=aux, dact="relu"),
        "relu_res": dict(bias=bias, act="relu", residual=res),
        "alpha": dict(bias=bias, alpha=0.5),
        "dropout": dict(bias=bias, act="relu", keep=keep),
    }


def _outside(got, ref, bound):
    """Number of elements outside the bound (NaN counts)."""
    return int((~((got.to(F64) - ref).abs() <= bound)).sum())


# ---------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("act", [None, "relu", "gelu"])
def test_linear_reference_equals_torch_f64(act):
    M, N, K = 77, 136, 120
    a, b = R.operands("a", M, N, K, 1)
    bias, res, aux = R.epilogue_operands("a", M, N, 20)
    fn = {None: lambda t: t, "relu": F.relu, "gelu": F.gelu}[act]
    pre = 0.5 * (a.to(F64) @ b.to(F64).t()) + bias.to(F64)
    x = aux.to(F64).requires_grad_(True)
    gx, = torch.autograd.grad(fn(x).sum(), x) if act else (torch.ones_like(x),)
    keep = (torch.rand(M, N, generator=torch.Generator().manual_seed(7)) >= 0.3).to(torch.float32)
    want = fn(pre) * keep.to(F64) * 1.25 * gx + res.to(F64)
    got, got_pre = R.linear(a, b, bias=bias, act=act, alpha=0.5, residual=res, dact_aux=aux if act else None, dact=act,
                            keep=(keep, 1.25))
    assert float((got_pre - pre).abs().max()) < 1e-13
    assert float((got - want).abs().max()) < 1e-12 * float(want.abs().max())


def test_wgrad_reference_equals_torch_f64_and_undoes_the_interleaved_order():
    from clip_dplm_amd.ops import il_source_rows
    M, N, K, hd, ilc = 300, 96, 64, 24, 48
    dy, x = R.wgrad_operands("a", M, N, K, 3)
    dw, db = R.wgrad(dy, x)
    assert torch.equal(dw, dy.to(F64).t() @ x.to(F64)) and torch.equal(db, dy.to(F64).sum(0))
    src = il_source_rows(N, hd, ilc)
    assert sorted(src.tolist()) == list(range(N)) and not torch.equal(src, torch.arange(N))
    dw2, db2 = R.wgrad(dy[:, src], x, il=(hd, ilc))
    assert torch.equal(dw2, dw) and torch.equal(db2, db)


def test_bf16_helpers_round_once_to_nearest_even():
    v = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -30, 300.7], dtype=F64)
    assert E.round_f64_to_bf16(v).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, 300.0]
    assert R.half_ulp_bf16(torch.tensor([1.0, 1.99, 2.0, 300.0])).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 1.0]
    assert float(R.gelu8_decode(torch.tensor([226]))) == 1.0 and abs(float(R.gelu8_decode(torch.tensor([26])))) < 4e-9


# ---------------------------------------------------------------------------------------------- the stand-in is inside
@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_f32_stand_in_is_inside_every_forward_bound(M, N, K, fam):
    a, b = R.operands(fam, M, N, K, 10)
    for name, kw in _requests(fam, M, N).items():
        ref, pre, e, e_pre = R.linear(a, b, want_bounds=True, **kw)
        for out_bf16 in (False, True):
            got, got_pre = emulate(a, b, out_bf16=out_bf16, **kw)
            bound = R.bf16_bound(ref, e) if out_bf16 else e
            assert _outside(got, ref, bound) == 0, (name, out_bf16, float(((got.to(F64) - ref).abs() / bound).max()))
            assert _outside(got_pre, pre, e_pre) == 0, name
            if fam == "c" and "gelu" not in (kw.get("act"), kw.get("dact")):
                assert torch.equal(got.to(F64), E.round_f64_to_bf16(ref) if out_bf16 else ref), name


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("M,N,K", WSHAPES)
def test_f32_stand_in_is_inside_every_weight_gradient_bound(M, N, K, fam):
    dy, x = R.wgrad_operands(fam, M, N, K, 30)
    dw, db, e_dw, e_db = R.wgrad(dy, x, want_bounds=True)
    for splits in (1, 2, 3):
        gw, gb = emulate_wgrad(dy, x, splits)
        assert _outside(gw, dw, e_dw) == 0 and _outside(gb, db, e_db) == 0
        if fam == "c":
            assert torch.equal(gw.to(F64), dw) and torch.equal(gb.to(F64), db)


# ---------------------------------------------------------------------------------------------- seeded faults
# fault -> (the request it is seeded in, bf16 output, shape): each must be caught on family (a) by the bound AND by the exact
# check of family (c)
FAULTS = {
    "product_dropped": ("plain", False, (129, 264, 160)),
    "half_step_skipped": ("plain", False, (129, 264, 160)),            # K % 64 == 32: the last 32-wide half K-step
    "row_duplicated": ("plain", False, (129, 264, 160)),
    "bias_shifted": ("plain", False, (15, 136, 64)),
    "truncation": ("plain", True, (129, 264, 160)),
    "residual_before_act": ("relu_res", False, (15, 136, 64)),
    "alpha_ignored": ("alpha", False, (15, 136, 64)),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_every_seeded_forward_fault_is_caught(fault):
    name, out_bf16, (M, N, K) = FAULTS[fault]
    caught = {}
    for fam in ("a", "c"):
        a, b = R.operands(fam, M, N, K, 10)
        kw = _requests(fam, M, N)[name]
        ref, _, e, _ = R.linear(a, b, want_bounds=True, **kw)
        bound = R.bf16_bound(ref, e) if out_bf16 else e
        good, _ = emulate(a, b, out_bf16=out_bf16, **kw)
        bad, _ = emulate(a, b, out_bf16=out_bf16, fault=fault, **kw)
        assert _outside(good, ref, bound) == 0
        exact_ref = E.round_f64_to_bf16(ref) if out_bf16 else ref
        caught[fam] = (_outside(bad, ref, bound) > 0, not torch.equal(bad.to(F64), exact_ref))
    assert caught["a"][0], f"{fault}: inside the bound on family (a)"
    # (the sums of family (c) at K = 160 stay below 256, where every integer IS a bf16 value: a truncating cast changes
    # nothing there - the bound on family (a) is what sees it, on about half of the elements: next test)
    assert caught["c"][1] or fault == "truncation", f"{fault}: passes the exact check of family (c)"


def test_truncation_is_caught_on_a_sizeable_share_of_the_elements():
    """A cast that truncates is off by up to one bf16 ulp, the bound allows half of one plus the f32 error: about half of
    the elements must fall outside, not a stray one."""
    M, N, K = 129, 264, 160
    a, b = R.operands("a", M, N, K, 10)
    ref, _, e, _ = R.linear(a, b, want_bounds=True)
    bad, _ = emulate(a, b, out_bf16=True, fault="truncation")
    assert _outside(bad, ref, R.bf16_bound(ref, e)) > 0.4 * M * N


@pytest.mark.parametrize("M,splits,dropped", [(1100, 3, 1), (1030, 2, 1), (1100, 3, 2)])
def test_a_dropped_split_of_the_weight_gradient_is_caught(M, splits, dropped):
    N, K = 136, 264
    for fam in ("a", "c"):
        dy, x = R.wgrad_operands(fam, M, N, K, 30)
        dw, db, e_dw, e_db = R.wgrad(dy, x, want_bounds=True)
        gw, gb = emulate_wgrad(dy, x, splits, dropped_split=dropped)
        if fam == "a":
            assert _outside(gw, dw, e_dw) > 0 and _outside(gb, db, e_db) > 0
        else:
            assert not torch.equal(gw.to(F64), dw) and not torch.equal(gb.to(F64), db)


def test_code_bound_admits_the_nearest_level_and_rejects_the_next():
    pre = torch.linspace(-6.0, 6.0, 4001, dtype=F64)
    g = E.act_grad(pre, "gelu")
    code = torch.clamp(torch.round((g - R.GD8_MIN) / R.GD8_STEP), 0, 255)
    bound = R.gelu_code_bound(pre, torch.zeros_like(pre))
    assert bool(((R.gelu8_decode(code) - g).abs() <= bound).all())
    assert bool(((R.gelu8_decode(code + 2) - g).abs() > bound).all())
