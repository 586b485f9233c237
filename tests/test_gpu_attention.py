"""The bf16 attention kernels (csrc/attention.hip) against the f64 reference of tests/attention_ref.py, at the branches of
the dispatcher the random-input parity tests of test_gpu_kernels.py do not reach:

  1 dropout in the general kernels (DROP = true instantiations), padded layout: two query blocks, two to four key blocks,
    run-time and compile-time head dims; dropout must keep the dispatcher off the whole-head kernels;
  2 dropout in the packed layout (mask element index from the packed token row, max_len as its stride);
  3 an exact dropout probe: q = 0 and 0 / 1 values make out and dV counts that bf16 holds exactly - compared bit for bit;
  4 key masks with holes, a dead leading key block and a sequence with no valid key (zero out, lse = -inf, zero dqkv, no
    NaN), through every forward / backward kernel choice the options offer;
  5 run-time head dims (every padded width DP, `dt < dtv` guards, zero padding in LDS);
  6 RoPE positions in the packed layout (rotation at staging and the rotating whole-head forward + prerotated backward).

Every case compares out, lse, delta (taken through the C entry points with a buffer of the test's own: the Python wrappers
drop it), dq, dk and dv with attention_ref.check: max-norm deviation from the f64 reference <= max(8 x the deviation of the
bf16 restatement, floor); tests/test_attention_ref_host.py shows on the CPU that this rule rejects twelve mutant
restatements (wrong dropout index, wrong normaliser, ignored mask hole, ...) at every case they apply to.  dout is NOT
zeroed at masked positions: a key mask hides keys, not queries.

Measured on an MI355X (worst kernel deviation / bound over the comparisons of each group; 1.0 = the bound):
    group 1 (dropout, padded)            48 comparisons, worst 0.132
    group 2 (dropout, packed)            12 comparisons, worst 0.125
    group 3 (exact probe)                10 comparisons, worst 0.125 (dq; out, dV, dK bit for bit)
    group 4 (holes, empty sequence)     396 comparisons, worst 0.125 (11 cases x 2 forward x 3 backward choices x 6 outputs)
    group 5 (run-time head dims)         54 comparisons, worst 0.167
    group 6 (packed RoPE)                12 comparisons, worst 0.125
532 comparisons.  0.125 = the kernel deviates from the f64 reference exactly as the restatement does: the largest error is the
rounding of the largest stored element, and both round the same value.  Before the backward kernels held lse = -inf of a
row with no valid key at a finite value, every case of group 4 failed: all of that sequence's dqkv was NaN.
"""
import math
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

_WORST = {}                              # group -> [comparisons, worst ratio]


def _ops():
    from clip_dplm_amd import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    for g in sorted(_WORST):
        print(f"\ngroup {g}: {_WORST[g][0]} comparisons, worst kernel deviation / bound = {_WORST[g][1]:.3f}", end="")
    print(f"\ntotal: {sum(v[0] for v in _WORST.values())} comparisons")


def _cases(group, **kw):
    cs = [c for c in ref.CASES if c.group == group and all(getattr(c, k) == v for k, v in kw.items())]
    return pytest.mark.parametrize("case", cs, ids=lambda c: c.name)


def _forward(case, dev):
    """out, lse of the kernels for a table case (and what the backward needs: the possibly rotated qkv, mask / cu, tables)."""
    ops, inp = _ops(), ref.inputs(case)
    H, D = case.H, case.D
    qkv = inp.qkv.to(dev)                                   # a fresh copy: the prerotated paths rotate it in place
    drop = (case.p, case.seed) if case.p > 0 else None
    tables = tuple(t.to(dev) for t in ref.rope_tables(case.L, D)) if case.rope else None
    if case.lens is not None:
        side = torch.tensor([0] + torch.tensor(case.lens).cumsum(0).tolist(), dtype=torch.int32, device=dev)
        if case.rope == "prerot":
            out, lse = ops.attn_varlen_fwd_rot_(qkv, side, case.L, H, D, tables, q_scale=case.scale)
        else:
            out, lse = ops.attn_varlen_fwd(qkv, side, case.L, H, D, rope=tables, q_scale=case.scale, dropout=drop)
    else:
        side = None if inp.mask is None else inp.mask.to(dev)
        if case.rope == "prerot":
            out, lse = ops.attn_fwd_rot_(qkv, case.B, case.L, H, D, tables, key_mask=side, q_scale=case.scale)
        else:
            out, lse = ops.attn_fwd(qkv, case.B, case.L, H, D, key_mask=side, rope=tables, q_scale=case.scale, dropout=drop)
    return SimpleNamespace(qkv=qkv, out=out, lse=lse, side=side, tables=tables)


def _backward(case, f, dev):
    """dqkv and delta through the C entry point, into buffers of the test's own that start as NaN."""
    from clip_dplm_amd._ffi import check, ptr
    ops = _ops()
    dout = ref.inputs(case).dout.to(dev)
    dqkv = torch.full_like(f.qkv, float("nan"))
    delta = torch.full_like(f.lse, float("nan"))
    cos, sin = f.tables if f.tables is not None else (None, None)
    p_, seed = (case.p, case.seed) if case.p > 0 else (0.0, 0)
    ptrs = (f.qkv.data_ptr(), ptr(f.side), ptr(cos), ptr(sin), f.out.data_ptr(), dout.data_ptr(), f.lse.data_ptr(),
            delta.data_ptr(), dqkv.data_ptr())
    tail = (case.H, case.D, float(case.scale), int(case.rope == "prerot"), float(p_), int(seed), ops._stream())
    if case.lens is not None:
        check(ops._lib().clipk_attn_varlen_bwd(*ptrs, len(case.lens), sum(case.lens), case.L, *tail), "clipk_attn_varlen_bwd")
    else:
        check(ops._lib().clipk_attn_bwd(*ptrs, case.B, case.L, *tail), "clipk_attn_bwd")
    return dqkv, delta


def _run(case, dev):
    f = _forward(case, dev)
    dqkv, delta = _backward(case, f, dev)
    return SimpleNamespace(out=f.out.cpu(), lse=f.lse.cpu(), delta=delta.cpu(), dqkv=dqkv.cpu())


def _compare(case, k, tag=""):
    """Every output of the kernels under `check`; the worst ratio goes to the module's summary."""
    r64, st = ref.yardsticks(case, k.out)
    for t in (k.out, k.delta, k.dqkv):
        assert torch.isfinite(t.float()).all(), (case.name, tag)
    ratio = ref.check_all(case, k, r64, st, tag)
    w = _WORST.setdefault(case.group, [0, 0.0])
    w[0], w[1] = w[0] + 6, max(w[1], ratio)
    return ratio


def _same(a, b):
    return all(torch.equal(getattr(a, n), getattr(b, n)) for n in ("out", "lse", "delta", "dqkv"))


# ------------------------------------------------------------------------------------------------ 1: dropout, padded
@_cases(1)
def test_dropout_padded(dev, case, kopt):
    k = _run(case, dev)
    _compare(case, k)
    if case.D in (24, 96) and case.p == 0.1:
        # 128 < L <= 256 is the whole-head range: with dropout the dispatcher must stay on the general kernels,
        # whatever the options say
        for whole, fused in ((0, 0), (1, 1)):
            kopt("attn_whole_fwd", whole)
            kopt("attn_fused_bwd", fused)
            assert _same(k, _run(case, dev)), (case.name, whole, fused)


def test_rope_with_dropout_is_refused(dev):
    from clip_dplm_amd._ffi import ClipkError
    ops = _ops()
    B, L, H, D = 2, 200, 2, 64
    qkv = torch.zeros(B * L, 3 * H * D, dtype=torch.bfloat16, device=dev)
    tables = tuple(t.to(dev) for t in ref.rope_tables(L, D))
    with pytest.raises(ClipkError, match="unsupported"):
        ops.attn_fwd(qkv, B, L, H, D, rope=tables, q_scale=0.125, dropout=(0.1, 7))
    out, lse = ops.attn_fwd(qkv, B, L, H, D, rope=tables, q_scale=0.125)
    with pytest.raises(ClipkError, match="unsupported"):
        ops.attn_bwd(qkv, out, out, lse, B, L, H, D, rope=tables, q_scale=0.125, dropout=(0.1, 7))


# ------------------------------------------------------------------------------------------------ 2: dropout, packed
@_cases(2)
def test_dropout_packed(dev, case):
    _compare(case, _run(case, dev))


# ------------------------------------------------------------------------------------------------ 3: exact probe
@_cases(3)
def test_dropout_exact_probe(dev, case):
    """P = 1 / 256, multiplier 2, 0 / 1 values: out and dV are counts times 2^-7 - bit for bit; dK = 0 exactly (q = 0)."""
    k = _run(case, dev)
    out, dv = ref.probe_expectation(case)
    dq_k, dk_k, dv_k = ref.split_dqkv(case, k.dqkv)
    assert torch.equal(k.out.double(), out), f"{int((k.out.double() != out).sum())} elements of out differ"
    assert torch.equal(dv_k.double(), dv), f"{int((dv_k.double() != dv).sum())} elements of dV differ"
    assert (dk_k == 0).all()
    assert (k.lse.double() - math.log(case.L)).abs().max() <= ref.FLOOR_F32 * math.log(case.L)
    r64, st = ref.yardsticks(case, k.out)
    ratio = ref.check(f"{case.name} dq", dq_k, ref.split_dqkv(case, r64.dqkv)[0], ref.split_dqkv(case, st.dqkv)[0],
                      ref.FLOOR_BF16)
    w = _WORST.setdefault(3, [0, 0.0])
    w[0], w[1] = w[0] + 5, max(w[1], ratio)


# ------------------------------------------------------------------------------------------------ 4: holes, empty sequence
@_cases(4)
def test_mask_holes_and_empty_sequence(dev, case, kopt):
    """b0 all valid, b1 single holes at 0, 63, 64, 127, 128, L - 1 and keys [64, 128) masked, b2 keys [0, 128) masked, b3 no
    valid key - through the general and the whole-head forward, the dQ + dK/dV pair and the whole-head backward with four
    and eight waves (the options change nothing where the shape has no such kernel)."""
    L = case.L
    for whole in (0, 1):
        kopt("attn_whole_fwd", whole)
        f = _forward(case, dev)
        for fused, waves in ((0, 4), (1, 4), (1, 8)):
            kopt("attn_fused_bwd", fused)
            kopt("attn_fused_waves", waves)
            tag = f" [whole_fwd={whole} fused_bwd={fused} waves={waves}]"
            dqkv, delta = _backward(case, f, dev)
            k = SimpleNamespace(out=f.out.cpu(), lse=f.lse.cpu(), delta=delta.cpu(), dqkv=dqkv.cpu())
            assert torch.isfinite(k.dqkv.float()).all(), f"{case.name}{tag}: {int(torch.isnan(k.dqkv.float()).sum())} NaN in dqkv"
            assert (k.out[3 * L:] == 0).all() and (k.lse[3] == float("-inf")).all(), tag
            assert (k.dqkv[3 * L:] == 0).all() and (k.delta[3] == 0).all(), tag
            assert torch.isfinite(k.lse[:3]).all(), tag
            _compare(case, k, tag)


# ------------------------------------------------------------------------------------------------ 5: run-time head dims
@_cases(5)
def test_runtime_head_dims(dev, case, kopt):
    k = _run(case, dev)
    _compare(case, k)
    if case.D in (72, 88):                # DP = 96 but not the hd-96 whole-head kernel: the option must change nothing
        for fused in (0, 1):
            kopt("attn_fused_bwd", fused)
            assert _same(k, _run(case, dev)), (case.name, fused)


@pytest.mark.parametrize("D", [168, 12])
def test_unsupported_head_dims_are_refused(dev, D):
    """check_common refuses them at every entry point, forward and backward, padded and packed, before anything is launched."""
    from clip_dplm_amd._ffi import ClipkError
    ops = _ops()
    B, L, H = 2, 200, 3
    qkv = torch.zeros(B * L, 3 * H * D, dtype=torch.bfloat16, device=dev)
    out = torch.zeros(B * L, H * D, dtype=torch.bfloat16, device=dev)
    lse = torch.zeros(B, H, L, dtype=torch.float32, device=dev)
    cu = torch.tensor([0, L, 2 * L], dtype=torch.int32, device=dev)
    for call in (lambda: ops.attn_fwd(qkv, B, L, H, D, q_scale=D ** -0.5),
                 lambda: ops.attn_bwd(qkv, out, out, lse, B, L, H, D, q_scale=D ** -0.5),
                 lambda: ops.attn_varlen_fwd(qkv, cu, L, H, D, q_scale=D ** -0.5),
                 lambda: ops.attn_varlen_bwd(qkv, out, out, lse.view(H, B * L), cu, L, H, D, q_scale=D ** -0.5)):
        with pytest.raises(ClipkError, match="unsupported"):
            call()


# ------------------------------------------------------------------------------------------------ 6: packed RoPE
@_cases(6)
def test_packed_rope_positions(dev, case):
    _compare(case, _run(case, dev))
