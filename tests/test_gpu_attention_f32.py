"""GPU: the exact-f32 attention kernels (csrc/attention_f32.hip: attn_f32_fwd_kernel, attn_f32_bwd_dq_kernel,
attn_f32_bwd_dkv_kernel, each <DT = 1 / 2 / 3, RW = 1 / 4>) against the f64 reference of tests/attention_f32_ref.py, branch by
branch.  Inputs are full-mantissa f32 values from seeded CPU generators; references are f64 on the CPU; nothing is masked out
or skipped.  The case table reaches all 18 instantiations (a case's id states its DT and RW; forward, dQ and dK/dV run in
every case): head dims 8 .. 192 with the DT 1 / 2 / 3 edges (64 | 65, 128 | 129) and the three `lpr_log` forms of the staging,
lengths 1 .. 130 on both sides of the 64-key blocks and of the 4 / 16 rows of a workgroup, the rows_per_wave threshold itself
(128 | 127 workgroups), no / prefix / hole masks with a dead first key block, a dead middle block and a sequence with no valid
key, logits peaked to +-60 in both key orders (every block rescales | none does) with a q = 0 row, and dropout p = 0.1 / 0.5 at
both RW in one DT of each size, its mask rebuilt in integer arithmetic (ops_emulator.drop_mult).

Every case goes through the C entry points with out, lse, delta and dqkv inside guarded buffers of the test's own (the Python
wrapper drops delta), is run twice (same bits), and compares out, lse, delta, dq, dk and dv with the project's rule
(attention_ref.check): max-norm deviation from f64 <= max(8 x the deviation of the f32 restatement, 64 x 2^-24 x magnitude).
(At L = 1 dq and dk are identically 0 in the reference - softmax over one key is constant - so the rule's bound is 0 and the
kernels return the rounding residue of dP - delta, about 1e-7: those two outputs of the two L = 1 cases are held to the bound
attention_f32_ref.single_key_bound derives from the number format.)
tests/test_attention_f32_ref_host.py shows on the CPU that this rule rejects nine mutant restatements (wrong dropout key index,
wrong normaliser, ignored mask hole, q / k / v rounded to bf16, ...) at every case they apply to.

What the code promises exactly is compared bit for bit: two calls; a sequence's results against the same sequence in a larger
batch; delta against the key mask; p = 0 with a seed against no dropout; guards and refused calls' outputs untouched.

Worst kernel deviation / bound per instantiation, measured on an MI355X (1.0 = the bound; the file prints them at the end of a
run with -s):
             DT1 RW1   DT1 RW4   DT2 RW1   DT2 RW4   DT3 RW1   DT3 RW4
  forward     0.131     0.127     0.143     0.142     0.161     0.183      (out, lse)
  dQ          0.144     0.153     0.201     0.154     0.255     0.179      (delta, dq)
  dK / dV     0.187     0.171     0.215     0.300     0.209     0.161      (dk, dv)
360 comparisons: the 56 cases of the table and the four larger batches of the batch-independence test.  0.125 = the kernel deviates from the f64 reference exactly as the f32
restatement does; the kernels sum in another order than torch (sequential fma chains over d and over the keys), hence the
somewhat larger figures, all within a third of the bound.  dq and dk of the two L = 1 cases: 0.034 and 0.083 of
single_key_bound.
"""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_f32_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

BAD_ARG, UNSUPPORTED = -1, -2           # include/clipk.h
GUARD = 1024                            # floats before and after every output
SENTINEL = -12288.0
KERNEL_OF = {"out": "fwd", "lse": "fwd", "delta": "dQ", "dq": "dQ", "dk": "dK/dV", "dv": "dK/dV"}
_WORST = {}                             # (kernel, DT, RW) -> [comparisons, worst ratio]


def _ops():
    from clip_dplm_amd import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    print("\nworst kernel deviation / bound per instantiation (comparisons):")
    for kern in ("fwd", "dQ", "dK/dV"):
        print(f"  {kern:6s}" + "".join(f"  DT{dt} RW{rw}: {_WORST.get((kern, dt, rw), [0, 0.0])[1]:.3f} ({_WORST.get((kern, dt, rw), [0])[0]})"
                                      for dt in (1, 2, 3) for rw in (1, 4)))


class _Guarded:
    """n floats between two GUARD-float fences, everything SENTINEL to begin with."""
    def __init__(self, shape, dev):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        self.view = self.buf[GUARD:GUARD + n].view(shape)

    def fences_intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[-GUARD:] == SENTINEL).all())


def _fwd(ops, qkv, mask, B, L, H, D, scale, p, seed, out, lse):
    return ops._lib().clipk_attn_f32_fwd(qkv.data_ptr(), None if mask is None else mask.data_ptr(), out.data_ptr(), lse.data_ptr(),
                                         B, L, H, D, float(scale), float(p), int(seed) & 0xFFFFFFFF, ops._stream())


def _bwd(ops, qkv, mask, out, dout, lse, B, L, H, D, scale, p, seed, delta, dqkv):
    return ops._lib().clipk_attn_f32_bwd(qkv.data_ptr(), None if mask is None else mask.data_ptr(), out.data_ptr(), dout.data_ptr(),
                                         lse.data_ptr(), delta.data_ptr(), dqkv.data_ptr(), B, L, H, D, float(scale), float(p),
                                         int(seed) & 0xFFFFFFFF, ops._stream())


def _run(case, inp, dev, p=None, seed=None, mask="case"):
    """Forward and backward of one case through the C entry points into guarded buffers -> results on the CPU."""
    ops = _ops()
    B, L, H, D = case.B, case.L, case.H, case.D
    p = case.p if p is None else p
    seed = (case.seed if p > 0 else 0) if seed is None else seed
    qkv, dout = inp.qkv.to(dev), inp.dout.to(dev)
    m = inp.mask if isinstance(mask, str) else mask
    m = None if m is None else m.to(dev)
    out, lse = _Guarded((B * L, H * D), dev), _Guarded((B, H, L), dev)
    delta, dqkv = _Guarded((B, H, L), dev), _Guarded((B * L, 3 * H * D), dev)
    assert _fwd(ops, qkv, m, B, L, H, D, case.scale, p, seed, out.view, lse.view) == 0
    assert _bwd(ops, qkv, m, out.view, dout, lse.view, B, L, H, D, case.scale, p, seed, delta.view, dqkv.view) == 0
    torch.cuda.synchronize()
    for nm, g in (("out", out), ("lse", lse), ("delta", delta), ("dqkv", dqkv)):
        assert g.fences_intact(), f"{case.name}: written outside {nm}"
        assert not bool((g.view == SENTINEL).any()), f"{case.name}: {nm} not fully written"
    return SimpleNamespace(out=out.view.cpu(), lse=lse.view.cpu(), delta=delta.view.cpu(), dqkv=dqkv.view.cpu())


def _same(a, b):
    return all(torch.equal(getattr(a, n).view(torch.int32), getattr(b, n).view(torch.int32)) for n in ("out", "lse", "delta", "dqkv"))


def _compare(case, k, inp=None, tag=""):
    r64, st = ref.yardsticks(case, k.out, inp)
    for t in (k.out, k.delta, k.dqkv):
        assert torch.isfinite(t).all(), (case.name, tag)
    ratios = ref.check_all(case, k, r64, st, tag, inp)
    for nm, r in ratios.items():
        w = _WORST.setdefault((KERNEL_OF[nm], case.DT, case.RW), [0, 0.0])
        w[0], w[1] = w[0] + 1, max(w[1], r)
    return ratios


# ------------------------------------------------------------------------------------------------ the case table
@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.name)
def test_case_table(dev, case):
    """Every case of attention_f32_ref.CASES: launch_fwd / launch_bwd<DT> pick RW by rows_per_wave (attention_f32.hip:426-443);
    rows past L of the last workgroup are staged as zeros (stage_rows: 64, 87-88) and skipped at the stores (219, 316, 399);
    masked keys get -inf scores (185) and a block without a valid key leaves m, l and the accumulators alone (188-195); a row
    without any valid key gives out = 0 and lse = -inf (220, 226), and zero gradient rows through `lse != -inf` (292, 367); the
    dropout element index is ((row0 + q) * H + h) * L + key (47-49, 196, 293, 368).  Outputs inside guarded buffers, two runs
    bit-identical (fixed summation order, no atomics), all six outputs under the rule."""
    inp = ref.inputs(case)
    k = _run(case, inp, dev)
    assert _same(k, _run(case, inp, dev)), f"{case.name}: not reproducible"
    if case.mask == "holes":
        L = case.L
        assert (k.out[3 * L:] == 0).all() and (k.lse[3] == float("-inf")).all()
        assert (k.dqkv[3 * L:] == 0).all() and torch.isfinite(k.lse[:3]).all()
    _compare(case, k)


# ------------------------------------------------------------------------------------------------ bitwise promises
@pytest.mark.parametrize("name", ["DT2-RW4-B2-L130-H8-D96-nomask-p0.1", "DT1-RW1-B2-L130-H2-D15-prefix-p0.5"])
def test_p_zero_with_a_seed_is_no_dropout(dev, name):
    """set_dropout (attention_f32.hip:445-450): p = 0 gives drop_thr = 0 and the seed is dropped - the bits of a call without
    dropout, whatever the seed."""
    case = ref.CASE_BY_NAME[name]
    inp = ref.inputs(case)
    assert _same(_run(case, inp, dev, p=0.0, seed=0), _run(case, inp, dev, p=0.0, seed=0x9E3779B9))
    assert not _same(_run(case, inp, dev, p=0.0, seed=0), _run(case, inp, dev))


@pytest.mark.parametrize("Bs,Bl,L,H,D,mask", [(16, 32, 16, 8, 17, None), (16, 32, 16, 8, 65, "prefix"), (1, 3, 130, 2, 129, "prefix"),
                                              (4, 8, 65, 7, 33, None)], ids=["RW4-DT1", "RW4-DT2", "RW1-DT3", "RW4-DT1-L65"])
def test_a_sequence_does_not_depend_on_its_batch(dev, Bs, Bl, L, H, D, mask):
    """A workgroup reads only rows [b L, (b + 1) L) of its own sequence (row0 = b L: attention_f32.hip:159, 240, 335) and both
    batches run the same RW: out, lse, delta and dqkv of Bs sequences are bit-identical whether they are the whole batch, the
    first or the last Bs of a batch of Bl.  Without dropout (its element index counts the packed row on purpose)."""
    assert ref.instantiation(Bs, L, H, D) == ref.instantiation(Bl, L, H, D)
    big = ref._case(Bl, L, H, D, mask)
    inp = ref.make_inputs(big)
    rows = Bs * L

    def sub(lo):
        c = ref._case(Bs, L, H, D, mask)
        return c, SimpleNamespace(qkv=inp.qkv[lo * L:lo * L + rows].contiguous(), dout=inp.dout[lo * L:lo * L + rows].contiguous(),
                                  mask=None if inp.mask is None else inp.mask[lo:lo + Bs].contiguous())
    kb = _run(big, inp, dev)
    _compare(big, kb, inp)
    for lo in (0, Bl - Bs):
        c, si = sub(lo)
        ks = _run(c, si, dev)
        part = SimpleNamespace(out=kb.out[lo * L:lo * L + rows], lse=kb.lse[lo:lo + Bs], delta=kb.delta[lo:lo + Bs],
                               dqkv=kb.dqkv[lo * L:lo * L + rows])
        assert _same(SimpleNamespace(**{n: getattr(part, n).contiguous() for n in ("out", "lse", "delta", "dqkv")}), ks), lo


@pytest.mark.parametrize("name", ["DT1-RW1-B4-L130-H2-D15-holes", "DT3-RW4-B4-L130-H4-D160-holes"])
def test_delta_does_not_depend_on_the_key_mask(dev, name):
    """delta = rowsum(dO * O) is computed from the rows' own dO and O before the key loop (attention_f32.hip:248-274): the same
    bits under no mask, the prefix mask and the mask with holes, and equal to the f64 row sum under the rule."""
    ops = _ops()
    case = ref.CASE_BY_NAME[name]
    inp = ref.inputs(case)
    B, L, H, D = case.B, case.L, case.H, case.D
    k = _run(case, inp, dev, mask=None)
    qkv, dout, out, lse = inp.qkv.to(dev), inp.dout.to(dev), k.out.to(dev), k.lse.to(dev)
    got = []
    for m in (None, ref.A.prefix_mask(L, ref.prefix_lens(B, L)), ref.A.hole_mask(L)):
        delta, dqkv = _Guarded((B, H, L), dev), _Guarded((B * L, 3 * H * D), dev)
        assert _bwd(ops, qkv, None if m is None else m.to(dev), out, dout, lse, B, L, H, D, case.scale, 0.0, 0, delta.view, dqkv.view) == 0
        torch.cuda.synchronize()
        assert delta.fences_intact() and dqkv.fences_intact() and torch.isfinite(dqkv.view).all()
        got.append(delta.view.cpu())
    assert all(torch.equal(g.view(torch.int32), got[0].view(torch.int32)) for g in got[1:])
    want64, want32 = ref.stored_delta(case, inp, k.out, torch.float64), ref.stored_delta(case, inp, k.out, torch.float32)
    ref.A.check(f"{name} delta", got[0], want64, want32, ref.FLOOR)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_return_before_any_launch(dev):
    """`check` and `set_dropout` run before the first launch (attention_f32.hip:452-457, 445-450, 463-469, 479-485): D = 193 and
    L * 3 H D >= 2^31 (32-bit staging offsets; arguments only, on a tiny buffer) are UNSUPPORTED, p = 1, p < 0 and NaN BAD_ARG, a
    qkv off a 16-byte boundary BAD_ARG - forward and backward, nothing written."""
    ops = _ops()
    B, L, H, D = 2, 16, 2, 8
    qkv = torch.zeros(B * L * 3 * H * 193 + 4, device=dev)
    dout = torch.zeros(B * L * H * 193, device=dev)
    bufs = [_Guarded((B * L * H * 193,), dev), _Guarded((B * H * L,), dev), _Guarded((B * H * L,), dev), _Guarded((B * L * 3 * H * 193,), dev)]
    out, lse, delta, dqkv = (g.view for g in bufs)

    def refused(code, q=qkv, B=B, L=L, H=H, D=D, p=0.0):
        assert _fwd(ops, q, None, B, L, H, D, 0.25, p, 7, out, lse) == code
        assert _bwd(ops, q, None, out, dout, lse, B, L, H, D, 0.25, p, 7, delta, dqkv) == code
        torch.cuda.synchronize()
        assert all(bool((g.buf == SENTINEL).all()) for g in bufs)

    refused(UNSUPPORTED, D=193)
    refused(UNSUPPORTED, B=1, L=1 << 20, H=8, D=96)                    # 3 * 8 * 96 * 2^20 >= 2^31
    refused(BAD_ARG, p=1.0)
    refused(BAD_ARG, p=-0.1)
    refused(BAD_ARG, p=float("nan"))
    refused(BAD_ARG, q=qkv[1:])
    with pytest.raises(ops._ffi.ClipkError, match=rf"\(status {UNSUPPORTED}\)"):
        ops.attn_f32_fwd(torch.zeros(B * L, 3 * H * 193, device=dev), B, L, H, 193)
