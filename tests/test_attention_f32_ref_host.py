"""tests/attention_f32_ref.py on the CPU: the f64 reference on full-mantissa f32 inputs is pinned against torch's own
attention + autograd, the f32 restatement passes its own rule, and the rule of the GPU file (attention_ref.check with
FLOOR_F32 on every output) is shown to reject every applicable mutant restatement at every case of the GPU table - so an
exact-f32 kernel with the same mistake would fail tests/test_gpu_attention_f32.py.

Where a mutant is not listed for a case (attention_f32_ref.mutants_for), the reason is that it changes nothing there:
  key64 / key128 / key192, norm_dropped, bwd_nodrop   need dropout, and a key index past 64 / 128 / 192;
  hole, subblock                                      need the mask with holes (a prefix mask has neither an isolated masked
                                                      key nor a fully masked aligned 64-key block);
  pad                                                 attention_ref writes it for the padded widths 32 .. 160 of the bf16
                                                      kernels: nothing to add at D % 32 == 0, undefined above 160; the
                                                      term it adds to the scores is 0 at key 0, so it changes nothing
                                                      at L = 1.
No case is dropped for a mutant that applies: the table below is complete."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_f32_ref as ref  # noqa: E402

F64 = torch.float64


def _sdpa(case, inp):
    """F.scaled_dot_product_attention in f64 + autograd on the same inputs (no dropout, every row with a valid key)."""
    B, L, H, D = case.B, case.L, case.H, case.D
    x = inp.qkv.double().requires_grad_(True)
    v5 = x.view(B, L, 3, H, D).permute(2, 0, 3, 1, 4)
    q, k, v = v5[0], v5[1], v5[2]
    am = None if inp.mask is None else inp.mask.bool()[:, None, None, :].expand(B, H, L, L)
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=am, scale=case.scale)
    out = o.permute(0, 2, 1, 3).reshape(B * L, H * D)
    g, = torch.autograd.grad(out, x, inp.dout.double())
    s = (q @ k.transpose(-1, -2)) * case.scale
    if am is not None:
        s = s.masked_fill(~am, float("-inf"))
    return out.detach(), torch.logsumexp(s, -1).detach(), g


@pytest.mark.parametrize("name", ["DT1-RW1-B2-L65-H2-D33-prefix", "DT2-RW1-B2-L130-H2-D96-nomask", "DT1-RW4-B2-L130-H8-D16-nomask-up",
                                  "DT1-RW1-B2-L130-H2-D16-nomask-down"])
def test_reference_vs_sdpa(name):
    case = ref.CASE_BY_NAME[name]
    inp = ref.inputs(case)
    r = ref.reference(case)
    out, lse, g = _sdpa(case, inp)
    assert torch.allclose(r.out, out, rtol=0, atol=1e-12)
    assert torch.allclose(r.lse, lse, rtol=0, atol=1e-12 * 64)
    assert torch.allclose(r.dqkv, g, rtol=0, atol=1e-10)
    want = (inp.dout.double() * out).view(case.B, case.L, case.H, case.D).sum(-1).permute(0, 2, 1)
    assert torch.allclose(r.delta, want, rtol=0, atol=1e-12)


def test_inputs_are_full_mantissa_and_peaked_scores_span_sixty():
    for case in ref.CASES:
        inp = ref.inputs(case)
        assert inp.qkv.dtype == torch.float32 and inp.qkv.shape == (case.B * case.L, 3 * case.H * case.D)
        nz = inp.qkv[inp.qkv != 0]
        assert float((nz.to(torch.bfloat16).float() != nz).float().mean()) > 0.9, case.name
    for order in ("up", "down"):
        case = ref.CASE_BY_NAME[f"DT1-RW4-B2-L130-H8-D16-nomask-{order}"]
        x = ref.inputs(case).qkv.double().view(2, 130, 3, 8, 16)
        s = torch.einsum("bihd,bjhd->bhij", x[:, :, 0], x[:, :, 1]) * case.scale
        assert s.max() > 45 and s.min() < -45
        assert (s[:, :, 0] == 0).all()                                       # the q = 0 row
        blockmax = torch.stack([s[:, :, 1:, j:j + 64].max(-1).values for j in (0, 64, 128)], -1)
        d = blockmax[..., 1:] - blockmax[..., :-1]
        assert (d > 0).all() if order == "up" else (d < 0).all()             # every later block raises / lowers the maximum


def test_case_table_reaches_every_instantiation_and_every_mutant():
    assert {(c.DT, c.RW) for c in ref.CASES} == {(dt, rw) for dt in (1, 2, 3) for rw in (1, 4)}
    used = set()
    for c in ref.CASES:
        assert (c.DT, c.RW) == ref.instantiation(c.B, c.L, c.H, c.D) and c.name.startswith(f"DT{c.DT}-RW{c.RW}-")
        assert c.B * c.H * c.L * c.L <= 16 * 130 * 130, c.name
        used.update(c.mutants)
    assert used == set(ref.MUTANTS)
    drop = {(c.DT, c.RW, c.p) for c in ref.CASES if c.p > 0 and c.L >= 130}
    assert {(dt, rw, p) for dt in (1, 2, 3) for rw in (1, 4) for p in (0.1, 0.5)} <= drop
    assert ref.instantiation(16, 16, 8, 8)[1] == 4 and ref.instantiation(1, 16, 127, 8)[1] == 1


def test_rows_without_a_valid_key():
    case = ref.CASE_BY_NAME["DT1-RW1-B4-L130-H2-D15-holes"]
    L = case.L
    for r in (ref.reference(case), ref.restate_f32(case)):
        for t in (r.out, r.delta, r.dqkv):
            assert torch.isfinite(t).all()
        assert (r.out[3 * L:] == 0).all() and (r.dqkv[3 * L:] == 0).all() and (r.lse[3] == float("-inf")).all()
        assert torch.isfinite(r.lse[:3]).all() and (r.out[:3 * L] != 0).any()


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.name)
def test_restatement_passes_and_every_mutant_is_rejected(case):
    inp = ref.inputs(case)
    T = inp.qkv.shape[0]
    st = ref.restate_f32(case)
    r64 = ref.reference(case, out=st.out)
    assert st.out.shape == (T, case.H * case.D) and st.dqkv.shape == (T, 3 * case.H * case.D)
    assert st.lse.shape == st.delta.shape == (case.B, case.H, case.L)
    for t in (st.out, st.delta, st.dqkv, r64.out, r64.delta, r64.dqkv):
        assert torch.isfinite(t).all()
    assert max(ref.check_all(case, st, r64, st).values()) <= 1 / 8 + 1e-12          # by construction
    assert case.mutants and case.mutants == tuple(ref.mutants_for(case))
    for m in case.mutants:
        mu = ref.restate_f32(case, mutant=m)
        bad = ref.rejected(case, mu, ref.reference(case, out=mu.out), st, tag=f" [{m}]")
        print(f"{case.name}: mutant {m} rejected on {bad}")
        assert bad, (case.name, m, ref.MUTANTS[m])


@pytest.mark.parametrize("name", ["DT1-RW1-B2-L1-H2-D8-nomask", "DT1-RW4-B16-L1-H8-D8-nomask"])
def test_single_key_bound_admits_two_summation_orders_and_rejects_a_rounded_delta(name):
    """L = 1: dq = dk = 0 exactly.  dS = dP - delta with the two sums taken in different orders (a sequential chain against a
    pairwise tree, in f32) stays inside single_key_bound; delta taken from an `out` rounded to bf16 does not; nor does dq with
    the key of another sequence."""
    case = ref.CASE_BY_NAME[name]
    inp = ref.inputs(case)
    T, H, D = case.B, case.H, case.D
    x = inp.qkv.view(T, 3, H, D)
    prod = inp.dout.view(T, H, D) * x[:, 2]
    chain = torch.zeros(T, H)
    for d in range(D):
        chain = chain + prod[..., d]
    tree = prod.view(T, H, D // 2, 2).sum(-1).view(T, H, D // 4, 2).sum(-1).sum(-1)
    sc = torch.tensor(case.scale)

    def result(dS, k=x[:, 1]):
        dq, dk = dS[..., None] * k * sc, dS[..., None] * x[:, 0] * sc
        return SimpleNamespace(dqkv=torch.stack([dq, dk, torch.zeros_like(dq)], 1).reshape(T, 3 * H * D))
    good = ref._zero_outputs(case, result(chain - tree), None, "", False)
    assert good["dq"][0] and good["dk"][0] and (chain != tree).any()
    rounded = (inp.dout.view(T, H, D) * x[:, 2].to(torch.bfloat16).float()).sum(-1)
    bad = ref._zero_outputs(case, result(chain - rounded), None, "", False)
    assert not bad["dq"][0] and not bad["dk"][0]
    st = ref.restate_f32(case)
    assert ref.rejected(case, SimpleNamespace(out=st.out, lse=st.lse, delta=st.delta, dqkv=result(chain - rounded).dqkv + st.dqkv),
                        ref.reference(case, out=st.out), st) == ["dq", "dk"]


def test_yardsticks_take_delta_from_the_out_they_are_given():
    case = ref.CASE_BY_NAME["DT1-RW1-B2-L65-H2-D33-prefix"]
    st = ref.restate_f32(case)
    fake = SimpleNamespace(out=st.out * 2)
    r64, s32 = ref.yardsticks(case, fake.out)
    assert torch.allclose(r64.delta, 2 * ref.reference(case).delta, rtol=0, atol=1e-4)
    assert torch.equal(r64.out, ref.reference(case).out) and s32.delta.dtype == torch.float32
