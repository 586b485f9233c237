"""tests/attention_ref.py on the CPU: the f64 reference is pinned against torch's own attention and against an explicit
triple loop, and the tolerance rule of the GPU tests (attention_ref.check) is shown to reject every mutant restatement at
every case of the GPU table - so a kernel with the same mistake would fail test_gpu_attention.py."""
import math
import os
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_ref as ref  # noqa: E402
from ops_emulator import drop_mult  # noqa: E402

F64 = torch.float64


def _adhoc(B, L, H, D, seed, *, p=0.0, mask=None, rope=None, lens=None):
    """A case outside the table with its inputs."""
    case = ref._case("adhoc", 0, D, ["delta64"], B=B, L=L, H=H, p=p, mask=None, rope=rope, lens=lens)
    g = torch.Generator().manual_seed(seed)
    T = sum(lens) if lens is not None else B * L
    inp = SimpleNamespace(qkv=torch.randn(T, 3 * H * D, generator=g).to(ref.BF),
                          dout=torch.randn(T, H * D, generator=g).to(ref.BF), mask=mask)
    return case, inp


def _sdpa(case, inp):
    """F.scaled_dot_product_attention in f64 + autograd on the same inputs (no dropout); rows without a valid key excluded
    by the caller."""
    B, L, H, D = case.B, case.L, case.H, case.D
    x = inp.qkv.double().requires_grad_(True)
    v5 = x.view(B, L, 3, H, D).permute(2, 0, 3, 1, 4)
    q, k, v = v5[0], v5[1], v5[2]
    if case.rope:
        cos, sin = ref.rope_tables(L, D)
        cosf, sinf = torch.cat([cos, cos], -1).double(), torch.cat([sin, sin], -1).double()
        q, k = q * cosf + ref._rot_half(q) * sinf, k * cosf + ref._rot_half(k) * sinf
    am = None if inp.mask is None else inp.mask.bool()[:, None, None, :].expand(B, H, L, L)
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=am, scale=case.scale)
    out = o.permute(0, 2, 1, 3).reshape(B * L, H * D)
    g, = torch.autograd.grad(out, x, inp.dout.double())
    s = (q @ k.transpose(-1, -2)) * case.scale
    if am is not None:
        s = s.masked_fill(~am, float("-inf"))
    return out.detach(), torch.logsumexp(s, -1).detach(), g


@pytest.mark.parametrize("mask_kind,rope", [(None, None), ("prefix", None), ("holes", None), ("holes", "kernel"),
                                            ("prefix", "kernel")])
def test_reference_vs_sdpa(mask_kind, rope):
    L = 150
    mask = {None: None, "prefix": ref.prefix_mask(L, [L, L - 63, 1]), "holes": ref.hole_mask(L)[:3]}[mask_kind]
    case, inp = _adhoc(3, L, 2, 16, 5, mask=mask, rope=rope)
    r = ref.reference(case, inp=inp)
    out, lse, g = _sdpa(case, inp)
    assert torch.allclose(r.out, out, rtol=0, atol=1e-12)
    assert torch.allclose(r.lse, lse, rtol=0, atol=1e-12)
    assert torch.allclose(r.dqkv, g, rtol=0, atol=1e-11)
    assert torch.allclose(r.delta, (inp.dout.double() * out).view(3, L, 2, 16).sum(-1).permute(0, 2, 1), rtol=0, atol=1e-12)


def test_reference_row_without_valid_key():
    L = 70
    mask = torch.ones(2, L, dtype=torch.uint8)
    mask[1] = 0
    case, inp = _adhoc(2, L, 2, 8, 6, mask=mask)
    for r in (ref.reference(case, inp=inp), ref.restate_bf16(case, inp=inp)):
        for t in (r.out, r.delta, r.dqkv):
            assert torch.isfinite(t).all()
        assert (r.out[L:] == 0).all() and (r.dqkv[L:] == 0).all() and (r.lse[1] == float("-inf")).all()
        assert torch.isfinite(r.lse[0]).all() and (r.out[:L] != 0).any()


def _triple_loop(case, inp, row0_of, Lstride):
    """out / lse / dqkv with dropout from explicit loops over (sequence, head, query, key); autograd for the gradient."""
    H, D = case.H, case.D
    x = inp.qkv.double().requires_grad_(True)
    outs, lses = [], []
    seqs, _ = ref.sequences(case, inp)
    for r0, n, _ in seqs:
        o_seq = [[None] * H for _ in range(n)]
        l_seq = torch.zeros(H, n, dtype=F64)
        for h in range(H):
            for i in range(n):
                q = x[r0 + i, h * D:(h + 1) * D]
                s = torch.stack([(q * x[r0 + j, (H + h) * D:(H + h + 1) * D]).sum() * case.scale for j in range(n)])
                P = torch.softmax(s, 0)
                acc = torch.zeros(D, dtype=F64)
                for j in range(n):
                    idx = torch.tensor(((row0_of(r0) + i) * H + h) * Lstride + j, dtype=torch.int64)
                    acc = acc + P[j] * float(drop_mult(case.p, case.seed, idx)) * x[r0 + j, (2 * H + h) * D:(2 * H + h + 1) * D]
                o_seq[i][h] = acc
                l_seq[h, i] = torch.logsumexp(s.detach(), 0)
        outs.append(torch.stack([torch.cat(o_seq[i]) for i in range(n)]))
        lses.append(l_seq)
    out = torch.cat(outs, 0)
    g, = torch.autograd.grad(out, x, inp.dout.double())
    return out.detach(), lses, g


def test_reference_vs_triple_loop_with_dropout():
    case, inp = _adhoc(2, 5, 2, 8, 7, p=0.3)
    r = ref.reference(case, inp=inp)
    out, lses, g = _triple_loop(case, inp, lambda r0: r0, 5)
    assert torch.allclose(r.out, out, rtol=0, atol=1e-12)
    assert torch.allclose(r.lse, torch.stack(lses), rtol=0, atol=1e-12)
    assert torch.allclose(r.dqkv, g, rtol=0, atol=1e-12)
    assert (r.out != ref.reference(ref._case("adhoc", 0, 8, ["delta64"], B=2, L=5, mask=None), inp=inp).out).any()


def test_reference_packed_with_dropout_vs_triple_loop_and_one_by_one():
    lens = [5, 1, 3]
    case, inp = _adhoc(None, None, 2, 8, 8, p=0.3, lens=lens)
    r = ref.reference(case, inp=inp)
    out, lses, g = _triple_loop(case, inp, lambda r0: r0, max(lens))       # packed row, max_len as the stride
    assert torch.allclose(r.out, out, rtol=0, atol=1e-12)
    assert torch.allclose(r.lse, torch.cat(lses, 1), rtol=0, atol=1e-12)
    assert torch.allclose(r.dqkv, g, rtol=0, atol=1e-12)
    # without dropout (where the packed row does not matter): each sequence alone as a padded batch of one
    case0, _ = _adhoc(None, None, 2, 8, 8, lens=lens)
    case0.rope = "kernel"
    r0 = ref.reference(case0, inp=inp)
    a = 0
    for n in lens:
        one, _ = _adhoc(1, n, 2, 8, 8, rope="kernel")
        one_inp = SimpleNamespace(qkv=inp.qkv[a:a + n], dout=inp.dout[a:a + n], mask=None)
        ro = ref.reference(one, inp=one_inp)
        assert torch.equal(r0.out[a:a + n], ro.out) and torch.equal(r0.dqkv[a:a + n], ro.dqkv)
        assert torch.equal(r0.lse[:, a:a + n], ro.lse[0]) and torch.equal(r0.delta[:, a:a + n], ro.delta[0])
        a += n


def test_case_table_and_mutant_coverage():
    used = set()
    for c in ref.CASES:
        assert c.mutants, c.name
        used.update(c.mutants)
        assert c.B >= 2 and c.H in (2, 3), c.name
    assert used == set(ref.MUTANTS), set(ref.MUTANTS) - used
    assert sorted({c.group for c in ref.CASES}) == [1, 2, 3, 4, 5, 6]


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.name)
def test_restatement_passes_and_every_mutant_is_rejected(case):
    inp = ref.inputs(case)
    T = inp.qkv.shape[0]
    st = ref.restate_bf16(case)
    r64 = ref.reference(case, out=st.out)
    assert st.out.shape == (T, case.H * case.D) and st.dqkv.shape == (T, 3 * case.H * case.D)
    assert st.lse.shape == st.delta.shape == ((case.H, T) if case.lens is not None else (case.B, case.H, case.L))
    for t in (st.out, st.delta, st.dqkv, r64.out, r64.delta, r64.dqkv):
        assert torch.isfinite(t).all()
    assert ref.check_all(case, st, r64, st) <= 1 / 8 + 1e-12          # by construction
    for m in case.mutants:
        mu = ref.restate_bf16(case, mutant=m)
        bad = ref.rejected(case, mu, ref.reference(case, out=mu.out), st, tag=f" [{m}]")
        print(f"{case.name}: mutant {m} rejected on {bad}")
        assert bad, (case.name, m, ref.MUTANTS[m])


@pytest.mark.parametrize("case", [c for c in ref.CASES if c.probe], ids=lambda c: c.name)
def test_exact_probe_argument_holds_on_the_restatement(case):
    """q = 0, V and dO in {0, 1}, p = 0.5, L = 256: P~ in {0, 2 / 256}, every sum a count <= 256 - exact in bf16."""
    st = ref.restate_bf16(case)
    out, dv = ref.probe_expectation(case)
    assert 0 < out.max() <= 2 and torch.equal(out.to(ref.BF).double(), out) and torch.equal(dv.to(ref.BF).double(), dv)
    dq, dk, dvs = ref.split_dqkv(case, st.dqkv)
    assert torch.equal(st.out.double(), out)
    assert torch.equal(dvs.double(), dv)
    assert (dk == 0).all() and (dq != 0).any()
    assert (st.lse.double() - math.log(case.L)).abs().max() <= ref.FLOOR_F32 * math.log(case.L)
