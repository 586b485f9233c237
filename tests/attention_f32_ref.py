"""Yardstick for the exact-f32 attention kernels (csrc/attention_f32.hip: clipk_attn_f32_fwd / clipk_attn_f32_bwd), built
from the one body of tests/attention_ref.py (`_sequence`: scores, masked keys -> -inf, lse, dropout on the probabilities at
element ((query token row) * H + h) * L + key, out, delta, dq / dk / dv; a row with no valid key gives out = 0, lse = -inf,
zero gradients and no NaN):

`reference(case)`: f64, nothing rounded - attention_ref.reference on THIS module's inputs.  `delta` is what the backward
    is asked to write: rowsum(dO * out) of the f32 `out` it is handed.
`restate_f32(case, mutant=None)`: the same body in f32 with the identity as its rounding - the "f32 restatement": what a
    kernel that keeps every operand, score, probability and statistic in f32 computes, in torch's summation order.
mutants of the restatement, one deliberate mistake each (MUTANTS): those of attention_ref that exist on this path, and
    `bf16in`: q, k and v rounded to bf16 before use - what the path exists to exclude.
    tests/test_attention_f32_ref_host.py shows that the rule rejects each at every case of the table it applies to.

The tolerance is the project's rule, attention_ref.check: max-norm deviation from f64 <= max(8 x the restatement's deviation on
the same inputs, floor x magnitude), with attention_ref.FLOOR_F32 = 64 x 2^-24 for EVERY output: all of them are f32 here.
One exception, forced by the arithmetic: at L = 1 the reference's dq and dk are identically 0 (softmax over one key is
constant), the rule's bound is then 0 x anything, and a correct f32 kernel returns the rounding residue of dP - delta; those
two outputs of the L = 1 cases are held to a bound derived from the number format instead (single_key_bound).

Inputs are full-mantissa f32 values from seeded CPU generators (attention_ref.inputs is bf16-valued and would hide an operand
rounded to bf16).  "peaked" inputs: q_i = a_i 1 + noise, k_j = b_j 1 + noise with b_j running from -1 to 1 along the keys,
with a step at every 64-key block ("up": each later block raises every row's maximum, so every block rescales the
accumulators; "down": the mirror image - the first block holds the maximum and every later one only adds its tail), and
q_scale = 60 / D: scores span about +-60.  Row 0 of every
sequence has q = 0 (all scores 0: the uniform row).

CASES is the one table both test files iterate over.  A case's name states the kernel instantiation the dispatcher picks for
it (attention_f32.hip: DT = 1 / 2 / 3 for D <= 64 / 128 / 192; `rows_per_wave`: RW = 4 when ceil(L / 16) H B >= 128, else 1);
forward, dQ and dK/dV share the pair, so the table reaches 3 x 2 x 3 = 18 instantiations.
"""
import functools
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attention_ref as A  # noqa: E402

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
FLOOR = A.FLOOR_F32

MUTANTS = {m: A.MUTANTS[m] for m in ("key64", "key128", "key192", "norm_dropped", "bwd_nodrop", "hole", "subblock", "pad")}
MUTANTS["bf16in"] = "(j) q, k and v rounded to bf16 before use"


def instantiation(B, L, H, D):
    """(DT, RW) of the kernels the dispatcher launches (clipk_attn_f32_fwd / _bwd, rows_per_wave)."""
    return 1 if D <= 64 else (2 if D <= 128 else 3), 4 if (L + 15) // 16 * H * B >= 128 else 1


def prefix_lens(B, L):
    """Valid-key counts of the "prefix" mask: the first sequence whole, the others 1 + (37 b mod L)."""
    return [L if b == 0 else 1 + (37 * b) % L for b in range(B)]


def mutants_for(case):
    """The mutants that change something at this case (the host test shows each rejected there)."""
    ms = ["bf16in"]
    if case.p > 0:
        ms += [f"key{k}" for k in (64, 128, 192) if case.L > k] + ["norm_dropped", "bwd_nodrop"]
    if case.mask == "holes":
        ms += ["hole", "subblock"]
    if case.D % 32 and case.D <= 160 and case.L > 1:     # (attention_ref's `pad` adds (padded_dim(D) - D) (key mod 3) to the
                                                         # scores: nothing at key 0, so nothing at all at L = 1)
        ms.append("pad")
    return ms


def _case(B, L, H, D, mask=None, p=0.0, peaked=None, tag=""):
    dt, rw = instantiation(B, L, H, D)
    name = f"DT{dt}-RW{rw}-B{B}-L{L}-H{H}-D{D}-{mask or 'nomask'}" + (f"-p{p}" if p else "") + (f"-{peaked}" if peaked else "") + tag
    scale = 60.0 / D if peaked else D ** -0.5
    c = SimpleNamespace(name=name, DT=dt, RW=rw, B=B, L=L, H=H, D=D, mask=mask, p=p, peaked=peaked, rope=None, lens=None,
                        seed=0xf3200000 + 977 * D + 31 * L + B, scale=float(torch.tensor(scale, dtype=F32)))
    c.mutants = tuple(mutants_for(c))
    return c


CASES = []
# head dims at RW = 1: the three lpr_log forms of the staging (D <= 16, <= 32, else), the DT 1 / 2 and 2 / 3 edges with one live
# column in the last tile (65, 129), the largest (192); lengths on both sides of the 64-key blocks and of the 4 rows of a workgroup
for _D, _L, _m in [(8, 1, None), (15, 3, "prefix"), (16, 16, None), (17, 63, "prefix"), (32, 64, None), (33, 65, "prefix"),
                   (64, 128, None), (65, 129, "prefix"), (96, 130, None), (128, 65, "prefix"), (129, 130, None), (160, 63, "prefix"),
                   (192, 129, None)]:
    CASES.append(_case(2, _L, 2, _D, _m))
# the same head dims at RW = 4 (9 x 8 x 2 = 144 workgroups; the last one of each head has 2 of its 16 rows inside L)
for _D, _m in [(15, "prefix"), (33, None), (64, "prefix"), (65, None), (96, "prefix"), (128, None), (129, "prefix"), (160, None),
               (192, "prefix")]:
    CASES.append(_case(2, 130, 8, _D, _m))
# the lengths at RW = 4
for _B, _L, _H, _D, _m in [(16, 1, 8, 8, None), (16, 3, 8, 17, "prefix"), (4, 63, 8, 16, "prefix"), (4, 64, 8, 32, None),
                           (4, 65, 7, 8, "prefix"), (2, 128, 8, 15, None), (2, 129, 8, 17, "prefix")]:
    CASES.append(_case(_B, _L, _H, _D, _m))
# the rows_per_wave threshold itself: 128 workgroups of 16 rows -> RW = 4, 127 -> RW = 1
CASES.append(_case(16, 16, 8, 8, "prefix", tag="-threshold"))
CASES.append(_case(1, 16, 127, 8, None, tag="-threshold"))
# masks with holes (attention_ref.hole_mask: b0 whole; b1 single holes and the MIDDLE 64-key block masked; b2 the first TWO
# blocks masked, then valid keys - the running maximum starts at -inf; b3 no valid key)
for _H, _D in [(2, 15), (2, 96), (2, 129), (4, 33), (4, 65), (4, 160)]:
    CASES.append(_case(4, 130, _H, _D, "holes"))
# peaked logits, both orders, both RW
for _H in (2, 8):
    for _pk in ("up", "down"):
        CASES.append(_case(2, 130, _H, 16, None, peaked=_pk))
CASES.append(_case(2, 130, 8, 96, "prefix", peaked="up"))
# dropout on the probabilities: one DT of each size at both RW, p = 0.1 unmasked and p = 0.5 masked; L = 200 for the key index
# past 192
for _H in (8, 2):
    for _D in (15, 96, 160):
        CASES.append(_case(2, 130, _H, _D, None, p=0.1))
        CASES.append(_case(2, 130, _H, _D, "prefix", p=0.5))
CASES.append(_case(1, 200, 4, 8, None, p=0.1))
CASES.append(_case(4, 130, 4, 17, "holes", p=0.1))
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def mask_of(case):
    if case.mask == "prefix":
        return A.prefix_mask(case.L, prefix_lens(case.B, case.L))
    if case.mask == "holes":
        assert case.B == 4 and case.L >= 130
        return A.hole_mask(case.L)
    return None


def make_inputs(case):
    """qkv f32 [B*L, 3*H*D], dout f32 [B*L, H*D], mask uint8 [B, L] or None."""
    g = torch.Generator().manual_seed(case.seed)
    B, L, H, D = case.B, case.L, case.H, case.D
    T = B * L
    qkv = torch.randn(T, 3, H, D, generator=g, dtype=F32)
    dout = torch.randn(T, H * D, generator=g, dtype=F32)
    if case.peaked:
        amp = 0.5 + 0.5 * torch.rand(T, 1, 1, generator=g)
        ramp = torch.linspace(-1.0, 0.6, L) + 0.2 * (torch.arange(L) // 64)     # a step up at every 64-key block
        ramp = ramp if case.peaked == "up" else -ramp
        qkv[:, 0] = amp + 0.05 * qkv[:, 0]
        qkv[:, 1] = ramp.repeat(B)[:, None, None] + 0.05 * qkv[:, 1]
        qkv[::L, 0] = 0.0
    return SimpleNamespace(qkv=qkv.reshape(T, 3 * H * D).contiguous(), dout=dout, mask=mask_of(case))


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return make_inputs(CASE_BY_NAME[name])


def inputs(case):
    """The table case's inputs: cached, read-only."""
    return _inputs(case.name)


# ------------------------------------------------------------------------------------------------ the two bodies
def reference(case, out=None, inp=None):
    return A.reference(case, out=out, inp=inputs(case) if inp is None else inp)


def restate_f32(case, out=None, mutant=None, inp=None):
    assert mutant is None or mutant in MUTANTS, mutant
    inp = inputs(case) if inp is None else inp
    if mutant == "bf16in":
        inp, mutant = SimpleNamespace(qkv=inp.qkv.to(BF).to(F32), dout=inp.dout, mask=inp.mask), None
    return A._run(case, F32, lambda t: t, mutant, out, False, inp)


# ------------------------------------------------------------------------------------------------ the rule
def outputs(case, res):
    dq, dk, dv = A.split_dqkv(case, res.dqkv)
    return [("out", res.out), ("lse", res.lse), ("delta", res.delta), ("dq", dq), ("dk", dk), ("dv", dv)]


def single_key_bound(case, inp):
    """(bound on |dq|, bound on |dk|), [T, H*D] each, for L = 1.  Softmax over one key is the constant 1, so dq = dk = 0 in
    exact arithmetic whatever the inputs: these two outputs have no magnitude of their own for the rule to scale with, and a
    restatement that happens to sum dP and delta in one order returns an exact 0.  What an f32 kernel returns is
        dS = dP - delta,   dP = sum_d dO_d v_d,   delta = sum_d dO_d out_d,   out = v exactly (P = 1, l = 1),
    two f32 sums of the SAME D products in whatever orders it likes (a chain of D fmas; per-lane partials and a 6-level
    butterfly): each within gamma(D + 6) A of the exact sum, A = sum_d |dO_d v_d|, gamma(n) = n h / (1 - n h), h = 2^-24
    (vector fma and add round to nearest).  Then dq_d = dS k_d q_scale and dk_d = dS q_d q_scale with at most three more
    roundings:  |dq_d| <= 2 gamma(D + 6) A q_scale |k_d| (1 + 2^-20), likewise dk with q.  Derived; nothing measured."""
    assert case.L == 1 and case.mask is None and case.p == 0
    T, H, D = case.B, case.H, case.D
    x = inp.qkv.to(F64).view(T, 3, H, D)
    a = (inp.dout.to(F64).view(T, H, D) * x[:, 2]).abs().sum(-1, keepdim=True)
    n = (D + 6) * 2.0 ** -24
    e = 2 * n / (1 - n) * a * case.scale * (1 + 2.0 ** -20)
    return (e * x[:, 1].abs()).reshape(T, H * D), (e * x[:, 0].abs()).reshape(T, H * D)


def _zero_outputs(case, got, inp, tag, report):
    """dq and dk of an L = 1 case against single_key_bound -> {output: worst |value| / bound}; report: print and assert."""
    bq, bk = single_key_bound(case, inputs(case) if inp is None else inp)
    dq, dk, _ = A.split_dqkv(case, got.dqkv.detach().cpu().to(F64))
    res = {}
    for nm, g, b in (("dq", dq, bq), ("dk", dk, bk)):
        ok = bool((g.abs() <= b).all())
        res[nm] = (ok, float((g.abs() / b.clamp(min=1e-300)).max()))
        if report:
            print(f"{case.name}{tag} {nm}: exactly 0 in the reference; worst |value| / derived bound {res[nm][1]:.3f}")
            assert ok, (case.name, nm, res[nm][1])
    return res


def check_all(case, got, r64, restated, tag="", inp=None):
    """attention_ref.check with FLOOR_F32 on every output -> {output: deviation / bound}.  At L = 1, dq and dk - exactly 0 in
    the reference - are held to single_key_bound instead."""
    zero = _zero_outputs(case, got, inp, tag, True) if case.L == 1 else {}
    res = {nm: A.check(f"{case.name}{tag} {nm}", g, r, s, FLOOR)
           for (nm, g), (_, r), (_, s) in zip(outputs(case, got), outputs(case, r64), outputs(case, restated)) if nm not in zero}
    res.update({nm: v[1] for nm, v in zero.items()})
    return res


def rejected(case, got, r64, restated, tag="", inp=None):
    zero = _zero_outputs(case, got, inp, tag, False) if case.L == 1 else {}
    return [nm for (nm, g), (_, r), (_, s) in zip(outputs(case, got), outputs(case, r64), outputs(case, restated))
            if not (zero[nm][0] if nm in zero else A.deviation(f"{case.name}{tag} {nm}", g, r, s, FLOOR)[0])]


def stored_delta(case, inp, out, dt):
    """rowsum(dO * out) of the `out` the backward is handed, [B, H, L]."""
    d = (inp.dout.to(dt) * out.detach().cpu().to(dt)).view(-1, case.H, case.D).sum(-1)
    return d.view(case.B, case.L, case.H).permute(0, 2, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _cached(name):
    case = CASE_BY_NAME[name]
    return reference(case), restate_f32(case)


def yardsticks(case, out, inp=None):
    """(f64 reference, f32 restatement) with `delta` taken from the f32 `out` that the backward under test was handed;
    table cases are computed once and shared."""
    if inp is None:
        inp = inputs(case)
        r64, st = _cached(case.name)
    else:
        r64, st = reference(case, inp=inp), restate_f32(case, inp=inp)
    return (SimpleNamespace(out=r64.out, lse=r64.lse, dqkv=r64.dqkv, delta=stored_delta(case, inp, out, F64)),
            SimpleNamespace(out=st.out, lse=st.lse, dqkv=st.dqkv, delta=stored_delta(case, inp, out, F32)))
