"""CPU: tests/gemm_f32_ref.py - the yardstick tests/test_gpu_gemm_f32.py compares the exact-f32 GEMM and weight-gradient
kernels with - pinned against an explicit triple loop, torch's own f32 product (a blocked summation order that is neither
the tiled kernel's chain nor the skinny kernel's split) held inside the derived bound on every family, family (c) shown to
be exact in f32, and every mutant - one deliberate mistake each - shown to be rejected at every shape it applies to: by the
exact check on family (c) and by the bound on (a), (b) and (d).  So the same mistake in a kernel fails the GPU file."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import gemm_f32_ref as R  # noqa: E402

F64, F32 = torch.float64, torch.float32
PAD = 3.0                       # what the mutants find where they must not read: operand padding, guard rows
# (M, N, K): tiled and skinny shapes of the GPU file - K % 4 != 0 and == 0, one and several 16-deep steps, M on both sides
# of 32 and 64 - each with enough elements that an integer coincidence on all of them is out of the question
SHAPES = [(5, 9, 3), (63, 37, 18), (64, 65, 17), (65, 33, 66), (17, 31, 260), (33, 40, 1284), (64, 33, 272)]
WSHAPES = [(1, 31, 127), (31, 33, 129), (33, 65, 31), (64, 31, 161), (100, 36, 33)]


def _case(fam, M, N, K):
    """Operands as the device tests store them: a / b rows padded to a multiple of 4 (+ 4) with PAD, the addend in a buffer
    of its own leading dimension ldadd = N + 3 != ldo = N with one guard row."""
    a, b = R.operands(fam, M, N, K, 10)
    bias, addend, alpha, asc = R.epilogue_operands(fam, M, N, 20)
    ld = (K + 3) // 4 * 4 + 4
    aw, bw = torch.full((M, ld), PAD), torch.full((N, ld), PAD)
    aw[:, :K], bw[:, :K] = a, b
    ldadd = N + 3
    abuf = torch.full((M + 1, ldadd), PAD)
    abuf[:M, :N] = addend
    return SimpleNamespace(fam=fam, M=M, N=N, K=K, a=a, b=b, aw=aw, bw=bw, bias=bias, addend=addend, abuf=abuf, ldadd=ldadd,
                           ldo=N, alpha=alpha, asc=asc)


def emulate(c, mutant=None):
    """The full request (alpha, bias, scaled addend) in torch f32, one rounded operation per step; mutant: one of MUTANTS."""
    M, N, K = c.M, c.N, c.K
    a, b = c.a, c.b
    if mutant == "k_last_dropped":
        a, b = a[:, :K - 1], b[:, :K - 1]
    elif mutant == "pair_swapped":                       # a[k] meets b[k + 1] and a[k + 1] meets b[k] in one K = 2 pair
        k0 = (K // 2) // 2 * 2
        b = b.clone()
        b[:, [k0, k0 + 1]] = c.b[:, [k0 + 1, k0]]
    elif mutant == "k_tail_overread":                    # the partial float4 of the K tail takes one element too many
        a, b = c.aw[:, :K + 1], c.bw[:, :K + 1]
    if mutant == "split_twice":                          # two splits of the contraction, the second partial tile added twice
        h = K // 2 // 4 * 4
        p0, p1 = a[:, :h] @ b[:, :h].t(), a[:, h:] @ b[:, h:].t()
        s = (p0 + p1) + p1
    else:
        s = a @ b.t() if a.shape[1] else torch.zeros(M, N)
    alpha, asc = torch.tensor(c.alpha, dtype=F32), torch.tensor(c.asc, dtype=F32)
    v = alpha * (s + c.bias) if mutant == "alpha_on_bias" else alpha * s + c.bias
    if mutant == "addend_ldo":                           # row stride of the OUTPUT used on the addend's buffer
        add = c.abuf.reshape(-1)[(torch.arange(M)[:, None] * c.ldo + torch.arange(N)[None, :])]
    elif mutant == "addend_row_plus_1":
        add = c.abuf[1:M + 1, :N]
    else:
        add = c.abuf[:M, :N]
    return v + asc * add


# mutant -> where it applies
MUTANTS = {
    "k_last_dropped": lambda c: True,
    "pair_swapped": lambda c: c.K >= 2,
    "k_tail_overread": lambda c: c.K % 4 != 0,
    "alpha_on_bias": lambda c: True,
    "addend_ldo": lambda c: c.M > 1,                     # (row 0 has the same offset under either stride)
    "addend_row_plus_1": lambda c: True,
    "split_twice": lambda c: c.M <= 64 and c.K >= 256 and c.K % 4 == 0,     # the skinny form is the one that splits
}


def _reference(c):
    return R.gemm(c.a, c.b, alpha=c.alpha, bias=c.bias, addend=c.addend, addend_scale=c.asc, want_bound=True)


# ---------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("fam", R.FAMILIES)
def test_reference_equals_a_triple_loop(fam):
    M, N, K = 3, 4, 5
    c = _case(fam, M, N, K)
    ref = R.gemm(c.a, c.b, alpha=c.alpha, bias=c.bias, addend=c.addend, addend_scale=c.asc)
    plain = R.gemm(c.a, c.b)
    for m in range(M):
        for n in range(N):
            s = 0.0
            for k in range(K):
                s += float(c.a[m, k]) * float(c.b[n, k])
            assert abs(float(plain[m, n]) - s) <= 1e-15 * max(1.0, abs(s))
            want = c.alpha * s + float(c.bias[n]) + c.asc * float(c.addend[m, n])
            assert abs(float(ref[m, n]) - want) <= 1e-13 * max(1.0, abs(want))
    dy, x = R.wgrad_operands(fam, M, N, K, 30)
    pw, pb = R.randn((N, K), 31), R.randn((N,), 32)
    dw, db = R.wgrad(dy, x, pre_w=pw, pre_b=pb)
    for n in range(N):
        assert abs(float(db[n]) - (sum(float(dy[m, n]) for m in range(M)) + float(pb[n]))) <= 1e-13
        for k in range(K):
            want = sum(float(dy[m, n]) * float(x[m, k]) for m in range(M)) + float(pw[n, k])
            assert abs(float(dw[n, k]) - want) <= 1e-13


def test_inputs_carry_full_mantissas():
    """Nothing is bf16-valued: most elements of (a), (b), (d) change when rounded to bf16; (c) holds small integers."""
    for fam in ("a", "b", "d"):
        a, b = R.operands(fam, 33, 40, 260, 10)
        for t in (a, b, *R.epilogue_operands(fam, 33, 40, 20)[:2], *R.wgrad_operands(fam, 33, 40, 65, 30)):
            assert float((t.to(torch.bfloat16).to(F32) != t).float().mean()) > 0.9
    a, b = R.operands("c", 33, 40, 260, 10)
    assert set(a.unique().tolist()) == set(b.unique().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert float(R.epilogue_operands("d", 33, 40, 20)[1].mean()) > 990


def test_gamma_is_the_standard_bound():
    assert R.gamma(1) == R.U / (1 - R.U) and R.gamma(1284 + 24) < 1.001 * 1308 * R.U
    assert R.SKINNY_ADDS == 24


# ---------------------------------------------------------------------------------------------- torch f32 is inside
@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_torch_f32_product_is_inside_the_bound_and_exact_on_integers(M, N, K, fam):
    c = _case(fam, M, N, K)
    for kw in (dict(), dict(alpha=c.alpha), dict(bias=c.bias), dict(addend=c.addend), dict(addend=c.addend, addend_scale=c.asc),
               dict(alpha=c.alpha, bias=c.bias, addend=c.addend, addend_scale=c.asc)):
        ref, e = R.gemm(c.a, c.b, want_bound=True, **kw)
        v = c.a @ c.b.t()
        if "alpha" in kw:
            v = torch.tensor(c.alpha, dtype=F32) * v
        if "bias" in kw:
            v = v + c.bias
        if "addend" in kw:
            v = v + (torch.tensor(c.asc, dtype=F32) * c.addend if "addend_scale" in kw else c.addend)
        assert R.outside(v, ref, e) == 0, (sorted(kw), float(((v.to(F64) - ref).abs() / e).max()))
        if fam == "c":
            assert torch.equal(v.to(F64), ref), sorted(kw)
    assert torch.equal(emulate(c), v)


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("M,N,K", WSHAPES)
def test_torch_f32_weight_gradient_is_inside_the_bound_and_exact_on_integers(M, N, K, fam):
    dy, x = R.wgrad_operands(fam, M, N, K, 30)
    pw = R.randint((N, K), 31, -3, 3) if fam == "c" else R.randn((N, K), 31)
    pb = R.randint((N,), 32, -3, 3) if fam == "c" else R.randn((N,), 32)
    for acc in (False, True):
        dw, db, e_dw, e_db = R.wgrad(dy, x, pre_w=pw if acc else None, pre_b=pb if acc else None, want_bound=True)
        gw, gb = dy.t() @ x, dy.sum(0)
        if acc:
            gw, gb = gw + pw, gb + pb
        assert R.outside(gw, dw, e_dw) == 0 and R.outside(gb, db, e_db) == 0
        if fam == "c":
            assert torch.equal(gw.to(F64), dw) and torch.equal(gb.to(F64), db)


# ---------------------------------------------------------------------------------------------- mutants
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_forward_mutant_is_rejected_wherever_it_applies(mutant):
    applied = 0
    for M, N, K in SHAPES:
        for fam in R.FAMILIES:
            c = _case(fam, M, N, K)
            if not MUTANTS[mutant](c):
                continue
            applied += 1
            ref, e = _reference(c)
            assert R.outside(emulate(c), ref, e) == 0
            bad = emulate(c, mutant)
            if fam == "c":
                assert not torch.equal(bad.to(F64), ref), f"{mutant} passes the exact check at {(M, N, K)}"
            else:
                n_out = R.outside(bad, ref, e)
                print(f"{mutant} ({fam}) {M}x{N}x{K}: {n_out} of {M * N} elements outside the bound")
                assert n_out > 0, f"{mutant} is inside the bound on family ({fam}) at {(M, N, K)}"
    assert applied >= 8, (mutant, applied)


def test_bias_gradient_summed_over_rows_rounded_up_to_32_is_rejected():
    """db over ceil(M / 32) * 32 rows of dY's buffer (the one-pass kernel walks 16 MT steps of 2 rows): the rows past M hold
    PAD here, NaN in the device test."""
    applied = 0
    for M, N, K in WSHAPES:
        if M % 32 == 0:
            continue
        for fam in R.FAMILIES:
            applied += 1
            dy, x = R.wgrad_operands(fam, M, N, K, 30)
            buf = torch.full(((M + 31) // 32 * 32, N), PAD)
            buf[:M] = dy
            _, db, _, e_db = R.wgrad(dy, x, want_bound=True)
            assert R.outside(dy.sum(0), db, e_db) == 0
            bad = buf.sum(0)
            if fam == "c":
                assert not torch.equal(bad.to(F64), db)
            else:
                assert R.outside(bad, db, e_db) > 0
    assert applied >= 8


def test_an_operand_rounded_to_bf16_is_rejected():
    """What DESIGN.md section 3.3 forbids on this path: the bound sees a bf16-rounded weight on families (a), (b), (d)."""
    for fam in ("a", "b", "d"):
        c = _case(fam, 33, 40, 260)
        ref, e = _reference(c)
        c.b = c.b.to(torch.bfloat16).to(F32)
        assert R.outside(emulate(c), ref, e) > 0.5 * c.M * c.N
