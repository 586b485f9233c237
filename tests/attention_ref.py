"""Yardstick for the bf16 attention kernels (csrc/attention.hip) in plain torch on the CPU, the L x L matrix materialised.

    S = scale q~ k~^T (q~, k~: after rotate-half RoPE),  masked keys -> -inf,  lse = LSE_j S_ij,  P = exp(S - lse)
    P~ = P * keep / (1 - p)  (ops_emulator.drop_mult at element ((query token row) * H + h) * Lstride + key),  out = P~ V
    delta = rowsum(dO * out),  dV = P~^T dO,  dS = P * ((dO V^T) * keep / (1 - p) - delta),
    dq~ = scale dS k~,  dk~ = scale dS^T q~,  dq / dk = RoPE^T of them
    a row with no valid key: out = 0, lse = -inf, P = 0 (zero gradient rows), no NaN anywhere

One body (`_sequence`) serves three users:

`reference(case, out=None)`: f64 on the bf16-valued inputs, nothing rounded.  `delta` is what the backward is ASKED to
    write: rowsum(dO * out) of the STORED bf16 `out` it is handed (the `out` argument; without one, the reference's own
    f64 out).  dS of the reference always uses the exact delta of its own out.  The host test pins this function against
    F.scaled_dot_product_attention + autograd and against an explicit triple loop with dropout.

`restate_bf16(case, out=None, mutant=None)`: the same in f32, rounded to bf16 exactly where the kernels round:
    * rotated q / k rows (rope_regs -> pack_bf16x2; clipk_rope_qk and the whole-head forward store the same bits);
    * the forward's P after the dropout multiplier (pack_acc_pair), un-normalised - exp(S - rowmax) - the division by the
      f32 row sum comes after P~ V;
    * the backward's P after the dropout multiplier (`pk` of the dK/dV kernel), normalised - exp(S - lse) with the f32 lse;
    * dS (pack_acc_pair in the dQ kernel, `dsk` in the dK/dV kernel), before the multiplication by `scale`;
    * the stored `out` and, after RoPE^T in f32, the stored `dqkv`;
    * `lse` and `delta` stay f32; delta comes from the stored bf16 out (the `out` argument or the restatement's own).
    Not restated: the forward's running maximum (P is rounded relative to the maximum so far, then rescaled in f32) and
    the f32 summation order of the matrix cores.

mutants of the restatement, one deliberate mistake each (MUTANTS): the host test shows that `check` rejects each of them at
    every case it applies to, i.e. that the tolerance rule would notice the same mistake in a kernel.

`check(name, got, r64, restated, floor)` is the project's tolerance rule (test_gpu_sinkhorn._close): max-norm deviation from
the f64 reference <= max(8 x the restatement's deviation on the same inputs, floor x magnitude), floor = 2^-7 for bf16
outputs and 64 x 2^-24 for the f32 statistics.

CASES is the one table of shapes, seeds and inputs both test files iterate over.
"""
import functools
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ops_emulator import drop_mult  # noqa: E402

F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
FLOOR_BF16 = 2.0 ** -7                  # one bf16 ulp of the largest element
FLOOR_F32 = 64 * 2.0 ** -24

MUTANTS = {
    "key64": "(a) dropout key index off by one from key 64",
    "key128": "(a) dropout key index off by one from key 128",
    "key192": "(a) dropout key index off by one from key 192",
    "norm_dropped": "(b) softmax normaliser taken from the dropped P",
    "bwd_nodrop": "(c) backward ignores the dropout mask",
    "stride_len": "(d) packed dropout index: the sequence's own length as the stride, not max_len",
    "row_local": "(d) packed dropout index: the row inside the sequence, not the packed row",
    "hole": "(e) a mask hole ignored (the first isolated masked key of each sequence let in)",
    "subblock": "(f) the keys of a fully masked 64-key sub-block let in",
    # (the same constant on every score of a row would shift lse alone - softmax does not see it - so the keys' padding varies)
    "pad": "(g) columns >= D of the padded head not zero in the score product (1 in q's padding, key mod 3 in k's)",
    "delta64": "(h) delta from the unrounded out, not from the stored bf16 out",
    # (a shift common to q and k cancels in q~ . k~ and in RoPE^T: rotary embeddings are relative - so the queries alone)
    "rope_packed": "(i) RoPE position of the query rows counted from the packed row, not from the sequence start",
}


DROPOUT_MUTANTS = frozenset(["key64", "key128", "key192", "norm_dropped", "bwd_nodrop"])     # need p > 0


def padded_dim(D):
    """DP of the kernels (ATTN_DISPATCH): the head dim rounded up to 32, 64, 96, 128 or 160."""
    return next(dp for dp in (32, 64, 96, 128, 160) if D <= dp)


def rope_tables(n, D):
    """cos / sin f32 [n, D/2] of the ESM-2 rotary embedding, positions 0 .. n - 1."""
    inv = 1.0 / (10000 ** (torch.arange(0, D, 2, dtype=F32) / D))
    fr = torch.arange(n, dtype=F32)[:, None] * inv[None]
    return fr.cos().contiguous(), fr.sin().contiguous()


def _rot_half(t):
    h = t.shape[-1] // 2
    return torch.cat([-t[..., h:], t[..., :h]], -1)


def _rot_half_t(t):
    h = t.shape[-1] // 2
    return torch.cat([t[..., h:], -t[..., :h]], -1)


def _round_bf16(t):
    return t.to(BF).to(t.dtype)


def _valid_keys(kmask, n, mutant):
    valid = torch.ones(n, dtype=torch.bool) if kmask is None else kmask.bool().clone()
    if mutant == "hole":
        for j in range(1, n - 1):
            if not valid[j] and valid[j - 1] and valid[j + 1]:
                valid[j] = True
                break
        else:
            if n > 1 and not valid[0] and valid[1]:
                valid[0] = True
    if mutant == "subblock":
        for j in range(0, n - 63, 64):
            if not valid[j:j + 64].any():
                valid[j:j + 64] = True
                break
    return valid


def _sequence(case, inp, row0, n, kmask, Lstride, dt, rnd, mutant, out_given, exact_delta):
    """One sequence (packed rows [row0, row0 + n)), every head at once -> out [n, H*D], lse / delta [H, n], dqkv [n, 3*H*D]."""
    H, D, scale = case.H, case.D, case.scale
    x = inp.qkv[row0:row0 + n].to(dt).view(n, 3, H, D).permute(1, 2, 0, 3)          # 3, H, n, D
    q, k, v = x[0], x[1], x[2]
    dO = inp.dout[row0:row0 + n].to(dt).view(n, H, D).permute(1, 0, 2)               # H, n, D
    cosf = sinf = cosq = sinq = None
    if case.rope:
        pos0 = row0 if mutant == "rope_packed" else 0          # the query rows' first position (the keys' is 0)
        cos, sin = rope_tables(pos0 + n, D)
        cosf, sinf = torch.cat([cos, cos], -1).to(dt), torch.cat([sin, sin], -1).to(dt)
        cosq, sinq, cosf, sinf = cosf[pos0:], sinf[pos0:], cosf[:n], sinf[:n]
        q, k = rnd(q * cosq + _rot_half(q) * sinq), rnd(k * cosf + _rot_half(k) * sinf)
    s = q @ k.transpose(-1, -2)
    if mutant == "pad":
        s = s + (padded_dim(D) - D) * (torch.arange(n) % 3).to(dt)[None, None, :]   # q padding 1, k padding (key mod 3)
    valid = _valid_keys(kmask, n, mutant)
    t = (s * scale).masked_fill(~valid[None, None, :], float("-inf"))
    m = t.max(-1).values
    dead = m == float("-inf")
    p_un = torch.exp(t - torch.where(dead, torch.zeros_like(m), m)[..., None])       # masked key: exp(-inf) = 0
    mult_f = mult_b = None
    if case.p > 0:
        qrow = torch.arange(n, dtype=torch.int64) + (0 if mutant == "row_local" else row0)
        key = torch.arange(n, dtype=torch.int64)
        if mutant in ("key64", "key128", "key192"):
            key = key + (key >= int(mutant[3:])).to(torch.int64)
        stride = n if mutant == "stride_len" else Lstride
        idx = ((qrow[None, :, None] * H + torch.arange(H, dtype=torch.int64)[:, None, None]) * stride + key[None, None, :])
        mult_f = drop_mult(case.p, case.seed, idx).to(dt)
        mult_b = torch.ones_like(mult_f) if mutant == "bwd_nodrop" else mult_f
    pd = p_un if mult_f is None else p_un * mult_f
    l = (pd if mutant == "norm_dropped" else p_un).sum(-1)
    lse = torch.where(dead, m, m + torch.log(torch.where(dead, torch.ones_like(l), l)))
    o = (rnd(pd) @ v) / torch.where(l > 0, l, torch.ones_like(l))[..., None]
    out = rnd(o)
    # ---- backward
    o_st = out if out_given is None else out_given[row0:row0 + n].to(dt).view(n, H, D).permute(1, 0, 2)
    delta = (dO * (o if mutant == "delta64" else o_st)).sum(-1)
    dl = (dO * o).sum(-1) if exact_delta else delta
    P = torch.exp(t - torch.where(dead, torch.full_like(lse, float("inf")), lse)[..., None])
    dP = dO @ v.transpose(-1, -2)
    if mult_b is not None:
        dP = dP * mult_b
    dS = rnd(P * (dP - dl[..., None]))
    Pd = rnd(P if mult_b is None else P * mult_b)
    dv = Pd.transpose(-1, -2) @ dO
    dq = (dS @ k) * scale
    dk = (dS.transpose(-1, -2) @ q) * scale
    if case.rope:
        dq, dk = dq * cosq + _rot_half_t(dq) * sinq, dk * cosf + _rot_half_t(dk) * sinf
    dqkv = rnd(torch.stack([dq, dk, dv], 0)).permute(2, 0, 1, 3).reshape(n, 3 * H * D)
    return out.permute(1, 0, 2).reshape(n, H * D), lse, delta, dqkv


def sequences(case, inp):
    """[(first packed row, length, key mask or None)] and the dropout index stride."""
    if case.lens is not None:
        rows, r = [], 0
        for n in case.lens:
            rows.append((r, n, None))
            r += n
        return rows, max(case.lens)
    mask = inp.mask
    return [(b * case.L, case.L, None if mask is None else mask[b]) for b in range(case.B)], case.L


def _run(case, dt, rnd, mutant=None, out=None, exact_delta=False, inp=None):
    inp = inputs(case) if inp is None else inp
    seqs, Lstride = sequences(case, inp)
    parts = [_sequence(case, inp, r0, n, km, Lstride, dt, rnd, mutant, out, exact_delta) for r0, n, km in seqs]
    res = SimpleNamespace(out=torch.cat([p[0] for p in parts], 0), dqkv=torch.cat([p[3] for p in parts], 0))
    if case.lens is not None:                                   # packed statistics: [H, T]
        res.lse, res.delta = torch.cat([p[1] for p in parts], 1), torch.cat([p[2] for p in parts], 1)
    else:                                                       # padded: [B, H, L]
        res.lse, res.delta = torch.stack([p[1] for p in parts], 0), torch.stack([p[2] for p in parts], 0)
    return res


def reference(case, out=None, inp=None):
    """f64, nothing rounded.  out: the stored bf16 `out` the backward under test consumes (delta = rowsum(dO * out))."""
    return _run(case, F64, lambda t: t, None, out, True, inp)


def restate_bf16(case, out=None, mutant=None, inp=None):
    assert mutant is None or mutant in MUTANTS, mutant
    return _run(case, F32, _round_bf16, mutant, out, False, inp)


def split_dqkv(case, dqkv):
    """dq, dk, dv [rows, H*D] of a dqkv [rows, 3*H*D]."""
    HD = case.H * case.D
    return dqkv[:, :HD], dqkv[:, HD:2 * HD], dqkv[:, 2 * HD:]


# ------------------------------------------------------------------------------------------------ the tolerance rule
def deviation(name, got, r64, restated, floor):
    """(ok, kernel deviation, bound) of the rule in the module docstring; infinities must sit where the reference's do."""
    got, r64, restated = (torch.as_tensor(t).detach().double().cpu() for t in (got, r64, restated))
    assert got.shape == r64.shape == restated.shape, (name, got.shape, r64.shape, restated.shape)
    fin = torch.isfinite(r64)
    same_inf = bool(torch.equal(got[~fin], r64[~fin])) and bool(torch.isfinite(got[fin]).all())
    assert torch.equal(restated[~fin], r64[~fin]) and torch.isfinite(restated[fin]).all(), name
    if not same_inf or not fin.any():
        print(f"{name}: non-finite entries {'agree' if same_inf else 'DIFFER'}")
        return same_inf, float("inf") if not same_inf else 0.0, 0.0
    dev_k = float((got[fin] - r64[fin]).abs().max())
    dev_r = float((restated[fin] - r64[fin]).abs().max())
    mag = float(r64[fin].abs().max())
    bound = max(8 * dev_r, floor * mag)
    print(f"{name}: kernel {dev_k:.3e}  bf16 restatement {dev_r:.3e}  magnitude {mag:.3e}  bound {bound:.3e}  "
          f"ratio {dev_k / bound if bound else float('inf'):.3f}")
    return dev_k <= bound, dev_k, bound


def check(name, got, r64, restated, floor):
    ok, dev_k, bound = deviation(name, got, r64, restated, floor)
    assert ok, (name, dev_k, bound)
    return dev_k / bound if bound else 0.0


def outputs(case, res):
    """(name, tensor, floor) of every compared output of a result (dq, dk, dv: one max norm each)."""
    dq, dk, dv = split_dqkv(case, res.dqkv)
    return [("out", res.out, FLOOR_BF16), ("lse", res.lse, FLOOR_F32), ("delta", res.delta, FLOOR_F32),
            ("dq", dq, FLOOR_BF16), ("dk", dk, FLOOR_BF16), ("dv", dv, FLOOR_BF16)]


def check_all(case, got, r64, restated, tag=""):
    """`check` on every output -> the worst deviation / bound ratio."""
    return max(check(f"{case.name}{tag} {nm}", g, r, s, fl) for (nm, g, fl), (_, r, _), (_, s, _) in
               zip(outputs(case, got), outputs(case, r64), outputs(case, restated)))


def rejected(case, got, r64, restated, tag=""):
    """names of the outputs on which `check` rejects `got`."""
    return [nm for (nm, g, fl), (_, r, _), (_, s, _) in zip(outputs(case, got), outputs(case, r64), outputs(case, restated))
            if not deviation(f"{case.name}{tag} {nm}", g, r, s, fl)[0]]


# ------------------------------------------------------------------------------------------------ the cases
def hole_mask(L):
    """[4, L] of group 4: b0 all valid; b1 single holes at 0, 63, 64, 127, 128, L - 1 and keys [64, 128) all masked; b2 keys
    [0, 128) masked (the running maximum starts dead and comes alive); b3 no valid key."""
    m = torch.ones(4, L, dtype=torch.uint8)
    m[1, [0, 63, 127, 128, L - 1]] = 0
    m[1, 64:128] = 0
    m[2, :128] = 0
    m[3] = 0
    return m


def prefix_mask(L, lens):
    return (torch.arange(L)[None] < torch.tensor(lens)[:, None]).to(torch.uint8)


def _case(name, group, D, mutants, *, B=2, L=200, H=2, p=0.0, mask="prefix", rope=None, lens=None, probe=False, qmul=1.0):
    """rope: None, "kernel" (tables handed to the kernels), "prerot" (q / k rotated in place first, backward prerotated).
    mask: None, "prefix" ([L, L - 63, ...]) or "holes".  lens: packed layout.  qmul: multiplier on the random q."""
    assert all(m in MUTANTS for m in mutants) and mutants, name
    assert p > 0 or not any(m in DROPOUT_MUTANTS for m in mutants), name
    if lens is not None:
        B, L = len(lens), max(lens)
    return SimpleNamespace(name=name, group=group, B=B, L=L, H=H, D=D, p=p, seed=0x5eed0000 + 977 * D + group,
                           mask=mask if lens is None else None, rope=rope, lens=lens, probe=probe, qmul=qmul,
                           scale=float(torch.tensor(D ** -0.5, dtype=F32)), mutants=tuple(mutants))   # the f32 the kernels get


def _pad_mut(D):
    return ["pad"] if D % 32 else []


DROP = [*sorted(DROPOUT_MUTANTS, key=list(MUTANTS).index), "delta64"]
PACKED_LENS = [200, 70, 1, 129]
CASES = []
# 1: dropout, padded layout (general kernels, DROP = true)
for _D, _p in [(8, 0.1), (24, 0.1), (40, 0.1), (64, 0.1), (96, 0.1), (160, 0.1), (96, 0.5)]:
    CASES.append(_case(f"drop_D{_D}_p{_p}", 1, _D, DROP + _pad_mut(_D), H=3 if _D == 24 else 2, p=_p))
CASES.append(_case("drop_D32_p0.1_nomask", 1, 32, DROP, p=0.1, mask=None))
# 2: dropout, packed layout
for _D in (32, 96):
    CASES.append(_case(f"drop_packed_D{_D}", 2, _D, DROP + ["stride_len", "row_local"], lens=PACKED_LENS, p=0.1))
# 3: exact dropout probe (delta64 does not apply: out is exact in bf16)
for _D in (32, 96):
    CASES.append(_case(f"probe_D{_D}", 3, _D, DROP[:5], L=256, p=0.5, mask=None, probe=True))
# 4: masks with holes and an empty sequence
for _D in (16, 24, 32):
    CASES.append(_case(f"holes_D{_D}_prerot", 4, _D, ["hole", "subblock", "delta64"] + _pad_mut(_D), B=4, H=3,
                       mask="holes", rope="prerot"))
    CASES.append(_case(f"holes_D{_D}", 4, _D, ["hole", "subblock", "delta64"] + _pad_mut(_D), B=4, H=3, mask="holes"))
CASES.append(_case("holes_D96", 4, 96, ["hole", "subblock", "delta64"], B=4, mask="holes"))
for _D in (64, 128):
    CASES.append(_case(f"holes_D{_D}_rope", 4, _D, ["hole", "subblock", "delta64"], B=4, mask="holes", rope="kernel"))
for _D in (160, 40):
    CASES.append(_case(f"holes_D{_D}", 4, _D, ["hole", "subblock", "delta64"] + _pad_mut(_D), B=4, mask="holes"))
# 5: run-time head dims
for _D in (8, 40, 56, 72, 88, 104, 120, 136, 152):
    CASES.append(_case(f"runtime_D{_D}", 5, _D, ["pad", "delta64"], H=3))
# 6: packed RoPE positions
CASES.append(_case("rope_packed_D64", 6, 64, ["rope_packed", "delta64"], lens=[200, 70, 129], rope="kernel"))
CASES.append(_case("rope_packed_D24", 6, 24, ["rope_packed", "delta64", "pad"], lens=[200, 70, 129], H=3, rope="prerot"))
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    case = CASE_BY_NAME[name]
    g = torch.Generator().manual_seed(case.seed)
    T = sum(case.lens) if case.lens is not None else case.B * case.L
    H, D = case.H, case.D
    qkv = torch.randn(T, 3, H, D, generator=g, dtype=F32)
    dout = torch.randn(T, H * D, generator=g, dtype=F32)
    if case.probe:
        # q = 0: every score 0, P = 1 / L; V[j, d] = bit (d mod 8) of j, dO in {0, 1}: every product and every sum of
        # at most 256 of them is exact in bf16 and f32
        qkv[:, 0] = 0
        j = torch.arange(case.L).repeat(case.B)
        bits = ((j[:, None] >> (torch.arange(D) % 8)[None, :]) & 1).to(F32)
        qkv[:, 2] = bits[:, None, :]
        dout = (torch.rand(T, H * D, generator=g) < 0.5).to(F32)
    qkv[:, 0] *= case.qmul
    mask = None
    if case.mask == "prefix":
        mask = prefix_mask(case.L, [case.L - 63 * b for b in range(case.B)])
    elif case.mask == "holes":
        mask = hole_mask(case.L)
    return SimpleNamespace(qkv=qkv.reshape(T, 3 * H * D).to(BF), dout=dout.to(BF), mask=mask)


def inputs(case):
    """qkv bf16 [T, 3*H*D], dout bf16 [T, H*D], mask uint8 [B, L] or None - from a seeded CPU generator, cached, read-only."""
    return _inputs(case.name)


def probe_expectation(case):
    """What the exact probe must give bit for bit: out [T, H*D], dv [T, H*D] (f64 holding bf16-exact values)."""
    inp = inputs(case)
    B, L, H, D = case.B, case.L, case.H, case.D
    i = torch.arange(B * L, dtype=torch.int64)
    idx = (i[None, :, None] * H + torch.arange(H)[:, None, None]) * L + torch.arange(L)[None, None, :]
    keep = (drop_mult(case.p, case.seed, idx) > 0).double().view(H, B, L, L)               # h, b, query, key
    v = inp.qkv.double().view(B, L, 3, H, D)[:, :, 2].permute(2, 0, 1, 3)                   # h, b, key, d
    dO = inp.dout.double().view(B, L, H, D).permute(2, 0, 1, 3)                             # h, b, query, d
    out = (keep @ v) * 2 / L
    dv = (keep.transpose(-1, -2) @ dO) * 2 / L
    return (out.permute(1, 2, 0, 3).reshape(B * L, H * D), dv.permute(1, 2, 0, 3).reshape(B * L, H * D))


# ------------------------------------------------------------------------------------------------ one reference per case
def stored_delta(case, out, dt):
    """rowsum(dO * out) of a stored bf16 `out` in the layout of the statistics ([B, H, L], packed [H, T])."""
    H, D = case.H, case.D
    d = (inputs(case).dout.to(dt) * out.detach().cpu().to(dt)).view(-1, H, D).sum(-1)              # T, H
    return d.t().contiguous() if case.lens is not None else d.view(case.B, case.L, H).permute(0, 2, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _cached(name):
    case = CASE_BY_NAME[name]
    return reference(case), restate_bf16(case)


def yardsticks(case, out):
    """(f64 reference, bf16 restatement) of a table case, computed once per case and shared, with `delta` taken from
    the stored bf16 `out` that the backward under test was handed."""
    r64, st = _cached(case.name)
    return (SimpleNamespace(out=r64.out, lse=r64.lse, dqkv=r64.dqkv, delta=stored_delta(case, out, F64)),
            SimpleNamespace(out=st.out, lse=st.lse, dqkv=st.dqkv, delta=stored_delta(case, out, F32)))
