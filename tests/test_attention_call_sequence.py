"""CPU: the sequence of GEMM and attention calls behind one forward + backward of a 2-layer encoder, path by path.

tests/ops_emulator.py stands in for the kernels; gemm_nt, gemm_wgrad, the six attention wrappers and rope_qk_ are each
wrapped to record, per call, the name, the tensor shapes and the arguments that select a path: the RoPE operand, the
pair-interleaved flag, `prerotated`, the dropout pair, the key mask, cu_seqlens.  The expected lists are written out
below from the shapes and the mode table of DESIGN.md §3 alone: however the encoders arrive at a path, the launches and
their arguments stay these.  The last two tests change a module switch between a forward and its backward: the backward
has to follow what the forward did.
"""
import inspect
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import ops_emulator  # noqa: E402

NL, F = 2, 128
SWITCHES = dict(PREROTATE_QK=True, ROPE_IN_QKV_EPILOGUE=True, ROPE_INTERLEAVED=True)
# what is recorded of each call (the emulator's own extra parameters are left out)
KEYS = {
    "gemm_nt": ("a", "b", "bias", "rope", "rope_interleaved", "dropout"),
    "gemm_wgrad": ("dy", "x", "il"),
    "rope_qk_": ("qkv", "B", "L", "H", "D", "rope"),
    "attn_fwd": ("qkv", "B", "L", "H", "D", "key_mask", "rope", "q_scale", "dropout"),
    "attn_fwd_rot_": ("qkv", "B", "L", "H", "D", "rope", "key_mask", "q_scale"),
    "attn_bwd": ("qkv", "out", "dout", "lse", "B", "L", "H", "D", "key_mask", "rope", "q_scale", "prerotated", "dropout"),
    "attn_varlen_fwd": ("qkv", "cu_seqlens", "max_len", "H", "D", "rope", "q_scale", "dropout"),
    "attn_varlen_fwd_rot_": ("qkv", "cu_seqlens", "max_len", "H", "D", "rope", "q_scale"),
    "attn_varlen_bwd": ("qkv", "out", "dout", "lse", "cu_seqlens", "max_len", "H", "D", "rope", "q_scale", "dropout",
                        "prerotated"),
}


def _describe(v):
    """A tensor as its shape, a tuple (a RoPE operand) item by item, anything else as it is."""
    if torch.is_tensor(v):
        return tuple(v.shape)
    if isinstance(v, (tuple, list)):
        return tuple(_describe(u) for u in v)
    return v


def _record(monkeypatch, log):
    """Install the emulator and wrap the recorded ops; a dropout pair (p, seed) is recorded as (p, n) with n counting the
    distinct seeds in the order they first appear."""
    from clip_dplm_amd import ops
    ops_emulator.install(monkeypatch)
    seeds = {}

    def wrap(name, fn):
        sig = inspect.signature(fn)

        def f(*args, **kw):
            bound = sig.bind(*args, **kw)
            bound.apply_defaults()
            rec = {k: _describe(bound.arguments[k]) for k in KEYS[name]}
            if rec.get("dropout") is not None:
                p, seed = rec["dropout"]
                rec["dropout"] = (p, seeds.setdefault(seed, len(seeds)))
            log.append((name, rec))
            return fn(*args, **kw)
        return f
    for n in KEYS:
        monkeypatch.setattr(ops, n, wrap(n, getattr(ops, n)))


def _switches(monkeypatch, **kw):
    from clip_dplm_amd import encoders
    for k, v in dict(SWITCHES, **kw).items():
        monkeypatch.setattr(encoders, k, v)


def _gemm(a, b, bias=True, rope=None, il=False, dropout=None):
    return ("gemm_nt", dict(a=a, b=b, bias=(b[0],) if bias else None, rope=rope, rope_interleaved=il, dropout=dropout))


def _wgrad(dy, x, il=(0, 0)):
    return ("gemm_wgrad", dict(dy=dy, x=x, il=il))


def _attention(geo, rot, rope_fwd, rope_bwd, prerotated, qs, drop=None):
    """The forward and the backward attention call of one layer.  geo: ("padded", B, L, H, D) or ("packed", lengths, H, D);
    rot: the forward that rotates q / k in place; rope_fwd / rope_bwd: whether each call is handed the RoPE tables."""
    H, D = geo[-2:]
    if geo[0] == "padded":
        _, B, L, _, _ = geo
        T, tables = B * L, ((L, D // 2), (L, D // 2))
        com = dict(qkv=(T, 3 * H * D), B=B, L=L, H=H, D=D, key_mask=(B, L), q_scale=qs)
        if rot:
            fwd = ("attn_fwd_rot_", dict(com, rope=tables))
        else:
            fwd = ("attn_fwd", dict(com, rope=tables if rope_fwd else None, dropout=drop))
        bwd = ("attn_bwd", dict(com, out=(T, H * D), dout=(T, H * D), lse=(B, H, L), rope=tables if rope_bwd else None,
                                prerotated=prerotated, dropout=drop))
        return fwd, bwd
    lengths = geo[1]
    T, mx = sum(lengths), max(lengths)
    tables = ((mx, D // 2), (mx, D // 2))
    com = dict(qkv=(T, 3 * H * D), cu_seqlens=(len(lengths) + 1,), max_len=mx, H=H, D=D, q_scale=qs)
    if rot:
        fwd = ("attn_varlen_fwd_rot_", dict(com, rope=tables))
    else:
        fwd = ("attn_varlen_fwd", dict(com, rope=tables if rope_fwd else None, dropout=drop))
    bwd = ("attn_varlen_bwd", dict(com, out=(T, H * D), dout=(T, H * D), lse=(H, T), rope=tables if rope_bwd else None,
                                   prerotated=prerotated, dropout=drop))
    return fwd, bwd


# mode -> (RoPE in the qkv GEMM's epilogue, pair-interleaved, forward rotates in place, forward gets the tables, prerotated)
ESM_MODES = {
    "epilogue": (True, False, False, False, 1),
    "interleaved": (True, True, False, False, 2),
    "in_place": (False, False, True, True, 1),
    "staging": (False, False, False, True, 0),
}


def _esm_expected(mode, geo):
    epi, il, rot, rope_fwd, pre = ESM_MODES[mode]
    H, D = geo[-2:]
    d = H * D
    T, L = (geo[1] * geo[2], geo[2]) if geo[0] == "padded" else (sum(geo[1]), max(geo[1]))
    a_fwd, a_bwd = _attention(geo, rot, rope_fwd, True, pre, D ** -0.5)
    X, Q, U = (T, d), (T, 3 * d), (T, F)
    fwd = [_gemm(X, (3 * d, d), rope=((L, D // 2), (L, D // 2), L, D, 2 * d) if epi else None, il=il), a_fwd,
           _gemm(X, (d, d)), _gemm(X, (F, d)), _gemm(U, (d, F))]
    bwd = [_gemm(X, (F, d), bias=False), _wgrad(X, U), _gemm(U, (d, F), bias=False), _wgrad(U, X),
           _gemm(X, (d, d), bias=False), _wgrad(X, X), a_bwd,
           _gemm(Q, (d, 3 * d), bias=False), _wgrad(Q, X, il=(D, 2 * d) if il else (0, 0))]
    return fwd * NL + bwd * NL


def _post_expected(geo, E, p_drop):
    H, D = geo[-2:]
    T = geo[1] * geo[2] if geo[0] == "padded" else sum(geo[1])
    X, Q, U = (T, E), (T, 3 * E), (T, F)
    fwd, bwd = [], []
    for i in range(NL):
        # the four dropout sites of layer i in the order their seeds first reach a recorded call
        da, d1, df, d2 = [(p_drop, 4 * i + j) for j in range(4)] if p_drop else [None] * 4
        a_fwd, a_bwd = _attention(geo, False, False, False, 0, float(D) ** -0.5, da)
        fwd += [_gemm(X, (3 * E, E)), a_fwd, _gemm(X, (E, E), dropout=d1), _gemm(X, (F, E), dropout=df),
                _gemm(U, (E, F), dropout=d2)]
        bwd = [_gemm(X, (F, E), bias=False, dropout=df), _wgrad(X, U), _gemm(U, (E, F), bias=False), _wgrad(U, X),
               _gemm(X, (E, E), bias=False), _wgrad(X, X), a_bwd, _gemm(Q, (E, 3 * E), bias=False), _wgrad(Q, X)] + bwd
    return fwd + bwd


def _esm(d, H):
    import clip_dplm_amd as K
    torch.manual_seed(0)
    return K.ESM2Encoder(num_layers=NL, hidden_size=d, num_heads=H, intermediate_size=F).eval()


def _esm_run(enc, lengths, packed, before_backward=None):
    """One forward + backward; padded: B = len(lengths) rows of max(lengths) positions with a ragged mask."""
    g = torch.Generator().manual_seed(7)
    if packed:
        cu = torch.tensor([0] + list(lengths), dtype=torch.int32).cumsum(0).to(torch.int32)
        y = enc.forward_packed(torch.randint(4, 24, (sum(lengths),), generator=g), cu, max(lengths))
    else:
        B, L = len(lengths), max(lengths)
        mask = (torch.arange(L)[None] < torch.tensor(lengths)[:, None]).long()
        y = enc(torch.randint(4, 24, (B, L), generator=g), attention_mask=mask)
    if before_backward is not None:
        before_backward()
    (y * torch.randn(y.shape, generator=g)).sum().backward()
    return {n: p.grad.clone() for n, p in enc.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("d,H,switches,mode", [
    (64, 2, dict(), "epilogue"),
    (64, 2, dict(ROPE_IN_QKV_EPILOGUE=False), "in_place"),
    (64, 2, dict(PREROTATE_QK=False), "staging"),
    (96, 4, dict(), "interleaved"),
    (96, 4, dict(ROPE_INTERLEAVED=False), "in_place"),
])
def test_esm_padded(monkeypatch, d, H, switches, mode):
    log = []
    _record(monkeypatch, log)
    _switches(monkeypatch, **switches)
    _esm_run(_esm(d, H), (8, 5), packed=False)
    assert log == _esm_expected(mode, ("padded", 2, 8, H, d // H))


@pytest.mark.parametrize("lengths,mode", [((130, 5), "in_place"), ((9, 4), "staging")])
def test_esm_packed(monkeypatch, lengths, mode):
    log = []
    _record(monkeypatch, log)
    _switches(monkeypatch)
    _esm_run(_esm(64, 2), lengths, packed=True)
    assert log == _esm_expected(mode, ("packed", lengths, 2, 32))


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("packed", [False, True])
def test_post_ln(monkeypatch, packed, training):
    import clip_dplm_amd as K
    log = []
    _record(monkeypatch, log)
    _switches(monkeypatch)
    E, H, lengths = 64, 2, (8, 5)
    torch.manual_seed(0)
    enc = K.TransformerSeqEncoder(embed_dim=E, num_layers=NL, nhead=H, dim_feedforward=F, dropout=0.1).train(training)
    g = torch.Generator().manual_seed(7)
    if packed:
        x = torch.randn(sum(lengths), E, generator=g).requires_grad_(True)
        y = enc.forward_packed(x, torch.tensor([0, 8, 13], dtype=torch.int32), max(lengths))
        geo = ("packed", lengths, H, E // H)
    else:
        x = torch.randn(2, 8, E, generator=g).requires_grad_(True)
        y = enc(x, src_key_padding_mask=torch.arange(8)[None] >= torch.tensor(lengths)[:, None])
        geo = ("padded", 2, 8, H, E // H)
    y.sum().backward()
    assert log == _post_expected(geo, E, 0.1 if training else None)


@pytest.mark.parametrize("lengths,packed", [((8, 5), False), ((130, 5), True)])
def test_backward_follows_the_forward_when_a_switch_flips(monkeypatch, lengths, packed):
    """In-place rotation in the forward (D = 32 without the RoPE epilogue; packed whole-head shapes), PREROTATE_QK
    switched off before backward(): `qkv` holds rotated q / k whatever the switch says now, so every parameter gradient
    must equal the one of the same run without the flip, bit for bit."""
    from clip_dplm_amd import encoders
    ops_emulator.install(monkeypatch)
    _switches(monkeypatch, ROPE_IN_QKV_EPILOGUE=False)
    ref = _esm_run(_esm(64, 2), lengths, packed)
    got = _esm_run(_esm(64, 2), lengths, packed,
                   before_backward=lambda: monkeypatch.setattr(encoders, "PREROTATE_QK", False))
    assert ref and got.keys() == ref.keys()
    for n in ref:
        assert torch.equal(got[n], ref[n]), n
