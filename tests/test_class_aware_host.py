"""CPU: the host side of the class-aware InfoNCE (loss.clip_loss with class_ids / same_class / label_smoothing).

The HIP kernels cannot run here: tests/class_aware_ref.py stands in for the two class-aware ops and tests/ops_emulator.py
for the plain ones, as in tests/test_distributed_gloo.py.  Under test: argument validation, the dispatch (the default
call runs exactly the plain ops), and the world-2 bookkeeping (ids all-gathered, counts gathered with the LSE vectors,
the column direction's key counts): distributed loss and gradients == the single-process f64 definition.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import class_aware_ref as R  # noqa: E402
from host_harness import (clip_loss_cases, install as _install, run_ranks, spy_gathers, trap_calls,  # noqa: E402
                          unit as _unit)


def _reference(a, b, s, ids, same_class, eps, symmetric):
    ad, bd = a.double().requires_grad_(True), b.double().requires_grad_(True)
    sd = torch.tensor(float(s), dtype=torch.float64, requires_grad=True)
    S = sd * (ad @ bd.t())
    w = (0.5, 0.5) if symmetric else (1.0, 0.0)
    L = R.loss_from_logits(S, a.shape[0], ids, same_class, eps, *w)
    return (L.item(),) + torch.autograd.grad(L, (ad, bd, sd))


# ---------------------------------------------------------------------------------------------- validation
def test_argument_validation():
    from clip_dplm_amd.loss import clip_loss
    a, b = _unit(8, 16, 1), _unit(8, 16, 2)
    s = torch.tensor(14.0)
    ids = torch.arange(8)
    bad = [dict(class_ids=ids.float()), dict(class_ids=ids > 3), dict(class_ids=ids[:7]), dict(class_ids=ids.view(2, 4)),
           dict(class_ids=[0] * 8), dict(class_ids=ids.to("meta")), dict(same_class="hard_negative"),
           dict(same_class=None), dict(label_smoothing=1.0), dict(label_smoothing=-0.1), dict(label_smoothing="0.1"),
           dict(label_smoothing=float("nan"))]
    for kw in bad:
        with pytest.raises(ValueError):
            clip_loss(a, b, s, **kw)
    # the kernels read f32 embeddings: bf16 / f16 / f64 (autocast, a .half() model) are refused, the cache's too
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        for kw in (dict(class_ids=ids), dict(label_smoothing=0.1)):
            with pytest.raises(ValueError, match="float32"):
                clip_loss(a.to(dt), b.to(dt), s, **kw)
            with pytest.raises(ValueError, match="float32"):
                clip_loss(a, b.to(dt), s, **kw)
            with pytest.raises(ValueError, match="float32"):
                clip_loss(a, b, s, cache=_unit(5, 16, 7).to(dt), **kw)
    with pytest.raises(ValueError):
        clip_loss(a, b, s, cache=_unit(5, 12, 7), class_ids=ids)
    wide_a, wide_b = _unit(8, 516, 3), _unit(8, 516, 4)
    for kw in (dict(class_ids=ids), dict(label_smoothing=0.1)):
        with pytest.raises(ValueError, match="P <= 512"):
            clip_loss(wide_a, wide_b, s, **kw)


def test_class_aware_ops_check_their_operands():
    """ops.simce_lse_cls / simce_grad_cls refuse operands the kernels would misread (before touching the device)."""
    from clip_dplm_amd import ops
    x, y, s = _unit(8, 16, 1), _unit(12, 16, 2), torch.tensor([14.0])
    ids_x, ids_y = torch.arange(8), torch.arange(12)
    v8, v12 = torch.zeros(8), torch.zeros(12)
    bad_lse = [dict(x=x.bfloat16()), dict(y=y.half()), dict(x=_unit(16, 8, 3).t()), dict(cache=_unit(4, 16, 4).bfloat16()),
               dict(cache=_unit(4, 12, 4)), dict(scale=s.double()), dict(cls_x=ids_x.int()), dict(cls_x=ids_x[:7]),
               dict(cls_y=ids_y.float()), dict(cls_x=None), dict(same_class="hard_negative"), dict(eps=1.0)]
    for kw in bad_lse:
        args = dict(x=x, y=y, scale=s, cls_x=ids_x, cls_y=ids_y, same_class="mask", eps=0.1, cache=None)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.simce_lse_cls(**args)
    good = dict(x=x, y=y, scale=s, lse_x=v8, lse_y=v12, cnt_x=v8, cnt_y=v12, w_row=0.5, w_col=0.5, inv_bg=1 / 12,
                nkeys_y=12, cls_x=ids_x, cls_y=ids_y)
    bad_grad = [dict(x=x.bfloat16()), dict(lse_x=v12), dict(lse_y=v12.double()), dict(cnt_x=v8.long()),
                dict(cnt_y=v8), dict(cls_y=ids_y[:11]), dict(upstream=torch.ones(2))]
    for kw in bad_grad:
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.simce_grad_cls(**args)
    # valid operands get past the checks: the CPU tensors are then refused for want of a device
    with pytest.raises(Exception) as e:
        ops.simce_grad_cls(**good)
    assert not isinstance(e.value, ValueError)


def test_default_call_never_reaches_class_aware_ops(monkeypatch):
    _install(monkeypatch.setattr)
    from clip_dplm_amd.loss import clip_loss
    calls = trap_calls(monkeypatch.setattr, ("simce_lse_cls", "simce_grad_cls"))
    a0, b0 = _unit(24, 16, 5), _unit(24, 16, 6)
    for kw in (dict(), dict(same_class="positive"), dict(class_ids=None, label_smoothing=0.0)):
        a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        clip_loss(a, b, torch.tensor(14.0, requires_grad=True), **kw).backward()
    assert calls == []
    # ... and a class-aware call does, with the definition's value and gradients
    ids = torch.tensor([0, 1, 2] * 8)
    for same_class, eps, symmetric in (("mask", 0.1, True), ("positive", 0.0, True), ("positive", 0.1, False)):
        a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        s = torch.tensor(14.0, requires_grad=True)
        loss = clip_loss(a, b, s, symmetric=symmetric, class_ids=ids, same_class=same_class, label_smoothing=eps)
        loss.backward()
        L, ga, gb, gs = _reference(a0, b0, 14.0, ids, same_class, eps, symmetric)
        assert abs(loss.item() - L) < 1e-5
        assert torch.allclose(a.grad.double(), ga, atol=1e-6) and torch.allclose(b.grad.double(), gb, atol=1e-6)
        assert abs(s.grad.item() - gs.item()) < 1e-5
    assert "simce_lse_cls" in calls and "simce_grad_cls" in calls


# ---------------------------------------------------------------------------------------------- gloo, world 2
CASES = (("mask", 0.1, True), ("positive", 0.0, True), ("positive", 0.1, False))


def _rank_body(rank, world):
    from clip_dplm_amd import loss as L
    cases = [(True, False, dict(same_class=c, label_smoothing=eps, symmetric=sym)) for c, eps, sym in CASES]
    return clip_loss_cases(cases, spy_gathers(L), rank, world)


@pytest.mark.timeout(300)
def test_world2_class_aware_matches_single_process():
    world, Bl, P = 2, 12, 16
    res = run_ranks(_rank_body, world)
    a, b = _unit(world * Bl, P, 1), _unit(world * Bl, P, 2)
    ids = torch.arange(world * Bl) % 5
    for k, (same_class, eps, symmetric) in enumerate(CASES):
        L, ga, gb, gs = _reference(a, b, 14.2849, ids, same_class, eps, symmetric)
        plain = _reference(a, b, 14.2849, None, same_class, 0.0, symmetric)[0]
        assert abs(L - plain) > 1e-3                                   # the ids (of both ranks) matter here
        ds = 0.0
        for r in range(world):
            loss, da, db, dsr, gathered = res[r][k]
            assert [dt for dt, _ in gathered] == [torch.float32, torch.int64, torch.float32]   # embeds, ids, LSE + counts
            assert abs(loss - L) < 1e-5, (k, r, loss, L)                               # the global loss on every rank
            sl = slice(r * Bl, (r + 1) * Bl)
            assert torch.allclose(da.double(), ga[sl], atol=1e-6), (k, r)
            assert torch.allclose(db.double(), gb[sl], atol=1e-6), (k, r)
            ds += dsr.item()
        assert abs(ds - gs.item()) < 1e-5                              # summed over ranks by the optimiser
