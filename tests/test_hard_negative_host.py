"""CPU: the yardstick of the hard-negative-weighted InfoNCE and the host side of loss.clip_loss(hard_negative_beta=).

The reference project names the variant and its weight only, so there are no recorded values: tests/hard_negative_ref.py
(the yardstick of the GPU tests) is pinned here first - against an independent transcription of the paper's form with
the weights written out, against F.cross_entropy at beta = 0, and its closed-form gradient against autograd.  The HIP
kernels cannot run here: hard_negative_ref stands in for the two hard-negative ops and tests/ops_emulator.py for the
plain ones in the tests of the argument checks, the dispatch and the world-2 bookkeeping (ids all-gathered, coefficient
rows gathered once).
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import hard_negative_ref as R  # noqa: E402
from host_harness import (clip_loss_cases, install as _install, run_ranks, spy_gathers, trap_calls,  # noqa: E402
                          unit as _unit)

SCALE = 14.2849


def _case(Mx=48, Ny=56, Nc=12, P=24, off=5, classes=7, seed=0):
    """f64 logits of a 48 x 68 block with class ids and cache columns (label_offset 5)."""
    a, k = _unit(Mx, P, seed + 1, torch.float64), _unit(Ny + Nc, P, seed + 2, torch.float64)
    g = torch.Generator().manual_seed(seed + 3)
    cls_y = torch.randint(0, classes, (Ny,), generator=g)
    cls_x = cls_y[off:off + Mx].clone()
    return SCALE * (a @ k.t()), Ny, off, cls_x, cls_y


def _paper_loss(S, Ny, off, cls_x, cls_y, beta):
    """Independent transcription, row by row: Robinson et al. eq. (4) with tau_plus = 0, the weights written out:
    loss_i = -log( e^{pos} / (e^{pos} + sum_{j in Neg} w_j e^{S_ij}) ),  w_j = e^{beta S_ij} / mean_{Neg} e^{beta S_ik}."""
    out = []
    for i in range(S.shape[0]):
        l = off + i
        js = [j for j in range(S.shape[1])
              if j != l and not (cls_x is not None and j < Ny and int(cls_y[j]) == int(cls_x[i]))]
        if not js:
            out.append(S.new_zeros(()))
            continue
        s = S[i, js]
        imp = torch.exp(beta * s)
        w = imp / imp.mean()
        ng = (w * torch.exp(s)).sum()
        out.append(-torch.log(torch.exp(S[i, l]) / (torch.exp(S[i, l]) + ng)))
    return torch.stack(out)


# ---------------------------------------------------------------------------------------------- the yardstick
@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0, 2.0])
def test_ref_equals_papers_form(beta):
    S, Ny, off, cls_x, cls_y = _case()
    for cx, cy in ((cls_x, cls_y), (None, None)):
        got = R.stats(S, Ny, off, cx, cy, beta)["loss"]
        assert torch.allclose(got, _paper_loss(S, Ny, off, cx, cy, beta), rtol=0, atol=1e-12)


def test_ref_beta0_is_cross_entropy():
    S, Ny, off, _, _ = _case()
    lab = off + torch.arange(S.shape[0])
    st = R.stats(S, Ny, off, None, None, 0.0)
    assert torch.allclose(st["loss"], F.cross_entropy(S, lab, reduction="none"), rtol=0, atol=1e-12)
    assert torch.allclose(st["lse_h"], torch.logsumexp(S, 1), rtol=0, atol=1e-12)
    sq = S[:, :Ny][:, off:off + S.shape[0]]                                      # a square block, both directions
    ref = 0.5 * (F.cross_entropy(sq, torch.arange(sq.shape[0])) + F.cross_entropy(sq.t(), torch.arange(sq.shape[0])))
    assert abs(R.loss_from_logits(sq, sq.shape[0], None, 0.0, 0.5, 0.5).item() - ref.item()) < 1e-12


@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
def test_ref_closed_form_gradient_equals_autograd(beta):
    S0, Ny, off, cls_x, cls_y = _case()
    for cx, cy in ((cls_x, cls_y), (None, None)):
        S = S0.clone().requires_grad_(True)
        g_auto, = torch.autograd.grad(R.stats(S, Ny, off, cx, cy, beta)["loss"].sum(), S)
        g = R.direction_grad(S0, Ny, off, cx, cy, beta)
        assert (g - g_auto).abs().max().item() < 1e-14
        assert g.sum(1).abs().max().item() < 1e-13                               # each row's gradient sums to zero
        neg = R.stats(S0, Ny, off, cx, cy, beta)["neg"]
        diag = R.stats(S0, Ny, off, cx, cy, beta)["diag"]
        assert bool((g[~neg & ~diag] == 0).all())                                # masked keys: exactly zero


def test_ref_standins_give_autograd_of_global_loss():
    """The two stand-ins chained as loss.InfoNCEFn chains the hard-negative kernels: G of both directions, dX, dscale."""
    B, Nc, P, beta = 40, 9, 16, 0.5
    a, b, cache = _unit(B, P, 1, torch.float64), _unit(B, P, 2, torch.float64), _unit(Nc, P, 3, torch.float64)
    ids = torch.arange(B) % 6
    ad, bd = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    sd = torch.tensor(SCALE, dtype=torch.float64, requires_grad=True)
    L = R.loss_from_logits(sd * (ad @ torch.cat([bd, cache]).t()), B, ids, beta, 0.5, 0.5)
    ga, gb, gs = torch.autograd.grad(L, (ad, bd, sd))
    sc = torch.tensor([SCALE], dtype=torch.float64)
    _, _, cr = R.simce_lse_hard(a, b, sc, beta, ids, ids, cache=cache)
    _, _, cc = R.simce_lse_hard(b, a, sc, beta, ids, ids)
    da, dsa = R.simce_grad_hard(a, b, sc, beta, cr, cc, 0.5, 0.5, 1.0 / B, cls_x=ids, cls_y=ids, cache=cache)
    db, _ = R.simce_grad_hard(b, a, sc, beta, cc, cr, 0.5, 0.5, 1.0 / B, cls_x=ids, cls_y=ids)
    assert (da - ga).abs().max().item() < 1e-14 and (db - gb).abs().max().item() < 1e-14
    assert abs(dsa.sum().item() - gs.item()) < 1e-14


@pytest.mark.parametrize("beta", [0.5, 1.0, 2.0])
def test_ref_loss_is_at_least_the_plain_loss(beta):
    S, Ny, off, cls_x, cls_y = _case()
    for cx, cy in ((cls_x, cls_y), (None, None)):
        hard = R.stats(S, Ny, off, cx, cy, beta)["loss"]
        plain = R.stats(S, Ny, off, cx, cy, 0.0)["loss"]
        assert bool((hard >= plain - 1e-12).all()) and bool((hard > plain + 1e-6).any())


def test_ref_row_without_negatives():
    """All pairs of one class, no cache: Neg_i is empty; loss 0, gradient exactly zero and finite."""
    S0 = _case(Mx=12, Ny=12, Nc=0, off=0)[0]
    ids = torch.zeros(12, dtype=torch.int64)
    S = S0.clone().requires_grad_(True)
    st = R.stats(S, 12, 0, ids, ids, 0.5)
    assert bool((st["loss"] == 0).all()) and bool((st["logNg"] == float("-inf")).all())
    g, = torch.autograd.grad(st["loss"].sum(), S)
    assert bool((g == 0).all())
    assert bool((R.direction_grad(S0, 12, 0, ids, ids, 0.5) == 0).all())
    coef = R.coefficients(st, 0.5)
    assert bool((coef[0] == 0).all()) and bool((coef[1:] == float("-inf")).all())
    # one row with negatives next to rows without: only that row carries loss and gradient
    ids2 = ids.clone()
    ids2[3] = 9                                                    # the query's id only: its keys all differ from it
    S = S0.clone().requires_grad_(True)
    loss = R.stats(S, 12, 0, ids2, ids, 0.5)["loss"]
    g, = torch.autograd.grad(loss.sum(), S)
    assert bool(torch.isfinite(g).all()) and loss[3] > 0 and bool((loss[torch.arange(12) != 3] == 0).all())
    assert bool((g[torch.arange(12) != 3] == 0).all())


# ---------------------------------------------------------------------------------------------- validation
def test_argument_validation():
    from clip_dplm_amd.loss import clip_loss
    a, b = _unit(8, 16, 1), _unit(8, 16, 2)
    s = torch.tensor(14.0)
    ids = torch.arange(8)
    bad = [dict(hard_negative_beta=-0.5), dict(hard_negative_beta=True), dict(hard_negative_beta="0.5"),
           dict(hard_negative_beta=float("nan")), dict(hard_negative_beta=float("inf")), dict(hard_negative_beta=None),
           dict(hard_negative_beta=0.5, same_class="positive"),
           dict(hard_negative_beta=0.5, same_class="positive", class_ids=ids),
           dict(hard_negative_beta=0.5, label_smoothing=0.1),
           dict(hard_negative_beta=0.5, class_ids=ids.float()), dict(hard_negative_beta=0.5, class_ids=ids > 3),
           dict(hard_negative_beta=0.5, class_ids=ids[:7]), dict(hard_negative_beta=0.5, class_ids=ids.view(2, 4)),
           dict(hard_negative_beta=0.5, class_ids=ids.to("meta")),
           dict(hard_negative_beta=0.5, cache=_unit(5, 12, 7))]
    for kw in bad:
        with pytest.raises(ValueError):
            clip_loss(a, b, s, **kw)
    for dt in (torch.bfloat16, torch.float64):
        with pytest.raises(ValueError, match="float32"):
            clip_loss(a.to(dt), b.to(dt), s, hard_negative_beta=0.5)
        with pytest.raises(ValueError, match="float32"):
            clip_loss(a, b, s, cache=_unit(5, 16, 7).to(dt), hard_negative_beta=0.5)
    with pytest.raises(ValueError, match="P <= 512"):
        clip_loss(_unit(8, 514, 3), _unit(8, 514, 4), s, hard_negative_beta=0.5)
    with pytest.raises(ValueError, match="P <= 512"):
        clip_loss(_unit(8, 516, 3), _unit(8, 516, 4), s, hard_negative_beta=0.5)


def test_hard_negative_ops_check_their_operands():
    from clip_dplm_amd import ops
    x, y, s = _unit(8, 16, 1), _unit(12, 16, 2), torch.tensor([14.0])
    ids_x, ids_y = torch.arange(8), torch.arange(12)
    for kw in (dict(beta=-1.0), dict(beta=float("nan")), dict(beta=True), dict(x=x.bfloat16()), dict(cls_x=None),
               dict(cls_y=ids_y.int()), dict(cache=_unit(4, 12, 4)), dict(scale=s.double())):
        args = dict(x=x, y=y, scale=s, beta=0.5, cls_x=ids_x, cls_y=ids_y)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.simce_lse_hard(**args)
    good = dict(x=x, y=y, scale=s, beta=0.5, coef_x=torch.zeros(3, 8), coef_y=torch.zeros(3, 12), w_row=0.5, w_col=0.5,
                inv_bg=1 / 12, cls_x=ids_x, cls_y=ids_y)
    for kw in (dict(coef_x=torch.zeros(3, 12)), dict(coef_y=torch.zeros(12, 3)), dict(coef_x=torch.zeros(3, 8).double()),
               dict(beta=-0.5), dict(upstream=torch.ones(2)), dict(cls_y=ids_y[:11])):
        args = dict(good)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.simce_grad_hard(**args)
    # valid operands get past the checks: the host tensors are then refused for want of a device
    for call in (lambda: ops.simce_lse_hard(x, y, s, 0.5, ids_x, ids_y), lambda: ops.simce_grad_hard(**good)):
        with pytest.raises(Exception) as e:
            call()
        assert not isinstance(e.value, ValueError)


def test_config_hard_negative_beta():
    from clip_dplm_amd.configuration_hybrid_clip import HybridCLIPConfig
    sub = dict(rna_config={}, protein_config={}, diffmap_config={})
    assert HybridCLIPConfig(**sub).hard_negative_beta == 0.5                   # the reference's defaults: on, 0.5
    assert HybridCLIPConfig(use_hard_negatives=True, hard_negative_weight=1.0, **sub).hard_negative_beta == 1.0
    assert HybridCLIPConfig(use_hard_negatives=False, hard_negative_weight=1.0, **sub).hard_negative_beta == 0.0
    with pytest.raises(AttributeError):
        HybridCLIPConfig(**sub).hard_negative_beta = 1.0                       # read-only
    assert "hard_negative_beta" not in HybridCLIPConfig(**sub).to_dict()


# ---------------------------------------------------------------------------------------------- dispatch
def _reference(a, b, s, ids, beta, symmetric, cache=None):
    ad, bd = a.double().requires_grad_(True), b.double().requires_grad_(True)
    sd = torch.tensor(float(s), dtype=torch.float64, requires_grad=True)
    K = bd if cache is None else torch.cat([bd, cache.double()])
    w = (0.5, 0.5) if symmetric else (1.0, 0.0)
    L = R.loss_from_logits(sd * (ad @ K.t()), a.shape[0], ids, beta, *w)
    return (L.item(),) + torch.autograd.grad(L, (ad, bd, sd))


def test_beta0_never_reaches_hard_ops_and_beta_does(monkeypatch):
    _install(monkeypatch.setattr)
    from clip_dplm_amd.loss import clip_loss, contrastive_loss
    calls = trap_calls(monkeypatch.setattr, ("simce_lse_hard", "simce_grad_hard"))
    a0, b0 = _unit(24, 16, 5), _unit(24, 16, 6)
    ids = torch.tensor([0, 1, 2] * 8)
    for kw in (dict(), dict(hard_negative_beta=0.0), dict(hard_negative_beta=0, class_ids=ids),
               dict(hard_negative_beta=0.0, same_class="positive", label_smoothing=0.1)):
        a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        clip_loss(a, b, torch.tensor(14.0, requires_grad=True), **kw).backward()
    assert calls == []
    cache = _unit(7, 16, 8)
    for ids_k, beta, symmetric, c in ((None, 0.5, True, None), (ids, 1.0, True, cache), (ids, 0.5, False, None),
                                      (None, 0.5, False, cache)):
        a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        s = torch.tensor(14.0, requires_grad=True)
        loss = clip_loss(a, b, s, symmetric=symmetric, class_ids=ids_k, cache=c, hard_negative_beta=beta)
        loss.backward()
        L, ga, gb, gs = _reference(a0, b0, 14.0, ids_k, beta, symmetric, c)
        assert abs(loss.item() - L) < 1e-5
        assert torch.allclose(a.grad.double(), ga, atol=1e-6) and torch.allclose(b.grad.double(), gb, atol=1e-6)
        assert abs(s.grad.item() - gs.item()) < 1e-5
    assert "simce_lse_hard" in calls and "simce_grad_hard" in calls
    # contrastive_loss passes it through: one-sided, the queue rows as negatives, temperature as the scale
    x = a0.clone().requires_grad_(True)
    loss = contrastive_loss(x, b0, temperature=0.1, queue=cache, hard_negative_beta=0.5)
    loss.backward()
    xd = a0.double().requires_grad_(True)
    S = 10.0 * (F.normalize(xd, dim=-1) @ torch.cat([F.normalize(b0.double(), dim=-1), cache.double()]).t())
    L = R.loss_from_logits(S, a0.shape[0], None, 0.5, 1.0, 0.0)
    ga, = torch.autograd.grad(L, xd)
    assert abs(loss.item() - L.item()) < 1e-5 and torch.allclose(x.grad.double(), ga, atol=1e-6)


# ---------------------------------------------------------------------------------------------- gloo, world 2
CASES = ((True, 0.5, True), (False, 1.0, True), (True, 0.5, False), (False, 0.5, False))      # (ids, beta, symmetric)


def _rank_body(rank, world):
    from clip_dplm_amd import loss as L
    cases = [(with_ids, False, dict(hard_negative_beta=beta, symmetric=sym)) for with_ids, beta, sym in CASES]
    return clip_loss_cases(cases, spy_gathers(L), rank, world)


@pytest.mark.timeout(300)
def test_world2_hard_negative_matches_single_process():
    world, Bl, P = 2, 12, 16
    res = run_ranks(_rank_body, world)
    a, b = _unit(world * Bl, P, 1), _unit(world * Bl, P, 2)
    ids = torch.arange(world * Bl) % 5
    for k, (with_ids, beta, symmetric) in enumerate(CASES):
        L, ga, gb, gs = _reference(a, b, SCALE, ids if with_ids else None, beta, symmetric)
        plain = _reference(a, b, SCALE, ids if with_ids else None, 0.0, symmetric)[0]
        assert L - plain > 1e-3                                        # the weights matter here
        want = [(torch.float32, (2, Bl, P))] + ([(torch.int64, (Bl,))] if with_ids else []) + [(torch.float32, (6, Bl))]
        ds = 0.0
        for r in range(world):
            loss, da, db, dsr, gathered = res[r][k]
            assert gathered == want, gathered                          # embeddings, (ids,) one stack of coefficients
            assert abs(loss - L) < 1e-5, (k, r, loss, L)               # the global loss on every rank
            sl = slice(r * Bl, (r + 1) * Bl)
            assert torch.allclose(da.double(), ga[sl], atol=1e-6), (k, r)
            assert torch.allclose(db.double(), gb[sl], atol=1e-6), (k, r)
            ds += dsr.item()
        assert abs(ds - gs.item()) < 1e-5                              # summed over ranks by the optimiser
