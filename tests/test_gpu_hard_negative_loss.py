"""GPU: hard-negative-weighted InfoNCE on the fused similarity kernels (include/clipk.h: clipk_simce_lse_hard /
clipk_simce_grad_hard) and its use through clip_loss, RNARBPCLIPModel and GraphedTrainStep.  The yardstick is the f64
torch restatement of the definition on materialised logits (tests/hard_negative_ref.py, itself pinned on the CPU by
tests/test_hard_negative_host.py); shapes and id patterns are those of tests/test_gpu_class_aware_loss.py.

Tolerances.  The project's bar for an f32 LSE of S against f64 is atol = 2e-5 (test_gpu_class_aware_loss.py).  An LSE
moves by at most the largest error of its exponents; C exponentiates (1 + beta) S and A beta S, and
lse_h = logaddexp(pos, log n + C - A), so the bar on lse_h, on loss_i = lse_h - pos and on their mean is
2e-5 * (1 + 2 beta).  dX keeps the class-aware test's rtol = 1e-4 with atol = 1e-6 * (1 + beta), d scale its
1e-5 * max(1, |ref|) times (1 + beta): the gradient's exponents carry the factor (1 + beta) at most.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hard_negative_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SCALE = 14.2849
SHAPES = [(32, 32, 0, 512, 0), (1024, 1024, 0, 512, 0), (512, 4096, 0, 512, 1024), (128, 128, 200, 128, 0),
          (100, 300, 0, 36, 0)]
PATTERNS = [None, "distinct", "one", "random", "runs"]
BETAS = [0.5, 1.0]


def _unit(shape, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return F.normalize(torch.randn(*shape, generator=g, dtype=torch.float64), dim=-1).float().to(dev)


def _ids(pattern, n, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    if pattern is None:
        return None
    if pattern == "distinct":
        ids = torch.randperm(n, generator=g) * 7 - 3 * n          # distinct, negative ones included
    elif pattern == "one":
        ids = torch.full((n,), 5)
    elif pattern == "random":
        ids = torch.randint(0, max(1, n // 4), (n,), generator=g)
    else:                           # runs of 100 that cross 64-key tiles; at these shapes a key split is one tile
        #                             (splits of several tiles: tests/test_gpu_simce.py)
        ids = (torch.arange(n) + 30) // 100 + (1 << 40)
    return ids.to(torch.int64).to(dev)


def _reference(a_g, b_g, cache, ids, beta, w_row, w_col, rows):
    """f64: both directions over the whole pair batch, the block loss of `rows`, dL/dA[rows], d scale."""
    K = b_g if cache is None else torch.cat([b_g, cache])
    A, K = a_g.double(), K.double()
    Ny = b_g.shape[0]
    D = A @ K.t()
    S = (SCALE * D).requires_grad_(True)
    r = R.stats(S, Ny, 0, ids, ids, beta)
    c = R.stats(S[:, :Ny].t(), Ny, 0, ids, ids, beta)
    L = (w_row * r["loss"].sum() + w_col * c["loss"].sum()) / Ny
    G, = torch.autograd.grad(L, S)
    block = (w_row * r["loss"][rows].sum() + w_col * c["loss"][rows].sum()) / Ny
    return dict(lse_r=r["lse_h"].detach(), pos_r=r["pos"].detach(), lse_c=c["lse_h"].detach(), pos_c=c["pos"].detach(),
                block=block.item(), dA=SCALE * G[rows] @ K, dscale=(G[rows] * D[rows]).sum().item())


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_match_definition(dev, shape, beta):
    from clip_dplm_amd import ops
    Mx, Ny, Nc, P, off = shape
    a_g, b_g = _unit((Ny, P), dev, 1), _unit((Ny, P), dev, 2)
    cache = _unit((Nc, P), dev, 3) if Nc else None
    rows = slice(off, off + Mx)
    x = a_g[rows].contiguous()
    sc = torch.tensor([SCALE], device=dev)
    w_row, w_col = 0.5, 0.5
    bar = 2e-5 * (1 + 2 * beta)
    for pattern in PATTERNS:
        ids = _ids(pattern, Ny, dev)
        cx = None if ids is None else ids[rows].contiguous()
        ref = _reference(a_g, b_g, cache, ids, beta, w_row, w_col, rows)
        lse_r, pos_r, coef_r = ops.simce_lse_hard(x, b_g, sc, beta, cx, ids, label_offset=off, cache=cache)
        lse_c, pos_c, coef_c = ops.simce_lse_hard(b_g, a_g, sc, beta, ids, ids)          # every key's own row
        what = f"{pattern}"
        err = dict(lse_r=(lse_r.double() - ref["lse_r"][rows]).abs().max().item(),
                   pos_r=(pos_r.double() - ref["pos_r"][rows]).abs().max().item(),
                   loss_r=((lse_r.double() - pos_r.double()) - (ref["lse_r"] - ref["pos_r"])[rows]).abs().max().item(),
                   lse_c=(lse_c.double() - ref["lse_c"]).abs().max().item(),
                   pos_c=(pos_c.double() - ref["pos_c"]).abs().max().item(),
                   loss_c=((lse_c.double() - pos_c.double()) - (ref["lse_c"] - ref["pos_c"])).abs().max().item())
        loss = ops.ce_combine(lse_r, pos_r, lse_c[rows].contiguous(), pos_c[rows].contiguous(), w_row, w_col, Ny)
        dx, dsc = ops.simce_grad_hard(x, b_g, sc, beta, coef_r, coef_c, w_row, w_col, 1.0 / Ny, cls_x=cx, cls_y=ids,
                                      label_offset=off, cache=cache)
        err["block"] = abs(loss.item() - ref["block"])
        err["dx"] = (dx.double() - ref["dA"]).abs().max().item()
        err["dscale"] = abs(dsc.sum().item() - ref["dscale"])
        print(f"hard-negative {shape} beta={beta} ids={what}: " + " ".join(f"{k}={v:.2e}" for k, v in err.items())
              + f" (bar {bar:.1e}; |dscale ref| {abs(ref['dscale']):.3e})")
        for k in ("lse_r", "pos_r", "loss_r", "lse_c", "pos_c", "loss_c", "block"):
            assert err[k] <= bar, (what, k, err[k], bar)
        for t in (lse_r, pos_r, coef_r[0], lse_c, pos_c, coef_c[0], dx, dsc):
            assert bool(torch.isfinite(t).all()), what
        assert torch.allclose(dx.double(), ref["dA"], rtol=1e-4, atol=1e-6 * (1 + beta)), (what, err["dx"])
        assert err["dscale"] < 1e-5 * max(1.0, abs(ref["dscale"])) * (1 + beta), (what, err["dscale"], ref["dscale"])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_beta0_is_plain(dev, shape):
    """beta = 0 through the hard-negative kernels: the plain statistics and gradient within the plain tolerances."""
    from clip_dplm_amd import ops
    Mx, Ny, Nc, P, off = shape
    a_g, b_g = _unit((Ny, P), dev, 4), _unit((Ny, P), dev, 5)
    cache = _unit((Nc, P), dev, 6) if Nc else None
    x = a_g[off:off + Mx].contiguous()
    sc = torch.tensor([SCALE], device=dev)
    lse0, pos0 = ops.simce_lse(x, b_g, sc, label_offset=off, cache=cache)
    lc0, _ = ops.simce_lse(b_g, a_g, sc)
    d0, s0 = ops.simce_grad(x, b_g, sc, lse0, lc0, 0.5, 0.5, 1.0 / Ny, label_offset=off, cache=cache)
    for ids in (None, _ids("distinct", Ny, dev)):
        cx = None if ids is None else ids[off:off + Mx].contiguous()
        lse1, pos1, coef1 = ops.simce_lse_hard(x, b_g, sc, 0.0, cx, ids, label_offset=off, cache=cache)
        lc1, _, cc1 = ops.simce_lse_hard(b_g, a_g, sc, 0.0, ids, ids)
        assert torch.allclose(lse1, lse0, rtol=0, atol=2e-5) and torch.allclose(pos1, pos0, rtol=0, atol=2e-5)
        assert torch.allclose(lc1, lc0, rtol=0, atol=2e-5)
        assert bool((coef1[2] == float("-inf")).all())                           # the beta factor is 0
        d1, s1 = ops.simce_grad_hard(x, b_g, sc, 0.0, coef1, cc1, 0.5, 0.5, 1.0 / Ny, cls_x=cx, cls_y=ids,
                                     label_offset=off, cache=cache)
        assert torch.allclose(d1, d0, rtol=1e-4, atol=1e-6)
        assert abs(s1.sum().item() - s0.sum().item()) < 1e-5 * max(1.0, abs(s0.sum().item()))


def test_clip_loss_beta0_is_bitwise_the_default_call(dev):
    """hard_negative_beta = 0 takes the existing path: same autograd function, same launches, same bits."""
    from clip_dplm_amd.loss import clip_loss
    B, P = 192, 128
    a0, b0, cache = _unit((B, P), dev, 20), _unit((B, P), dev, 21), _unit((50, P), dev, 22)
    ids = _ids("random", B, dev, seed=2)
    for kw in (dict(), dict(symmetric=False), dict(cache=cache), dict(class_ids=ids),
               dict(class_ids=ids, same_class="positive", label_smoothing=0.1)):
        got = []
        for extra in (dict(), dict(hard_negative_beta=0.0)):
            a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
            s = torch.tensor(SCALE, device=dev, requires_grad=True)
            loss = clip_loss(a, b, s, **kw, **extra)
            loss.backward()
            got.append((loss.detach(), a.grad, b.grad, s.grad, type(loss.grad_fn).__name__))
        assert got[0][4] == got[1][4]
        for u, v in zip(got[0][:4], got[1][:4]):
            assert torch.equal(u, v), kw


@pytest.mark.parametrize("beta", BETAS)
def test_one_class_without_cache_is_exactly_zero(dev, beta):
    """Pattern `one`, no cache: no row has a negative; loss exactly 0, every gradient exactly 0, nothing non-finite."""
    from clip_dplm_amd import ops
    from clip_dplm_amd.loss import clip_loss
    for Mx, Ny, Nc, P, off in (s for s in SHAPES if s[2] == 0):
        a_g, b_g = _unit((Ny, P), dev, 1), _unit((Ny, P), dev, 2)
        ids = _ids("one", Ny, dev)
        x, cx = a_g[off:off + Mx].contiguous(), ids[off:off + Mx].contiguous()
        sc = torch.tensor([SCALE], device=dev)
        lse, pos, coef = ops.simce_lse_hard(x, b_g, sc, beta, cx, ids, label_offset=off)
        lse_c, pos_c, coef_c = ops.simce_lse_hard(b_g, a_g, sc, beta, ids, ids)
        assert torch.equal(lse, pos) and torch.equal(lse_c, pos_c)
        assert bool((coef[0] == 0).all()) and bool((coef[1:] == float("-inf")).all())
        dx, dsc = ops.simce_grad_hard(x, b_g, sc, beta, coef, coef_c, 0.5, 0.5, 1.0 / Ny, cls_x=cx, cls_y=ids,
                                      label_offset=off)
        assert bool((dx == 0).all()) and bool((dsc == 0).all())
    a, b = _unit((96, 64), dev, 7).requires_grad_(True), _unit((96, 64), dev, 8).requires_grad_(True)
    s = torch.tensor(SCALE, device=dev, requires_grad=True)
    loss = clip_loss(a, b, s, class_ids=_ids("one", 96, dev), hard_negative_beta=beta)
    loss.backward()
    assert loss.item() == 0.0 and bool((a.grad == 0).all()) and bool((b.grad == 0).all()) and s.grad.item() == 0.0


def _clip_ref(a, b, s, ids, beta, symmetric, cache=None):
    ad = a.detach().double().requires_grad_(True)
    bd = b.detach().double().requires_grad_(True)
    sd = s.detach().double().requires_grad_(True)
    K = bd if cache is None else torch.cat([bd, cache.double()])
    S = sd * (ad @ K.t())
    w = (0.5, 0.5) if symmetric else (1.0, 0.0)
    L = R.loss_from_logits(S, a.shape[0], ids, beta, *w)
    return (L,) + torch.autograd.grad(L, (ad, bd, sd))


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("case", ["symmetric", "one_sided", "cache", "class_ids", "class_ids_cache_one_sided"])
def test_clip_loss_autograd(dev, case, beta):
    from clip_dplm_amd.loss import clip_loss
    B, P = 96, 64
    a0, b0 = _unit((B, P), dev, 7), _unit((B, P), dev, 8)
    symmetric = "one_sided" not in case
    cache = _unit((150, P), dev, 9) if "cache" in case else None
    ids = torch.randint(0, 20, (B,), generator=torch.Generator().manual_seed(9)).to(dev) if "class_ids" in case else None
    runs = []
    for _ in range(2):
        a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        s = torch.tensor(SCALE, device=dev, requires_grad=True)
        loss = clip_loss(a, b, s, symmetric=symmetric, cache=cache, class_ids=None if ids is None else ids.to(torch.int32),
                         hard_negative_beta=beta)
        loss.backward()
        runs.append((loss.detach().clone(), a.grad.clone(), b.grad.clone(), s.grad.clone()))
    L, ga, gb, gs = _clip_ref(a0, b0, s, ids, beta, symmetric, cache)
    plain = _clip_ref(a0, b0, s, ids, 0.0, symmetric, cache)[0]
    loss, da, db, ds = runs[0]
    print(f"clip_loss {case} beta={beta}: loss err {abs(loss.item() - L.item()):.2e} dA {(da.double() - ga).abs().max():.2e} "
          f"dB {(db.double() - gb).abs().max():.2e} dscale {abs(ds.item() - gs.item()):.2e} (ref {gs.item():.3e})")
    assert L.item() > plain.item() + 1e-3                                        # the weights matter here
    assert abs(loss.item() - L.item()) <= 2e-5 * (1 + 2 * beta)
    assert torch.allclose(da.double(), ga, rtol=1e-4, atol=1e-6 * (1 + beta))
    assert torch.allclose(db.double(), gb, rtol=1e-4, atol=1e-6 * (1 + beta))
    assert abs(ds.item() - gs.item()) < 1e-5 * max(1.0, abs(gs.item())) * (1 + beta)
    for u, v in zip(runs[0], runs[1]):                                           # deterministic under one split plan
        assert torch.equal(u, v)


def test_rank_blocks_concatenate_to_global(dev):
    """The per-rank label_offset blocks of a 4-rank global batch give the global statistics and gradient."""
    from clip_dplm_amd import ops
    W, Bl, P, beta = 4, 256, 512, 0.5
    Bg = W * Bl
    a_g, b_g = _unit((Bg, P), dev, 13), _unit((Bg, P), dev, 14)
    ids = _ids("random", Bg, dev, seed=3)
    sc = torch.tensor([SCALE], device=dev)
    lse_r, pos_r, coef_r = ops.simce_lse_hard(a_g, b_g, sc, beta, ids, ids)
    _, _, coef_c = ops.simce_lse_hard(b_g, a_g, sc, beta, ids, ids)
    da_g, _ = ops.simce_grad_hard(a_g, b_g, sc, beta, coef_r, coef_c, 0.5, 0.5, 1.0 / Bg, cls_x=ids, cls_y=ids)
    parts = []
    for r in range(W):
        sl = slice(r * Bl, (r + 1) * Bl)
        x, cx = a_g[sl].contiguous(), ids[sl].contiguous()
        l, p, c = ops.simce_lse_hard(x, b_g, sc, beta, cx, ids, label_offset=r * Bl)
        # (another split plan for the 256-row block: a different, fixed summation order)
        assert torch.allclose(l, lse_r[sl], rtol=0, atol=2e-5) and torch.allclose(p, pos_r[sl], rtol=0, atol=2e-5)
        d, _ = ops.simce_grad_hard(x, b_g, sc, beta, c, coef_c, 0.5, 0.5, 1.0 / Bg, cls_x=cx, cls_y=ids,
                                   label_offset=r * Bl)
        parts.append(d)
    assert torch.allclose(torch.cat(parts), da_g, rtol=1e-4, atol=1e-6 * (1 + beta))


def test_graphed_train_step_with_hard_negatives_equals_eager(dev):
    """GraphedTrainStep with the class ids as one more input and hard_negative_beta = 0.5: a different class pattern on
    every replay, the same losses and weights as the steps issued eagerly."""
    import clip_dplm_amd as K
    from clip_dplm_amd.training import GraphedTrainStep

    def build():
        torch.manual_seed(1)
        m = K.RNARBPCLIPModel(rna_dim=40, rbp_dim=128, projection_dim=64, dropout=0.0)
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        return m.to(dev).train()
    g = torch.Generator().manual_seed(3)
    batches = []
    for k in range(3):
        rna, rbp = torch.randn(32, 6, 40, generator=g), torch.randn(32, 9, 128, generator=g)
        cls = torch.randint(0, 4 + 6 * k, (32,), generator=g)
        batches.append((rna.to(dev), rbp.to(dev), cls.to(dev)))
    me = build()
    oe = K.FusedAdamW(me, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    eager = []
    for i, (rna, rbp, cls) in enumerate(batches):
        oe.zero_grad()
        loss = me(rna, rbp, class_ids=cls, hard_negative_beta=0.5)[2]
        loss.backward()
        oe.step(lr=1e-3 * (1 + i))
        eager.append(loss.item())
    mg = build()
    og = K.FusedAdamW(mg, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    step = GraphedTrainStep(mg, og, lambda r, p, c: mg(r, p, class_ids=c, hard_negative_beta=0.5)[2], batches[0])
    graphed = [step(rna, rbp, cls, lr=1e-3 * (1 + i)).item() for i, (rna, rbp, cls) in enumerate(batches)]
    assert graphed == eager, (graphed, eager)
    for (n, p), (_, q) in zip(me.named_parameters(), mg.named_parameters()):
        assert torch.equal(p, q), n
    # the weights change the loss: the class-aware model's first step without them differs
    masked = build()(*batches[0][:2], class_ids=batches[0][2])[2].item()
    assert masked != eager[0]
