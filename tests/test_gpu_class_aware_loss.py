"""GPU: class-aware InfoNCE and label smoothing on the fused similarity + CE kernels (include/clipk.h:
clipk_simce_lse_cls / clipk_simce_grad_cls), the class-filtered rank (clipk_sim_rank_cls), and their use through
clip_loss, RNARBPCLIPModel, GraphedTrainStep and retrieval_metrics.  The reference is the f64 torch restatement of the
definitions on materialised logits (tests/class_aware_ref.py)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_aware_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SCALE = 14.2849
SHAPES = [(32, 32, 0, 512, 0), (1024, 1024, 0, 512, 0), (512, 4096, 0, 512, 1024), (128, 128, 200, 128, 0),
          (100, 300, 0, 36, 0)]
PATTERNS = ["distinct", "one", "random", "runs"]


def _unit(shape, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return F.normalize(torch.randn(*shape, generator=g, dtype=torch.float64), dim=-1).float().to(dev)


def _ids(pattern, n, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
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


def _reference(a_g, b_g, cache, ids, same_class, eps, w_row, w_col, rows):
    """f64: stats of both directions over the whole pair batch, the block loss of `rows`, dL/dA[rows], d scale."""
    K = b_g if cache is None else torch.cat([b_g, cache])
    A, K = a_g.double(), K.double()
    Ny = b_g.shape[0]
    D = A @ K.t()
    S = (SCALE * D).requires_grad_(True)
    lse_r, tgt_r, cnt_r = R.stats(S, Ny, 0, ids, ids, same_class, eps)[:3]
    lse_c, tgt_c, cnt_c = R.stats(S[:, :Ny].t(), Ny, 0, ids, ids, same_class, eps)[:3]
    L = (w_row * (lse_r - tgt_r).sum() + w_col * (lse_c - tgt_c).sum()) / Ny
    G, = torch.autograd.grad(L, S)
    block = (w_row * (lse_r - tgt_r)[rows].sum() + w_col * (lse_c - tgt_c)[rows].sum()) / Ny
    return dict(lse_r=lse_r.detach(), tgt_r=tgt_r.detach(), cnt_r=cnt_r, lse_c=lse_c.detach(), tgt_c=tgt_c.detach(),
                cnt_c=cnt_c, block=block.item(), dA=SCALE * G[rows] @ K, dscale=(G[rows] * D[rows]).sum().item())


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("same_class", ["mask", "positive"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_match_definition(dev, shape, same_class, eps):
    from clip_dplm_amd import ops
    Mx, Ny, Nc, P, off = shape
    a_g, b_g = _unit((Ny, P), dev, 1), _unit((Ny, P), dev, 2)
    cache = _unit((Nc, P), dev, 3) if Nc else None
    rows = slice(off, off + Mx)
    x = a_g[rows].contiguous()
    sc = torch.tensor([SCALE], device=dev)
    w_row, w_col = 0.5, 0.5
    for pattern in PATTERNS:
        ids = _ids(pattern, Ny, dev)
        cx = ids[rows].contiguous()
        ref = _reference(a_g, b_g, cache, ids, same_class, eps, w_row, w_col, rows)
        lse_r, tgt_r, cnt_r = ops.simce_lse_cls(x, b_g, sc, cx, ids, same_class, eps, label_offset=off, cache=cache)
        lse_c, tgt_c, cnt_c = ops.simce_lse_cls(b_g, a_g, sc, ids, ids, same_class, eps)     # every key's own row
        what = f"{pattern}"
        assert torch.allclose(lse_r.double(), ref["lse_r"][rows], rtol=0, atol=2e-5), what
        assert torch.allclose(tgt_r.double(), ref["tgt_r"][rows], rtol=0, atol=2e-5), what
        assert torch.equal(cnt_r.double(), ref["cnt_r"][rows]), what
        assert torch.allclose(lse_c.double(), ref["lse_c"], rtol=0, atol=2e-5), what
        assert torch.allclose(tgt_c.double(), ref["tgt_c"], rtol=0, atol=2e-5), what
        assert torch.equal(cnt_c.double(), ref["cnt_c"]), what
        loss = ops.ce_combine(lse_r, tgt_r, lse_c[rows].contiguous(), tgt_c[rows].contiguous(), w_row, w_col, Ny)
        assert abs(loss.item() - ref["block"]) < 1e-5, (what, loss.item(), ref["block"])
        dx, dsc = ops.simce_grad_cls(x, b_g, sc, lse_r, lse_c, cnt_r, cnt_c, w_row, w_col, 1.0 / Ny, Ny, cls_x=cx,
                                     cls_y=ids, same_class=same_class, eps=eps, label_offset=off, cache=cache)
        assert torch.allclose(dx.double(), ref["dA"], rtol=1e-4, atol=1e-6), (what, (dx.double() - ref["dA"]).abs().max())
        assert abs(dsc.sum().item() - ref["dscale"]) < 1e-5 * max(1.0, abs(ref["dscale"])), what


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_distinct_ids_no_smoothing_is_plain(dev, shape, kopt):
    """All ids distinct and eps = 0: the plain loss; the LSE bit for bit, the rest within the plain tolerances.
    (The class-aware passes are the tiled kernels' instantiations; below 64 rows the plain path would default to the
    first-generation kernel, another summation order, so the plain side is pinned to the tiled kernels.)"""
    from clip_dplm_amd import ops
    kopt("simce_kernel", 2)
    Mx, Ny, Nc, P, off = shape
    a_g, b_g = _unit((Ny, P), dev, 4), _unit((Ny, P), dev, 5)
    cache = _unit((Nc, P), dev, 6) if Nc else None
    x = a_g[off:off + Mx].contiguous()
    sc = torch.tensor([SCALE], device=dev)
    ids = _ids("distinct", Ny, dev)
    cx = ids[off:off + Mx].contiguous()
    for same_class in ("mask", "positive"):
        lse0, pos0 = ops.simce_lse(x, b_g, sc, label_offset=off, cache=cache)
        lse1, tgt1, cnt1 = ops.simce_lse_cls(x, b_g, sc, cx, ids, same_class, 0.0, label_offset=off, cache=cache)
        lse2, tgt2, cnt2 = ops.simce_lse_cls(x, b_g, sc, None, None, same_class, 0.0, label_offset=off, cache=cache)
        assert torch.equal(lse1, lse0) and torch.equal(lse2, lse0)
        assert torch.allclose(tgt1, pos0, rtol=0, atol=2e-5) and torch.allclose(tgt2, pos0, rtol=0, atol=2e-5)
        assert bool((cnt1 == 1).all()) and bool((cnt2 == 1).all())
    lc0, _ = ops.simce_lse(b_g, a_g, sc)
    lc1, _, cc1 = ops.simce_lse_cls(b_g, a_g, sc, ids, ids)
    assert torch.equal(lc1, lc0)
    d0, s0 = ops.simce_grad(x, b_g, sc, lse0, lc0, 0.5, 0.5, 1.0 / Ny, label_offset=off, cache=cache)
    d1, s1 = ops.simce_grad_cls(x, b_g, sc, lse1, lc1, cnt1, cc1, 0.5, 0.5, 1.0 / Ny, Ny, cls_x=cx, cls_y=ids,
                                label_offset=off, cache=cache)
    assert torch.allclose(d1, d0, rtol=1e-4, atol=1e-6)
    assert abs(s1.sum().item() - s0.sum().item()) < 1e-5 * max(1.0, abs(s0.sum().item()))


def _clip_ref(a, b, s, ids, same_class, eps, symmetric, cache=None):
    ad = a.detach().double().requires_grad_(True)
    bd = b.detach().double().requires_grad_(True)
    sd = s.detach().double().requires_grad_(True)
    K = bd if cache is None else torch.cat([bd, cache.double()])
    S = sd * (ad @ K.t())
    w = (0.5, 0.5) if symmetric else (1.0, 0.0)
    L = R.loss_from_logits(S, a.shape[0], ids, same_class, eps, *w)
    return (L,) + torch.autograd.grad(L, (ad, bd, sd))


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("same_class", ["mask", "positive"])
def test_clip_loss_autograd(dev, symmetric, same_class):
    from clip_dplm_amd.loss import clip_loss
    B, P = 96, 64
    a0, b0 = _unit((B, P), dev, 7), _unit((B, P), dev, 8)
    ids = torch.randint(0, 20, (B,), generator=torch.Generator().manual_seed(9)).to(dev)
    for eps in (0.0, 0.1):
        a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        s = torch.tensor(SCALE, device=dev, requires_grad=True)
        loss = clip_loss(a, b, s, symmetric=symmetric, class_ids=ids.to(torch.int32), same_class=same_class,
                         label_smoothing=eps)
        loss.backward()
        L, ga, gb, gs = _clip_ref(a0, b0, s, ids, same_class, eps, symmetric)
        assert abs(loss.item() - L.item()) < 1e-5
        assert torch.allclose(a.grad.double(), ga, rtol=1e-4, atol=1e-6)
        assert torch.allclose(b.grad.double(), gb, rtol=1e-4, atol=1e-6)
        assert abs(s.grad.item() - gs.item()) < 1e-5 * max(1.0, abs(gs.item()))


def test_label_smoothing_matches_torch_cross_entropy(dev):
    """No ids, eps > 0: F.cross_entropy(..., label_smoothing=eps) in each direction, over [S | S_cache] for the rows."""
    from clip_dplm_amd.loss import clip_loss
    B, P, Nc, eps = 128, 128, 200, 0.1
    a0, b0, cache = _unit((B, P), dev, 10), _unit((B, P), dev, 11), _unit((Nc, P), dev, 12)
    a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    s = torch.tensor(SCALE, device=dev, requires_grad=True)
    loss = clip_loss(a, b, s, symmetric=True, cache=cache, label_smoothing=eps)
    loss.backward()
    ad, bd = a0.double().requires_grad_(True), b0.double().requires_grad_(True)
    lab = torch.arange(B, device=dev)
    S = SCALE * (ad @ bd.t())
    Sc = SCALE * (ad @ cache.double().t())
    ref = 0.5 * (F.cross_entropy(torch.cat([S, Sc], 1), lab, label_smoothing=eps)
                 + F.cross_entropy(S.t(), lab, label_smoothing=eps))
    ga, gb = torch.autograd.grad(ref, (ad, bd))
    assert abs(loss.item() - ref.item()) < 1e-5
    assert torch.allclose(a.grad.double(), ga, rtol=1e-4, atol=1e-6)
    assert torch.allclose(b.grad.double(), gb, rtol=1e-4, atol=1e-6)


def test_rank_blocks_concatenate_to_global(dev):
    """The per-rank label_offset blocks of a 4-rank global batch give the global stats, loss and gradient."""
    from clip_dplm_amd import ops
    W, Bl, P = 4, 256, 512
    Bg = W * Bl
    a_g, b_g = _unit((Bg, P), dev, 13), _unit((Bg, P), dev, 14)
    ids = _ids("random", Bg, dev, seed=3)
    sc = torch.tensor([SCALE], device=dev)
    for same_class in ("mask", "positive"):
        lse_r, tgt_r, cnt_r = ops.simce_lse_cls(a_g, b_g, sc, ids, ids, same_class, 0.1)
        lse_c, tgt_c, cnt_c = ops.simce_lse_cls(b_g, a_g, sc, ids, ids, same_class, 0.1)
        da_g, _ = ops.simce_grad_cls(a_g, b_g, sc, lse_r, lse_c, cnt_r, cnt_c, 0.5, 0.5, 1.0 / Bg, Bg, cls_x=ids,
                                     cls_y=ids, same_class=same_class, eps=0.1)
        parts = []
        for r in range(W):
            sl = slice(r * Bl, (r + 1) * Bl)
            x, cx = a_g[sl].contiguous(), ids[sl].contiguous()
            l, t, c = ops.simce_lse_cls(x, b_g, sc, cx, ids, same_class, 0.1, label_offset=r * Bl)
            assert torch.equal(l, lse_r[sl]) and torch.equal(c, cnt_r[sl])
            assert torch.allclose(t, tgt_r[sl], rtol=0, atol=2e-5)
            d, _ = ops.simce_grad_cls(x, b_g, sc, l, lse_c, c, cnt_c, 0.5, 0.5, 1.0 / Bg, Bg, cls_x=cx, cls_y=ids,
                                      same_class=same_class, eps=0.1, label_offset=r * Bl)
            parts.append(d)
        assert torch.allclose(torch.cat(parts), da_g, rtol=1e-5, atol=1e-7)


def test_graphed_train_step_with_class_ids_equals_eager(dev):
    """GraphedTrainStep with the class ids as one more input: a different class pattern on every replay, the same
    losses and weights as the steps issued eagerly."""
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
    for k in range(5):
        rna, rbp = torch.randn(32, 6, 40, generator=g), torch.randn(32, 9, 128, generator=g)
        cls = torch.randint(0, 4 + 6 * k, (32,), generator=g)
        batches.append((rna.to(dev), rbp.to(dev), cls.to(dev)))
    me = build()
    oe = K.FusedAdamW(me, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    eager = []
    for i, (rna, rbp, cls) in enumerate(batches):
        oe.zero_grad()
        loss = me(rna, rbp, class_ids=cls, same_class="positive", label_smoothing=0.1)[2]
        loss.backward()
        oe.step(lr=1e-3 * (1 + i))
        eager.append(loss.item())
    mg = build()
    og = K.FusedAdamW(mg, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    step = GraphedTrainStep(mg, og, lambda r, p, c: mg(r, p, class_ids=c, same_class="positive",
                                                       label_smoothing=0.1)[2], batches[0])
    graphed = [step(rna, rbp, cls, lr=1e-3 * (1 + i)).item() for i, (rna, rbp, cls) in enumerate(batches)]
    assert graphed == eager, (graphed, eager)
    for (n, p), (_, q) in zip(me.named_parameters(), mg.named_parameters()):
        assert torch.equal(p, q), n
    # the class ids change the loss: the plain model's first step differs
    plain = build()(*batches[0][:2])[2].item()
    assert plain != eager[0]


def test_filtered_ranks(dev):
    """Exact scores (small multiples of 1/4: every dot product is exact in f32) with duplicated gallery rows, so ties
    across and within classes are exercised bit for bit."""
    from clip_dplm_amd import ops, retrieval
    Mx, Ny, P = 300, 700, 64
    g = torch.Generator().manual_seed(4)
    x = (torch.randint(-2, 3, (Mx, P), generator=g) / 4.0).float().to(dev)
    y = (torch.randint(-2, 3, (Ny, P), generator=g) / 4.0).float().to(dev)
    y[torch.randint(0, Ny, (Ny // 8,), generator=g).to(dev)] = y[torch.randint(0, Ny, (Ny // 8,), generator=g).to(dev)]
    labels = torch.randint(0, Ny, (Mx,), generator=g).to(dev)
    S = x.double() @ y.double().t()
    plain, _ = ops.sim_rank(x, y, labels=labels)
    for pattern in PATTERNS:
        ids = _ids(pattern, Ny, dev, seed=5)
        r, _ = ops.sim_rank(x, y, labels=labels, class_ids=ids)
        assert torch.equal(r, R.filtered_rank(S, labels, ids)), pattern
        if pattern == "distinct":
            assert torch.equal(r, plain)
        assert torch.equal(retrieval.ranks(x, y, labels, class_ids=ids), r)
    # duplicate partners: a perfect model reaches recall@1 = 1 only with the ids
    B, P = 256, 32
    base = _unit((64, P), dev, 17)
    grp = torch.arange(B, device=dev) % 64
    a = b = base[grp].contiguous()
    m0 = retrieval.retrieval_metrics(a, b)
    m1 = retrieval.retrieval_metrics(a, b, class_ids=grp)
    assert m0["a_to_b"]["top1"] < 0.5 and m1["a_to_b"]["top1"] == 1.0 and m1["b_to_a"]["top1"] == 1.0
