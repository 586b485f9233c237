"""GPU: fused top-k and rank-of-positive over embedding galleries (include/clipk.h: clipk_sim_topk / clipk_sim_rank) and
the retrieval API on top of them (clip_dplm_amd/retrieval.py).

Order contract: score descending, equal scores by the lower gallery index."""
import gc

import pytest
import torch

from clip_dplm_amd import ops, retrieval

pytestmark = pytest.mark.gpu


def _grid_inputs(n, P, g, dev):
    """Entries in {-3..3}/4: every f32 product and partial sum is exact, so S equals the f64 product."""
    return (torch.randint(-3, 4, (n, P), generator=g).float() / 4).to(dev)


def _exact_reference(x, y, scale):
    """Integer dot products D = 16 <x, y> (exact), and the order key -D * (Ny + 1) + j: unique, ascending = best first."""
    D = torch.round((x.double() @ y.double().t()) * 16).long()
    Ny = y.shape[0]
    key = -D * (Ny + 1) + torch.arange(Ny, device=x.device)
    return D, key


@pytest.mark.parametrize("P", [4, 60, 120, 512, 1028])
@pytest.mark.parametrize("Ny", ["k", 63, 4097, 100003])
def test_exact_ties_bit_for_bit(dev, P, Ny):
    g = torch.Generator().manual_seed(P * 7 + (0 if Ny == "k" else Ny))
    scale = 0.25                                                   # power of two: scale * S stays exact
    x_all = _grid_inputs(1000, P, g, dev)
    for k in (1, 7, 32, 64):
        ny = k if Ny == "k" else Ny
        if k > ny:
            continue
        if Ny == "k" and k != 64 and P not in (4, 512):
            continue                                               # Ny = k: a handful of shapes is enough
        y = _grid_inputs(ny, P, g, dev)
        if ny > 8:                                                 # duplicated gallery rows: exact ties by construction
            src = torch.randint(0, ny, (ny // 8,), generator=g).to(dev)
            dst = torch.randint(0, ny, (ny // 8,), generator=g).to(dev)
            y[dst] = y[src]
        D, key = _exact_reference(x_all, y, scale)
        ref_key, ref_idx = torch.topk(key, k, dim=1, largest=False, sorted=True)
        ref_scores = (D.gather(1, ref_idx).double() / 16 * scale).float()
        labels = torch.randint(0, ny, (1000,), generator=g).to(dev)
        dl = D.gather(1, labels[:, None])
        jj = torch.arange(ny, device=dev)
        ref_rank = (D > dl).sum(1) + ((D == dl) & (jj[None, :] < labels[:, None])).sum(1)
        for Mx in (1, 63, 65, 1000):
            x = x_all[:Mx].contiguous()
            s, i = ops.sim_topk(x, y, k, scale=scale)
            assert torch.equal(i, ref_idx[:Mx]), (Mx, ny, k, P)
            assert torch.equal(s, ref_scores[:Mx]), (Mx, ny, k, P)
            r, pos = ops.sim_rank(x, y, labels=labels[:Mx], scale=scale)
            assert torch.equal(r, ref_rank[:Mx]), (Mx, ny, k, P)
            assert torch.equal(pos, (dl[:Mx, 0].double() / 16 * scale).float())
            if Mx <= ny:                                           # labels label_offset + i
                off = (ny - Mx) // 2
                lab = torch.arange(off, off + Mx, device=dev)
                dl2 = D[:Mx].gather(1, lab[:, None])
                want = (D[:Mx] > dl2).sum(1) + ((D[:Mx] == dl2) & (jj[None, :] < lab[:, None])).sum(1)
                r2, _ = ops.sim_rank(x, y, label_offset=off, scale=scale)
                assert torch.equal(r2, want)
        del D, key


def _unit(n, P, g, dev):
    v = torch.randn(n, P, generator=g, dtype=torch.float64)
    return (v / v.norm(dim=1, keepdim=True)).float().to(dev)


@pytest.mark.parametrize("P,k", [(120, 10), (512, 16), (128, 64), (256, 1)])
def test_random_unit_vectors_against_f64(dev, kopt, P, k):
    g = torch.Generator().manual_seed(P + k)
    x, y = _unit(300, P, g, dev), _unit(30011, P, g, dev)
    scale = 14.2857
    s, i = ops.sim_topk(x, y, k, scale=scale)
    S64 = x.double() @ y.double().t()
    assert (s[:, :-1] >= s[:, 1:]).all()
    assert ((s.double() - scale * S64.gather(1, i)).abs() <= 2e-5 * scale).all()
    assert all(len(set(row)) == k for row in i.cpu().tolist())
    kth = S64.gather(1, i).min(1).values
    rest = S64.scatter(1, i, float("-inf")).max(1).values
    assert (rest <= kth + 4e-6).all()                             # a valid top-k up to a 4e-6 window
    s2, i2 = ops.sim_topk(x, y, k, scale=scale)
    assert torch.equal(s, s2) and torch.equal(i, i2)
    labels = torch.randint(0, y.shape[0], (300,), generator=g).to(dev)
    r, pos = ops.sim_rank(x, y, labels=labels, scale=scale)
    for splits in (1, 2, 5, 64, 1000):                             # every split plan gives the same bits
        kopt("retrieval_splits", splits)
        s3, i3 = ops.sim_topk(x, y, k, scale=scale)
        assert torch.equal(s, s3) and torch.equal(i, i3), splits
        r3, pos3 = ops.sim_rank(x, y, labels=labels, scale=scale)
        assert torch.equal(r, r3) and torch.equal(pos, pos3), splits


def test_topk_and_rank_agree(dev):
    g = torch.Generator().manual_seed(3)
    x, y = _unit(500, 128, g, dev), _unit(5000, 128, g, dev)
    # half the labels are each query's best match (rank 0), the rest random
    k = 10
    s, i = ops.sim_topk(x, y, k)
    labels = torch.randint(0, 5000, (500,), generator=g).to(dev)
    labels[::2] = i[::2, 0]
    labels[1::4] = i[1::4, 3]
    r, pos = ops.sim_rank(x, y, labels=labels)
    hit = (i == labels[:, None])
    assert torch.equal(hit.any(1), r < k)
    rows = torch.nonzero(r < k).flatten()
    assert len(rows) >= 250
    assert torch.equal(i[rows, r[rows]], labels[rows])
    assert torch.equal(s[rows, r[rows]], pos[rows])                # the same bits from both entry points
    assert (r[::2] == 0).all()


def test_ascending_gallery_every_score_inserts(dev):
    # scores rise along the key order: every key beats the current k-th; k = 64 lists the last 64 keys, newest first
    Ny, P = 70001, 4
    y = torch.zeros(Ny, P, device=dev)
    y[:, 0] = torch.arange(1, Ny + 1, device=dev, dtype=torch.float32) / 65536
    x = torch.zeros(130, P, device=dev)
    x[:, 0] = 1.0
    s, i = ops.sim_topk(x, y, 64)
    want = torch.arange(Ny - 1, Ny - 65, -1, device=dev)
    assert (i == want[None, :]).all()
    assert torch.equal(s, y[want, 0][None, :].expand(130, -1))
    r, _ = ops.sim_rank(x, y, labels=torch.full((130,), 5, dtype=torch.int64, device=dev))
    assert (r == Ny - 6).all()


def test_out_of_range_device_labels(dev):
    g = torch.Generator().manual_seed(4)
    x, y = _unit(70, 64, g, dev), _unit(300, 64, g, dev)
    labels = torch.randint(0, 300, (70,), generator=g).to(dev)
    labels[3], labels[40] = -1, 300
    r, pos = ops.sim_rank(x, y, labels=labels)
    assert r[3] == -1 and r[40] == -1 and torch.isnan(pos[3]) and torch.isnan(pos[40])
    ok = torch.ones(70, dtype=torch.bool, device=dev)
    ok[3] = ok[40] = False
    assert (r[ok] >= 0).all()


def test_large_gallery_64bit_offsets(dev):
    Ny, P = (1 << 21) + 13, 1024                                   # Ny * P > 2^31 elements: 8 GiB of f32
    torch.manual_seed(5)
    y = torch.randn(Ny, P, device=dev)
    y.div_(y.norm(dim=1, keepdim=True))
    planted = torch.tensor([(1 << 21) + 1, (1 << 21) + 7, Ny - 1, 12345], device=dev)
    x = y[planted].clone()                                         # exact copies of gallery rows beyond 2^21
    try:
        s, i = ops.sim_topk(x, y, 1)
        assert torch.equal(i[:, 0], planted)
        assert ((s[:, 0] - 1.0).abs() <= 1e-5).all()
        r, pos = ops.sim_rank(x, y, labels=planted)
        assert (r == 0).all() and torch.equal(pos, s[:, 0])
        # margin: the runner-up is far below (random unit rows in 1024 dimensions)
        s5, _ = ops.sim_topk(x, y, 5)
        assert (s5[:, 0] - s5[:, 1] > 1e-3).all()
    finally:
        del y, x
        gc.collect()
        torch.cuda.empty_cache()


def _loader(n_batches, B, shapes, g, dev):
    return [tuple(torch.randn(B, *sh, generator=g).to(dev) for sh in shapes) for _ in range(n_batches)]


def _check_model(model, loader):
    model.eval()
    with torch.no_grad():
        pairs = [retrieval.default_embed_fn(model, b) for b in loader]
    correct, total, near = 0, 0, 0
    for a, b in pairs:
        L = a.double() @ b.double().t()
        top2 = L.topk(2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) >= 1e-5
        near += int((~clear).sum())
        lab = torch.arange(a.shape[0], device=a.device)
        correct += int(((L.argmax(1) == lab) & clear).sum())
        total += int(clear.sum())
    res = retrieval.evaluate_retrieval(model, loader, per_batch=True)
    n = sum(a.shape[0] for a, _ in pairs)
    assert near <= n // 50
    # the kernel's top1 over all rows minus its verdict on the near-tie rows == the f64 argmax accuracy on the rest
    ranks_ab = torch.cat([retrieval.ranks(a, b) for a, b in pairs])
    clear_all = torch.cat([(lambda t: (t[:, 0] - t[:, 1]) >= 1e-5)((a.double() @ b.double().t()).topk(2, 1).values)
                           for a, b in pairs])
    assert int(((ranks_ab == 0) & clear_all).sum()) == correct
    if near == 0:
        assert res["a_to_b"]["top1"] == correct / total
    assert res["a_to_b"]["n"] == n and res["b_to_a"]["n"] == n
    # global mode == retrieval_metrics on the concatenated embeddings
    glob = retrieval.evaluate_retrieval(model, loader)
    want = retrieval.retrieval_metrics(torch.cat([a for a, _ in pairs]), torch.cat([b for _, b in pairs]))
    assert glob == want


def test_model_level_rnaprotein_clip(dev):
    import clip_dplm_amd as K
    torch.manual_seed(6)
    cfg = K.HybridCLIPConfig(rna_config={"hidden_size": 64, "num_hidden_layers": 2},
                             protein_config={"hidden_size": 96, "num_hidden_layers": 2}, diffmap_config={},
                             projection_dim=64)
    m = K.RNAProteinCLIP(cfg).to(dev)
    g = torch.Generator().manual_seed(7)
    _check_model(m, _loader(4, 128, [(64,), (96,)], g, dev))


def test_model_level_rnarbp_clip(dev):
    import clip_dplm_amd as K
    torch.manual_seed(8)
    m = K.RNARBPCLIPModel(rna_dim=40, rbp_dim=128, projection_dim=64, dropout=0.0).to(dev)
    g = torch.Generator().manual_seed(9)
    _check_model(m, _loader(3, 96, [(5, 40), (5, 128)], g, dev))


def test_embedding_index_matches_one_shot_topk(dev):
    g = torch.Generator().manual_seed(10)
    chunks = [_unit(n, 96, g, dev) for n in (37, 1, 1500, 1024, 3, 2000)]
    idx = retrieval.EmbeddingIndex(96, dev)
    for c in chunks:
        idx.add(c)
    gallery = torch.cat(chunks)
    assert len(idx) == gallery.shape[0]
    q = _unit(77, 96, g, dev)
    s0, i0 = retrieval.topk(q, gallery, 20)
    s1, i1 = idx.search(q, 20)
    assert torch.equal(s0, s1) and torch.equal(i0, i1)
    idx2 = retrieval.EmbeddingIndex(96, dev)
    sd = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in idx.state_dict().items()}
    idx2.load_state_dict(sd)
    s2, i2 = idx2.search(q, 20)
    assert torch.equal(s0, s2) and torch.equal(i0, i2)
    # bf16 embeddings are cast to f32 on the way in: the same as casting the whole gallery
    idx3 = retrieval.EmbeddingIndex(96, dev)
    for c in chunks:
        idx3.add(c.bfloat16())
    s3, i3 = idx3.search(q, 20)
    s4, i4 = retrieval.topk(q, gallery.bfloat16(), 20)
    assert torch.equal(s3, s4) and torch.equal(i3, i4)
