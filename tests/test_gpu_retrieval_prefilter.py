"""GPU: prefiltered exact top-k (retrieval.topk / EmbeddingIndex with prefilter="bf16" / "bf16x3"; include/clipk.h
clipk_split_bf16, clipk_sim_topk_cand, clipk_sim_rerank).  The contract is bitwise equality with prefilter=None."""
import gc

import pytest
import torch

from clip_dplm_amd import ops, retrieval

pytestmark = pytest.mark.gpu

MODES = ("bf16", "bf16x3")


def _unit(v):
    return v / v.norm(dim=1, keepdim=True)


def _data(kind, Mq, Ny, P, g, dev):
    """(queries, gallery) f32 on dev."""
    if kind == "random":
        return _unit(torch.randn(Mq, P, generator=g, device=dev)), _unit(torch.randn(Ny, P, generator=g, device=dev))
    if kind == "clustered":                              # near-duplicates: centres plus noise of about 1e-3
        c = _unit(torch.randn(max(2, Ny // 50), P, generator=g, device=dev))
        pick = lambda n: c[torch.randint(0, c.shape[0], (n,), generator=g, device=dev)]  # noqa: E731
        y = pick(Ny) + 1e-3 / P ** 0.5 * torch.randn(Ny, P, generator=g, device=dev)
        x = pick(Mq) + 1e-3 / P ** 0.5 * torch.randn(Mq, P, generator=g, device=dev)
        return x, y
    if kind == "grid":                                   # entries in {-3..3}/4, duplicated rows: exact ties
        q = (torch.randint(-3, 4, (Mq, P), generator=g, device=dev).float() / 4)
        y = (torch.randint(-3, 4, (Ny, P), generator=g, device=dev).float() / 4)
        if Ny > 8:
            src = torch.randint(0, Ny, (Ny // 8,), generator=g, device=dev)
            dst = torch.randint(0, Ny, (Ny // 8,), generator=g, device=dev)
            y[dst] = y[src]
        return q, y
    if kind == "ascending":                              # shape d's pattern: every key beats the previous ones
        y = 0.01 * torch.randn(Ny, P, generator=g, device=dev)
        y[:, 0] = torch.arange(1, Ny + 1, device=dev, dtype=torch.float32) / Ny
        x = 0.01 * torch.randn(Mq, P, generator=g, device=dev)
        x[:, 0] = 1.0
        return x, y
    if kind == "cancel":                                 # sum |x_p y_p| >> |x . y|
        h = P // 2
        u = torch.randn(Ny, h, generator=g, device=dev)
        v = torch.randn(Mq, h, generator=g, device=dev)
        return (torch.cat([v, -v + 1e-2 * torch.randn(Mq, h, generator=g, device=dev)], 1),
                torch.cat([u, u], 1))
    raise ValueError(kind)


KINDS = ("random", "clustered", "grid", "ascending", "cancel")
# (Ny, Mq, k, scale, candidates): a subset of the grid that hits every value; Ny "kc" / "kc+1" follow the candidates
COMBOS = [
    ("kc", 1, 1, 1.0, None), ("kc+1", 63, 10, 0.25, "k+1"), ("kc", 65, 32, 14.3, "k+1"), ("kc+1", 64, 63, -1.0, None),
    (4097, 64, 32, 1.0, None), (4097, 65, 63, -1.0, "k+1"), (4097, 1000, 1, 14.3, "k+1"), (4097, 63, 10, 0.25, None),
    (100003, 1000, 10, 1.0, None), (100003, 65, 63, 0.25, None), (100003, 1, 32, -1.0, "k+1"),
    (100003, 64, 1, 14.3, None),
]


def _kc(k, cand, mode):
    if cand is not None:
        return k + 1
    return 64 if mode == "bf16" else min(64, max(16, 2 * k))


@pytest.mark.parametrize("P", [4, 60, 120, 512, 1028])
@pytest.mark.parametrize("kind", KINDS)
def test_equals_exact_path(dev, P, kind):
    g = torch.Generator(device=dev).manual_seed(P * 31 + KINDS.index(kind))
    for Ny, Mq, k, scale, cand in COMBOS:
        if P == 1028 and Ny == 100003 and Mq == 1000:
            Mq = 300                                     # keeps the exact reference cheap at the widest rows
        for mode in MODES:
            kc = _kc(k, cand, mode)
            ny = kc if Ny == "kc" else kc + 1 if Ny == "kc+1" else Ny
            x, y = _data(kind, Mq, ny, P, g, dev)
            s0, i0 = retrieval.topk(x, y, k, scale=scale)
            s1, i1, st = retrieval.topk(x, y, k, scale=scale, prefilter=mode,
                                        candidates=None if cand is None else kc, return_stats=True)
            key = (kind, P, ny, Mq, k, scale, kc, mode, st["certified"])
            assert torch.equal(i1, i0), key
            assert torch.equal(s1, s0), key
            assert st["queries"] == Mq and st["candidates"] == kc and st["prefilter"] == mode
            assert 0 <= st["certified"] <= Mq
            if ny <= kc:
                assert st["certified"] == Mq, key            # every key is a candidate
            del x, y
    torch.cuda.empty_cache()


@pytest.mark.parametrize("Ny", [65, 4097])               # a one-key tail tile; several key splits
@pytest.mark.parametrize("kc", [16, 32, 64])             # the three list widths of the candidate pass
@pytest.mark.parametrize("mode", MODES)
def test_equals_exact_path_every_list_width(dev, mode, kc, Ny):
    """All six candidate kernels at a ragged shape: one full query block plus one row, plane pitch 64 with a zero pad."""
    Mq, P, k = 129, 36, kc // 2
    g = torch.Generator(device=dev).manual_seed(kc * 7 + Ny)
    for kind in ("random", "grid"):
        x, y = _data(kind, Mq, Ny, P, g, dev)
        s0, i0 = retrieval.topk(x, y, k)
        s1, i1, st = retrieval.topk(x, y, k, prefilter=mode, candidates=kc, return_stats=True)
        assert torch.equal(i1, i0) and torch.equal(s1, s0), (kind, mode, kc, Ny, st)
        assert st["queries"] == Mq and st["candidates"] == kc and st["prefilter"] == mode


def test_certified_fraction_and_fallback(dev):
    g = torch.Generator(device=dev).manual_seed(11)
    for P in (120, 512):
        x, y = _data("random", 1000, 4097, P, g, dev)
        s0, i0 = retrieval.topk(x, y, 10)
        for mode in MODES:
            s1, i1, st = retrieval.topk(x, y, 10, prefilter=mode, return_stats=True)
            assert torch.equal(s1, s0) and torch.equal(i1, i0)
            assert st["certified"] >= 0.99 * st["queries"], (P, mode, st)
    x, y = _data("clustered", 1000, 4097, 120, g, dev)
    s0, i0 = retrieval.topk(x, y, 10)
    s1, i1, st = retrieval.topk(x, y, 10, prefilter="bf16", return_stats=True)
    assert st["certified"] < st["queries"], st           # near-duplicates: bf16 cannot separate them, the fallback runs
    assert torch.equal(s1, s0) and torch.equal(i1, i0)


@pytest.mark.parametrize("kind", KINDS)
def test_measured_error_within_the_bound(dev, kind):
    """Every candidate: |approximate - exact score| <= eps_q (the whole bound), and the bf16 MFMA's undocumented
    accumulation, measured against the f64 sum of the same bf16 operand products, within half its term."""
    g = torch.Generator(device=dev).manual_seed(100 + KINDS.index(kind))
    worst = 0.0
    for P in (4, 60, 120, 512, 1028):
        for Ny, Mq, scale in ((4097, 200, 1.0), (4097, 65, -1.0), (100003, 64, 14.3), (100003, 63, 0.25)):
            x, y = _data(kind, Mq, Ny, P, g, dev)
            for mode in MODES:
                hi, lo = retrieval._new_planes(Ny, P, mode, dev)
                nm = torch.zeros(1, device=dev)
                ops.split_bf16(y, hi, lo, nm)
                cs, ci = ops.sim_topk_cand(x, hi, lo, Ny, P, 64, scale)
                es, ei, _ = ops.sim_rerank(x, y, cs, ci, 64, 0.0, nm, scale)   # exact scores of all 64 candidates
                o1, o2 = ci.argsort(1), ei.argsort(1)
                assert torch.equal(ci.gather(1, o1), ei.gather(1, o2))
                approx, exact = cs.gather(1, o1).double(), es.gather(1, o2).double()
                xn = x.double().norm(dim=1, keepdim=True)
                eps = (abs(scale) * xn * float(nm) * retrieval.prefilter_eps_rel(P, mode)
                       + (abs(scale) * P * (xn + float(nm) + 1) + 1) * 2.0 ** -120)
                err = (approx - exact).abs()
                assert (err <= eps).all(), (kind, P, Ny, mode, float((err / eps).max()))
                # accumulation alone: the products of the bf16 operands the kernel saw, summed in f64
                pp = ops.plane_pitch(P)
                xq = torch.zeros(Mq, pp, device=dev)
                xq[:, :P] = x
                xh = xq.bfloat16().double()
                terms = [(xh, hi)]
                if mode == "bf16x3":
                    xl = (xq - xq.bfloat16().float()).bfloat16().double()
                    terms += [(xl, hi), (xh, lo)]
                emu = torch.zeros(Mq, 64, dtype=torch.float64, device=dev)
                mag = torch.zeros_like(emu)
                for a, plane in terms:
                    rows = plane[ci.gather(1, o1)].double()                   # [Mq, 64, pp]
                    prod = rows * a[:, None, :]
                    emu += prod.sum(2)
                    mag += prod.abs().sum(2)
                n = P * len(terms)
                acc_err = (approx - scale * emu).abs()
                allowed = 0.5 * abs(scale) * n * 2.0 ** -22 * mag + (scale * emu).abs() * 2.0 ** -23 + 2.0 ** -120
                assert (acc_err <= allowed).all(), (kind, P, Ny, mode, float((acc_err / allowed).max()))
                worst = max(worst, float((err / eps).max()))
            del x, y
    assert worst <= 1.0


def test_rerank_alone_has_the_exact_bits(dev):
    g = torch.Generator(device=dev).manual_seed(12)
    for P, Ny in ((4, 17), (60, 64), (120, 40), (1028, 64)):
        x = torch.randn(70, P, generator=g, device=dev)
        y = torch.randn(Ny, P, generator=g, device=dev)
        for scale in (1.0, -0.25, 14.3):
            s_all, i_all = ops.sim_topk(x, y, Ny, scale=scale)      # every key's exact score, in order
            for kc in (2, 9, Ny):
                ci = torch.stack([torch.randperm(Ny, generator=g, device=dev)[:kc] for _ in range(70)])
                cs = torch.zeros(70, kc, device=dev)                  # any finite approximate scores
                k = max(1, kc // 2)
                s, i, _ = ops.sim_rerank(x, y, cs, ci, k, retrieval.prefilter_eps_rel(P, "bf16"),
                                         torch.full((1,), 1e3, device=dev), scale)
                member = (i_all[:, :, None] == ci[:, None, :]).any(2)  # [70, Ny]: key of the full list is a candidate
                pos = member.float().cumsum(1) - 1
                want_i = torch.empty(70, k, dtype=torch.int64, device=dev)
                want_s = torch.empty(70, k, device=dev)
                r, c = torch.nonzero(member & (pos < k), as_tuple=True)
                want_i[r, pos[r, c].long()] = i_all[r, c]
                want_s[r, pos[r, c].long()] = s_all[r, c]
                assert torch.equal(i, want_i) and torch.equal(s, want_s), (P, Ny, scale, kc)


def test_split_planes(dev):
    g = torch.Generator(device=dev).manual_seed(13)
    for P in (4, 60, 1028):
        y = torch.randn(333, P, generator=g, device=dev) * torch.rand(333, 1, generator=g, device=dev) * 3
        y[5, :] *= 2.0 ** -125                                       # subnormal parts
        hi, lo = retrieval._new_planes(333, P, "bf16x3", dev)
        nm = torch.zeros(1, device=dev)
        ops.split_bf16(y, hi, lo, nm)
        pp = ops.plane_pitch(P)
        assert torch.equal(hi[:, :P], y.bfloat16()) and (hi[:, P:].float() == 0).all()
        assert torch.equal(lo[:, :P], (y - y.bfloat16().float()).bfloat16()) and (lo[:, P:].float() == 0).all()
        true = float(y.double().norm(dim=1).max())
        assert true <= float(nm) <= true * (1 + 1e-6) and pp % 32 == 0


def test_embedding_index_with_prefilter(dev):
    g = torch.Generator(device=dev).manual_seed(14)
    chunks = [_unit(torch.randn(n, 96, generator=g, device=dev)) for n in (37, 1, 1500, 1024, 3, 2000)]
    q = _unit(torch.randn(77, 96, generator=g, device=dev))
    exact = retrieval.EmbeddingIndex(96, dev)
    for c in chunks:
        exact.add(c)
    s0, i0 = exact.search(q, 20)
    for mode in MODES:
        idx = retrieval.EmbeddingIndex(96, dev, prefilter=mode)
        for c in chunks:                                              # crosses two capacity growths
            idx.add(c)
        assert len(idx) == sum(c.shape[0] for c in chunks)
        s1, i1, st = idx.search(q, 20, return_stats=True)
        assert torch.equal(s1, s0) and torch.equal(i1, i0) and st["prefilter"] == mode
        sd = idx.state_dict()
        assert set(sd) == {"dim", "embeds"} and torch.equal(sd["embeds"], exact.state_dict()["embeds"])
        idx2 = retrieval.EmbeddingIndex(96, dev, prefilter=mode)
        idx2.load_state_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in sd.items()})
        s2, i2 = idx2.search(q, 20, candidates=21)
        assert torch.equal(s2, s0) and torch.equal(i2, i0)
        assert torch.equal(idx2._norm, idx._norm)


def test_large_gallery_and_side_stream(dev):
    Ny, P = 1 << 22, 512                                             # Ny * P = 2^31 elements
    g = torch.Generator(device=dev).manual_seed(15)
    y = torch.randn(Ny, P, generator=g, device=dev)
    y.div_(y.norm(dim=1, keepdim=True))
    planted = torch.tensor([(1 << 22) - 1, (1 << 21) + 5, 3, (1 << 22) - 64], device=dev)
    x = torch.cat([y[planted] + 0.05 * _unit(torch.randn(4, P, generator=g, device=dev)),
                   _unit(torch.randn(60, P, generator=g, device=dev))])
    try:
        s0, i0 = retrieval.topk(x, y, 5)
        assert torch.equal(i0[:4, 0], planted)
        for mode in MODES:
            idx = retrieval.EmbeddingIndex(P, dev, prefilter=mode)
            idx.add(y)
            s1, i1, st = idx.search(x, 5, return_stats=True)
            assert torch.equal(s1, s0) and torch.equal(i1, i0), (mode, st)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                s2, i2 = idx.search(x, 5)
            torch.cuda.current_stream().wait_stream(side)
            assert torch.equal(s2, s0) and torch.equal(i2, i0)
            del idx
            gc.collect()
            torch.cuda.empty_cache()
    finally:
        del y, x
        gc.collect()
        torch.cuda.empty_cache()
