"""CPU: the host side of the k-nearest-neighbour graph (clip_dplm_amd.neighbors) and of the two scores on it
(mixing.kbet, mixing.lisi_knn): argument errors before any device work, the restatements of tests/knn_ref.py against
scikit-learn, the f64 glue on host graphs against the references, and the round loop of knn_graph driven through a torch
restatement of ops.sim_knn."""
import math

import numpy as np
import pytest
import torch

import knn_ref as ref

F64 = torch.float64


def _grid(n, P, g):
    return torch.randint(-3, 4, (n, P), generator=g).float() / 4


# ------------------------------------------------------------------------------------------------ argument errors
def test_every_argument_error_of_neighbors(monkeypatch):
    import clip_dplm_amd
    from clip_dplm_amd import neighbors, ops

    def boom():
        raise AssertionError("the device library was touched")
    monkeypatch.setattr(ops, "_lib", boom)
    assert clip_dplm_amd.knn_graph is neighbors.knn_graph and clip_dplm_amd.neighbors is neighbors
    x, y = torch.zeros(100, 8), torch.zeros(50, 8)
    bad = [
        (dict(x=[[0.0] * 8] * 100, k=5), "tensor"), (dict(x=x.double(), k=5), "float32"), (dict(x=torch.zeros(100), k=5), "2-D"),
        (dict(x=torch.zeros(100, 6), k=5), "multiple of 4"), (dict(x=torch.zeros(0, 8), k=5), "non-empty"),
        (dict(x=x, k=5, y=y.double()), "float32"), (dict(x=x, k=5, y=torch.zeros(50, 12)), "columns"),
        (dict(x=x, k=5, y=torch.zeros(50, 6)), "multiple of 4"),
        (dict(x=x, k=0), "k must"), (dict(x=x, k=100), "k must"), (dict(x=x, k=5.0), "k must"), (dict(x=x, k=True), "k must"),
        (dict(x=x, k=51, y=y), "k must"), (dict(x=torch.zeros(2000, 4), k=1025), "k must"),
        (dict(x=x, k=5, metric="sqeuclidean"), "metric"), (dict(x=x, k=5, row_block=0), "row_block"),
        (dict(x=x, k=5, row_block=64.0), "row_block"),
        (dict(x=x, k=5), "device"), (dict(x=x, k=50, y=y), "device"),              # host clouds: there is no CPU fallback
    ]
    for kw, word in bad:
        with pytest.raises((ValueError, TypeError), match=word):
            neighbors.knn_graph(**kw)
    g = neighbors.KNNGraph(torch.zeros(4, 3, dtype=torch.int64), torch.zeros(4, 3))
    for kw, word in ((dict(labels=torch.zeros(4), num_labels=2), "integer"), (dict(labels=torch.zeros(4, 1).long(), num_labels=2), "1-D"),
                     (dict(labels=torch.zeros(4).long(), num_labels=0), "num_labels"),
                     (dict(labels=torch.zeros(4).long(), num_labels=2.0), "num_labels")):
        with pytest.raises((ValueError, TypeError), match=word):
            g.label_counts(**kw)


def test_every_argument_error_of_kbet_and_lisi_knn(monkeypatch):
    import clip_dplm_amd
    from clip_dplm_amd import mixing, neighbors, ops

    def boom():
        raise AssertionError("the device library was touched")
    monkeypatch.setattr(ops, "_lib", boom)
    assert clip_dplm_amd.kbet is mixing.kbet and clip_dplm_amd.lisi_knn is mixing.lisi_knn
    x, lab = torch.zeros(100, 8), torch.arange(100) % 3
    graph = neighbors.KNNGraph(torch.zeros(100, 20, dtype=torch.int64), torch.zeros(100, 20))
    common = [
        (dict(x=x.double()), "float32"), (dict(x=torch.zeros(100, 6)), "multiple of 4"), (dict(x=torch.zeros(100)), "2-D"),
        (dict(x=[[0.0] * 8] * 100), "tensor"), (dict(lab=lab.float()), "integer"), (dict(lab=lab[:99]), "entries"),
        (dict(lab=lab[:, None]), "1-D"), (dict(num_labels=0), "num_labels"), (dict(num_labels=3.0), "num_labels"),
        (dict(num_labels=True), "num_labels"), (dict(k=0), "k must"), (dict(k=100), "k must"), (dict(k=5.0), "k must"),
        (dict(graph=(graph.indices, graph.sqdist)), "KNNGraph"),
        (dict(graph=neighbors.KNNGraph(graph.indices.int(), graph.sqdist)), "int64"),
        (dict(graph=neighbors.KNNGraph(graph.indices, graph.sqdist[:, :5])), "int64"),
        (dict(graph=neighbors.KNNGraph(graph.indices[:50], graph.sqdist[:50])), "entries"),
        (dict(graph=graph, k=21), "exceeds"),
        (dict(), "device"),                                                   # a host cloud and no graph
    ]
    for fn, name, extra in ((mixing.kbet, "batch", [(dict(alpha=0.0), "alpha"), (dict(alpha=1), "alpha"),
                                                   (dict(alpha="0.05"), "alpha"), (dict(generator=7), "generator")]),
                            (mixing.lisi_knn, "labels", [(dict(perplexity=0.0), "perplexity"), (dict(perplexity="30"), "perplexity"),
                                                         (dict(perplexity=40.0), "neighbours"),
                                                         (dict(perplexity=0.5), "neighbours")])):
        for kw, word in common + extra:
            kw = dict(kw)
            args = {"x": kw.pop("x", x), name: kw.pop("lab", lab)}
            args.update(kw)
            with pytest.raises((ValueError, TypeError), match=word):
                fn(**args)


def test_ops_argument_errors(monkeypatch):
    from clip_dplm_amd import _ffi, ops

    def boom():
        raise AssertionError("the device library was touched")
    monkeypatch.setattr(ops, "_lib", boom)
    x, y = torch.zeros(8, 8), torch.zeros(20, 8)
    for kw, exc in ((dict(k=0), ValueError), (dict(k=65), ValueError), (dict(k=5.0), ValueError), (dict(diag_offset=-2), ValueError),
                    (dict(bias=torch.zeros(19)), ValueError), (dict(bias=torch.zeros(20, dtype=F64)), ValueError),
                    (dict(after=torch.zeros(8)), ValueError), (dict(after=(torch.zeros(8), torch.zeros(8))), ValueError),
                    (dict(after=(torch.zeros(7), torch.zeros(7).long())), ValueError),
                    (dict(x=x.double()), TypeError), (dict(y=torch.zeros(20, 12)), ValueError),
                    (dict(), _ffi.ClipkError)):                              # host tensors: no CPU fallback
        args = dict(x=x, y=y, k=5)
        args.update(kw)
        with pytest.raises(exc):
            ops.sim_knn(**args)
    idx = torch.zeros(8, 3, dtype=torch.int64)
    for kw, exc in ((dict(idx=idx.int()), ValueError), (dict(idx=idx[:7]), ValueError), (dict(idx=idx[:, :0]), ValueError),
                    (dict(idx=idx[0]), ValueError), (dict(x=x.double()), TypeError), (dict(), _ffi.ClipkError)):
        args = dict(x=x, y=y, idx=idx)
        args.update(kw)
        with pytest.raises(exc):
            ops.pair_sqdist(**args)


def test_c_entry_points_refuse_before_any_launch():
    """No device here: every refusal below is made before a kernel would be launched."""
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    BAD, UNS = -1, -2
    assert lib.clipk_sim_knn_workspace(10, 100, 64, 65) == 0 and lib.clipk_sim_knn_workspace(10, 100, 64, 0) == 0
    assert lib.clipk_sim_knn_workspace(10, 100, 6, 16) == 0 and lib.clipk_sim_knn_workspace(0, 100, 64, 16) == 0
    assert lib.clipk_sim_knn_workspace(10, 100, 64, 16) == lib.clipk_sim_topk_workspace(10, 100, 64, 16) > 0
    assert lib.clipk_sim_knn_workspace(10, 100, 64, 17) == lib.clipk_sim_topk_workspace(10, 100, 64, 64)   # no 32-slot lists
    assert lib.clipk_sim_knn_workspace(10, 5, 64, 16) > 0                   # k may exceed Ny: the tail is (-inf, -1)
    fake, big = 4096, 1 << 40
    def call(**kw):
        a = dict(X=fake, Mx=4, Y=fake, Ny=100, P=8, scale=1.0, bias=None, diag=-1, a_s=None, a_i=None, k=16, s=fake, i=fake,
                 ws=fake, wsb=big, st=None)                                 # in the order of the C arguments
        a.update(kw)
        return lib.clipk_sim_knn(*a.values())
    for kw, want in ((dict(X=None), BAD), (dict(Y=None), BAD), (dict(s=None), BAD), (dict(i=None), BAD), (dict(ws=None), BAD),
                     (dict(Mx=0), BAD), (dict(Ny=0), BAD), (dict(k=0), BAD), (dict(diag=-2), BAD), (dict(a_s=fake), BAD),
                     (dict(a_i=fake), BAD), (dict(k=65), UNS), (dict(P=6), UNS), (dict(X=fake + 4), BAD), (dict(wsb=16), BAD)):
        assert call(**kw) == want, kw
    for args, want in (((None, 4, fake, 100, 8, fake, 3, fake, None), BAD), ((fake, 4, fake, 100, 8, None, 3, fake, None), BAD),
                       ((fake, 4, fake, 100, 8, fake, 0, fake, None), BAD), ((fake, 0, fake, 100, 8, fake, 3, fake, None), BAD),
                       ((fake, 4, fake, 100, 6, fake, 3, fake, None), UNS), ((fake, 4, fake + 8, 100, 8, fake, 3, fake, None), BAD)):
        assert lib.clipk_pair_sqdist(*args) == want, args


# ------------------------------------------------------------------------------------------------ the restatements
def test_knn_ref_agrees_with_sklearn():
    from sklearn.neighbors import NearestNeighbors
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(300, 16, generator=g, dtype=F64), torch.randn(500, 16, generator=g, dtype=F64)   # no ties
    idx, d2, _ = ref.knn_graph(x, 70)
    dist, ind = NearestNeighbors(n_neighbors=71, algorithm="brute").fit(x.numpy()).kneighbors(x.numpy())
    assert (ind[:, 0] == np.arange(300)).all()
    assert np.array_equal(ind[:, 1:], idx.numpy())
    np.testing.assert_allclose(dist[:, 1:] ** 2, d2.numpy(), rtol=1e-10, atol=1e-12)
    idx, d2, _ = ref.knn_graph(x, 70, y)
    dist, ind = NearestNeighbors(n_neighbors=70, algorithm="brute").fit(y.numpy()).kneighbors(x.numpy())
    assert np.array_equal(ind, idx.numpy())
    np.testing.assert_allclose(dist ** 2, d2.numpy(), rtol=1e-10, atol=1e-12)


def test_select_cursor_and_tails():
    z = torch.tensor([[1.0, 3.0, 3.0, 2.0, 3.0, 0.0]], dtype=F64)
    s, i = ref.select(z, 3)
    assert i.tolist() == [[1, 2, 4]] and s.tolist() == [[3.0, 3.0, 3.0]]
    s, i = ref.select(z, 3, after=(torch.tensor([3.0]), torch.tensor([2])))       # inside the run of equal keys
    assert i.tolist() == [[4, 3, 0]]
    s, i = ref.select(z, 4, diag_offset=3, after=(torch.tensor([3.0]), torch.tensor([4])))
    assert i.tolist() == [[0, 5, -1, -1]] and s[0, 2:].tolist() == [-math.inf, -math.inf]
    s, i = ref.select(z, 8, after=(torch.tensor([-math.inf]), torch.tensor([-1])))
    assert (i == -1).all() and torch.isinf(s).all()


# ------------------------------------------------------------------------------------------------ the round loop
@pytest.mark.parametrize("k", [64, 65, 128, 130])
def test_round_loop_with_duplicates_across_the_boundary(monkeypatch, k):
    """knn_graph's rounds through the restated ops.sim_knn: rows 1..99 are copies of three points, so every row's 64th
    and 128th neighbour lie inside a run of equal keys, which the cursor must split without a repeat or a gap."""
    from clip_dplm_amd import neighbors, ops
    g = torch.Generator().manual_seed(k)
    x = _grid(400, 4, g)
    x[1:100] = x[torch.randint(100, 103, (99,), generator=g)]
    asked = []

    def fake(xb, ys, kk, scale=None, bias=None, diag_offset=-1, after=None):
        asked.append(kk)
        return ref.sim_knn(xb, ys, kk, scale, bias, diag_offset, after)
    monkeypatch.setattr(ops, "sim_knn", fake)
    want, _, _ = ref.knn_graph(x, k)
    for row_block in (65536, 150):
        asked.clear()
        got = neighbors._rounds(x, x, k, True, row_block)
        assert torch.equal(got, want)
        rounds = [min(64, k - c) for c in range(0, k, 64)]
        assert asked == rounds * len(range(0, 400, row_block))
    assert all(len(set(r)) == k and i not in r for i, r in enumerate(want.tolist()))
    y = _grid(300, 4, g)
    y[50:150] = y[0]
    got = neighbors._rounds(x, y, k, False, 65536)
    assert torch.equal(got, ref.knn_graph(x, k, y)[0])


# ------------------------------------------------------------------------------------------------ kBET and LISI glue
def _host_graph(n, k, seed, G, P=8):
    from clip_dplm_amd import neighbors
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, G, (n,), generator=g)
    x = torch.randn(n, P, generator=g, dtype=F64) + 1.5 * torch.randn(G, P, generator=g, dtype=F64)[lab]
    idx, d2, _ = ref.knn_graph(x, k)
    return neighbors.KNNGraph(idx, d2), lab


def test_kbet_on_a_host_graph_agrees_with_scipy():
    from clip_dplm_amd import mixing
    graph, lab = _host_graph(400, 40, 1, 4)
    lab5 = lab.clone()
    lab5[lab5 >= 2] += 1                                                       # label 2 of 0..4 has no points
    for labels, num_labels, G in ((lab * 7 - 3, None, 4), (lab, 4, 4), (lab5, 5, 5)):
        r = mixing.kbet(None, labels, graph=graph, num_labels=num_labels)
        stat, p, rate = ref.kbet_ref(graph.indices, (lab5 if G == 5 else lab).numpy(), G)
        assert r.k == 40 and int(r.dof) == 3 and r.expected_rejection_rate is None
        np.testing.assert_allclose(r.stat.numpy(), stat, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(r.pvalue.numpy(), p, rtol=1e-12, atol=1e-12)
        assert float(r.rejection_rate) == rate and float(r.acceptance) == 1 - rate
    r = mixing.kbet(None, lab, graph=graph, k=25, alpha=0.2, generator=torch.Generator().manual_seed(5))
    sub = graph.indices[:, :25]
    stat, p, rate = ref.kbet_ref(sub, lab.numpy(), 4, alpha=0.2)
    np.testing.assert_allclose(r.pvalue.numpy(), p, rtol=1e-12, atol=1e-12)
    perm = torch.randperm(400, generator=torch.Generator().manual_seed(5))
    _, _, rate_p = ref.kbet_ref(sub, lab[perm].numpy(), 4, alpha=0.2)
    assert r.k == 25 and float(r.rejection_rate) == rate and float(r.expected_rejection_rate) == rate_p
    assert rate_p < rate                                                       # blobs by label: the real labels are rejected


@pytest.mark.parametrize("perplexity", [5.0, 30.0])
def test_lisi_knn_on_a_host_graph_agrees_with_the_loop(perplexity):
    from clip_dplm_amd import mixing, neighbors
    graph, lab = _host_graph(300, 89, 2, 3)
    d2 = graph.sqdist.clone()
    d2[0] = 2.25                                                               # all-equal distances: H = log k at every beta
    d2[1] = 1e7                                                                # exp(-beta d) underflows: sum P == 0, H = 0
    d2[2, :] = torch.linspace(0.0, 4.0, 89, dtype=F64) ** 2                    # a zero distance (an equal other row)
    graph = neighbors.KNNGraph(graph.indices, d2)
    for labels, num_labels in ((lab * 3 + 1, None), (lab, 3)):
        got = mixing.lisi_knn(None, labels, perplexity=perplexity, graph=graph, num_labels=num_labels)
        want = ref.lisi_knn_ref(d2.sqrt().numpy(), lab[graph.indices].numpy(), 3, perplexity)
        assert got.dtype == torch.float32 and got.shape == (300,)
        assert got[1] == -1.0 and want[1] == -1.0
        np.testing.assert_allclose(got.double().numpy(), want, rtol=2.0 ** -24, atol=1e-9)      # 1e-9, and the f32 result's rounding
    got64 = mixing._lisi_knn_f64(graph, lab[graph.indices], 3, perplexity)
    np.testing.assert_allclose(got64.numpy(), want, rtol=0, atol=1e-9)
    k20 = mixing.lisi_knn(None, lab, perplexity=5.0, graph=graph, k=20, num_labels=3)
    want = ref.lisi_knn_ref(d2[:, :20].sqrt().numpy(), lab[graph.indices[:, :20]].numpy(), 3, 5.0)
    np.testing.assert_allclose(k20.double().numpy(), want, rtol=2.0 ** -24, atol=1e-9)


def test_label_counts():
    from clip_dplm_amd import neighbors
    g = neighbors.KNNGraph(torch.tensor([[1, 2, 3], [0, 0, -1]]), torch.zeros(2, 3))
    lab = torch.tensor([0, 2, 2, 5])
    assert g.label_counts(lab, 3).tolist() == [[0, 0, 2], [2, 0, 0]]
    assert g.k == 3 and torch.equal(g.distances, torch.zeros(2, 3))
