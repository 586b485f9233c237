"""CPU: clip_dplm_amd.paga without a device - every argument error before any device work, the exports and the library's
new symbol, and the torch glue (host counts, the PAGA formulas, Kruskal's forest, modularity, preservation) on host
graphs against the loops of tests/paga_ref.py."""
import numpy as np
import pytest
import torch

import paga_ref as ref

F64 = torch.float64
EPS = 2.0 ** -52


def _host_graph(x, k):
    from clip_dplm_amd.neighbors import KNNGraph
    idx, d2 = ref.knn_host(x, k)
    return KNNGraph(torch.from_numpy(idx), torch.from_numpy(d2))


@pytest.fixture(scope="module")
def chains():
    """seed -> (cloud, labels, host KNNGraph of 14 other rows, reference counts) of the five-blob chain."""
    out = {}
    for seed in range(3):
        x, lab = ref.blob_chain(seed)
        g = _host_graph(x, 14)
        out[seed] = (x, lab, g, ref.counts_ref(g.indices.numpy(), lab, 5))
    return out


# ------------------------------------------------------------------------------------------------ argument errors
def test_every_argument_error_before_any_device_work(monkeypatch):
    import clip_dplm_amd
    from clip_dplm_amd import diffusion, ops, paga
    from clip_dplm_amd.neighbors import KNNGraph

    def boom():
        raise AssertionError("the device library was touched")
    monkeypatch.setattr(ops, "_lib", boom)
    assert clip_dplm_amd.paga is paga and "paga" in clip_dplm_amd.__all__
    for name in ("group_edge_counts", "connectivities_tree", "modularity", "paga_preservation", "PAGAResult",
                 "PAGAPreservation"):
        assert getattr(clip_dplm_amd, name) is getattr(paga, name) and name in clip_dplm_amd.__all__ and name in paga.__all__
    assert paga.MAX_GROUPS == ops.LABEL_PAIRS_MAX_G == 1024
    x = torch.zeros(100, 8)
    lab = torch.zeros(100, dtype=torch.int64)
    g = KNNGraph(torch.zeros(100, 14, dtype=torch.int64), torch.zeros(100, 14))
    cross = KNNGraph(torch.zeros(10, 12, dtype=torch.int64), torch.zeros(10, 12))      # k > N - 1: not against itself
    bad = [
        (dict(x_or_graph=[[0.0] * 8] * 100), "tensor"), (dict(x_or_graph=x.double()), "float32"),
        (dict(x_or_graph=torch.zeros(100)), "2-D"), (dict(x_or_graph=torch.zeros(100, 6)), "multiple of 4"),
        (dict(x_or_graph=x, metric="sqeuclidean"), "metric"),
        (dict(x_or_graph=x, n_neighbors=1), "n_neighbors"), (dict(x_or_graph=x, n_neighbors=101), "n_neighbors"),
        (dict(x_or_graph=x, n_neighbors=15.0), "n_neighbors"),
        (dict(x_or_graph=torch.zeros(2000, 4), groups=torch.zeros(2000, dtype=torch.int64), n_neighbors=1026), "n_neighbors"),
        (dict(x_or_graph=x, groups=lab.double()), "integer"), (dict(x_or_graph=x, groups=[0] * 100), "integer"),
        (dict(x_or_graph=x, groups=lab == 0), "integer"), (dict(x_or_graph=x, groups=lab[:99]), "99 entries for 100 rows"),
        (dict(x_or_graph=x, groups=lab.reshape(10, 10)), "1-D"),
        (dict(x_or_graph=g, groups=lab[:50]), "50 entries for 100 rows"),
        (dict(x_or_graph=x, num_groups=0), "num_groups"), (dict(x_or_graph=x, num_groups=1025), "num_groups"),
        (dict(x_or_graph=x, num_groups=3.0), "num_groups"), (dict(x_or_graph=x, num_groups=True), "num_groups"),
        (dict(x_or_graph=x, tree=1), "tree"),
        (dict(x_or_graph=cross, groups=lab[:10]), "against itself"),
        (dict(x_or_graph=KNNGraph(torch.zeros(10, 3, dtype=torch.int32), torch.zeros(10, 3)), groups=lab[:10]), "int64"),
        (dict(x_or_graph=x), "device"),                                               # a host cloud: no CPU search
    ]
    for kw, word in bad:
        with pytest.raises((ValueError, TypeError), match=word):
            paga.paga(**{"groups": lab, **kw})
    bad = [
        (dict(graph=x), "KNNGraph"), (dict(graph=KNNGraph(g.indices, torch.zeros(100, 3))), "int64 indices"),
        (dict(labels=lab[:7]), "7 entries for 100 rows"), (dict(labels=lab.float()), "integer"),
        (dict(num_groups=0), "num_groups"), (dict(num_groups=1025), "num_groups"), (dict(num_groups=2.0), "num_groups"),
        (dict(key_labels=lab.float()), "key_labels"), (dict(key_labels=lab[:0]), "empty"),
        (dict(key_labels=lab.reshape(4, 25)), "1-D"),
    ]
    for kw, word in bad:
        with pytest.raises((ValueError, TypeError), match=word):
            paga.group_edge_counts(**{"graph": g, "labels": lab, "num_groups": 4, **kw})
    for conn in (torch.zeros(3, 3), torch.zeros(3, 4, dtype=F64), torch.zeros(3, dtype=F64), [[0.0]], torch.zeros(0, 0, dtype=F64)):
        with pytest.raises(ValueError, match="conn must"):
            paga.connectivities_tree(conn)
    sg = diffusion.SymGraph(torch.zeros(101, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=F64))
    bad = [
        (dict(graph=g), "SymGraph"), (dict(graph=diffusion.SymGraph(sg.indptr.int(), sg.indices, sg.weights)), "SymGraph"),
        (dict(graph=diffusion.SymGraph(sg.indptr, sg.indices, torch.zeros(3, dtype=F64))), "SymGraph"),
        (dict(labels=lab[:99]), "99 entries for 100 rows"), (dict(labels=lab.float()), "integer"),
        (dict(num_groups=0), "num_groups"), (dict(num_groups=1025), "num_groups"),
        (dict(resolution=-0.5), "resolution"), (dict(resolution="1"), "resolution"), (dict(resolution=True), "resolution"),
        (dict(resolution=float("inf")), "resolution"), (dict(resolution=float("nan")), "resolution"),
    ]
    for kw, word in bad:
        with pytest.raises((ValueError, TypeError), match=word):
            paga.modularity(**{"graph": sg, "labels": lab, "num_groups": 4, **kw})
    lab3 = torch.arange(100) % 3
    bad = [
        (dict(groups=torch.arange(100) % 2), "at least 3 groups"), (dict(groups=lab3, num_groups=2), "at least 3 groups"),
        (dict(groups=lab3, n_comps=3), "unexpected"), (dict(groups=lab3[:9]), "9 entries for 100 rows"),
        (dict(x_b=KNNGraph(torch.zeros(90, 14, dtype=torch.int64), torch.zeros(90, 14)), groups=lab3), "100 entries for 90 rows"),
        (dict(x_a=x, groups=lab3), "device"), (dict(x_b=x, groups=lab3), "device"),
        (dict(groups=lab3, n_neighbors=0, x_a=x), "n_neighbors"),
    ]
    for kw, word in bad:
        with pytest.raises((ValueError, TypeError), match=word):
            paga.paga_preservation(**{"x_a": g, "x_b": g, **kw})


def test_ops_argument_errors(monkeypatch):
    from clip_dplm_amd import _ffi, ops

    def boom():
        raise AssertionError("the device library was touched")
    monkeypatch.setattr(ops, "_lib", boom)
    idx = torch.zeros(10, 3, dtype=torch.int64)
    lab = torch.zeros(10, dtype=torch.int32)
    good = dict(idx=idx, row_labels=lab, num_groups=4)
    bad = [
        (dict(idx=idx.int()), "idx must"), (dict(idx=idx[:, 0]), "idx must"), (dict(idx=idx.T.contiguous().T), "idx must"),
        (dict(idx=idx[:0]), "idx must"), (dict(idx=torch.zeros(2, 1025, dtype=torch.int64), row_labels=lab[:2]), "k <= 1024"),
        (dict(idx=[[0]]), "idx must"),
        (dict(row_labels=lab.long()), "row_labels must"), (dict(row_labels=lab[:9]), "row_labels must"),
        (dict(row_labels=torch.zeros(20, dtype=torch.int32)[::2]), "row_labels must"),
        (dict(key_labels=lab.long()), "key_labels must"), (dict(key_labels=lab[:0]), "key_labels must"),
        (dict(key_labels=lab.reshape(2, 5)), "key_labels must"),
        (dict(num_groups=0), "num_groups"), (dict(num_groups=1025), "num_groups"), (dict(num_groups=4.0), "num_groups"),
        (dict(out=torch.zeros(4, 4, dtype=torch.int32)), "out must"), (dict(out=torch.zeros(4, 5, dtype=torch.int64)), "out must"),
        (dict(out=torch.zeros(4, 8, dtype=torch.int64)[:, ::2]), "out must"),
    ]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            ops.knn_label_pairs(**{**good, **kw})
    with pytest.raises(_ffi.ClipkError, match="device"):                  # host tensors: there is no CPU fallback
        ops.knn_label_pairs(**good)


def test_library_exports_the_entry_point():
    """The symbol with its signature, the ABI version unchanged, and every refusal before any launch."""
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    assert lib.clipk_version() == 7 == _ffi.ABI_VERSION
    assert hasattr(lib, "clipk_knn_label_pairs") and len(_ffi.SIGNATURES["clipk_knn_label_pairs"][1]) == 9
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data
    ok = dict(idx=p, M=4, k=2, row_labels=p, key_labels=p, Ny=4, G=2, counts=p, stream=None)

    def call(**kw):
        return lib.clipk_knn_label_pairs(*{**ok, **kw}.values())
    for name in ("idx", "row_labels", "key_labels", "counts"):
        assert call(**{name: None}) == -1
    assert call(M=0) == -1 and call(Ny=0) == -1 and call(k=0) == -1 and call(k=1025) == -1 and call(G=0) == -1
    assert call(G=1025) == -2


# ------------------------------------------------------------------------------------------------ counts on host graphs
def test_host_counts_equal_the_loops():
    from clip_dplm_amd import paga
    from clip_dplm_amd.neighbors import KNNGraph
    rng = np.random.default_rng(0)
    M, Ny, k, G = 57, 41, 6, 5
    idx = rng.integers(-1, Ny + 1, (M, k))                                 # both invalid ends: -1 and Ny
    rl = rng.integers(-1, G + 1, M)                                        # and labels -1 and G
    kl = rng.integers(-1, G + 1, Ny)
    rl[:2], kl[:2] = (2 ** 40, -2 ** 40), (2 ** 31, -2 ** 31 - 1)          # beyond int32
    assert (idx == -1).any() and (idx == Ny).any() and (rl == G).any() and (kl == -1).any()
    g = KNNGraph(torch.from_numpy(idx), torch.zeros(M, k))
    got = paga.group_edge_counts(g, torch.from_numpy(rl), G, torch.from_numpy(kl))
    assert got.dtype == torch.int64 and got.shape == (G, G)
    assert np.array_equal(got.numpy(), ref.counts_ref(idx, rl, G, kl))
    # the labels of the rows for both ends: indices at or beyond M count nowhere
    idx2 = rng.integers(-1, M + 1, (M, k))
    g2 = KNNGraph(torch.from_numpy(idx2), torch.zeros(M, k))
    got2 = paga.group_edge_counts(g2, torch.from_numpy(rl), G)
    assert np.array_equal(got2.numpy(), ref.counts_ref(idx2, rl, G)) and 0 < int(got2.sum()) < M * k
    # G = 1 and a table with an empty label
    assert paga.group_edge_counts(g2, torch.zeros(M, dtype=torch.int64), 1).tolist() == [[int(((idx2 >= 0) & (idx2 < M)).sum())]]
    got3 = paga.group_edge_counts(g2, torch.from_numpy(rl % 3).int(), 7)               # int32 labels too
    assert np.array_equal(got3.numpy(), ref.counts_ref(idx2, rl % 3, 7)) and int(got3[3:].sum()) == 0


# ------------------------------------------------------------------------------------------------ the PAGA formulas
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_paga_formulas_bit_for_bit_and_recovered_topology(chains, seed):
    """Host torch and numpy do the same three IEEE operations (a conversion and two divisions): equal bits.  The five blobs
    lie on a line, 3.0 apart with unit noise: the tree is the chain, chain edges are strong, every other pair is weak."""
    from clip_dplm_amd import paga
    x, lab, g, C = chains[seed]
    ns, expected, conn = ref.paga_ref(C, lab, 5)
    res = paga.paga(g, torch.from_numpy(lab), num_groups=5)
    assert res.num_groups == 5 and res.k == 14
    assert np.array_equal(res.counts.numpy(), C) and np.array_equal(res.sizes.numpy(), ns) and ns.tolist() == list(ref.BLOB_SIZES)
    assert res.expected.dtype == F64 and np.array_equal(res.expected.numpy(), expected)
    assert res.connectivities.dtype == F64 and np.array_equal(res.connectivities.numpy(), conn)
    assert np.array_equal(conn, conn.T) and (np.diag(conn) == 0).all() and (np.diag(expected) == 0).all()
    assert (expected[~np.eye(5, dtype=bool)] > 0).all()                    # every off-diagonal pair has its expectation
    # the topology, in numpy
    chain = [(a, a + 1) for a in range(4)]
    assert ref.tree_edges(ref.tree_ref(conn)) == chain
    assert all(conn[a, b] >= 0.46 for a, b in chain)
    assert all(conn[a, b] <= 0.04 for a in range(5) for b in range(a + 2, 5))
    assert (conn == 1).any() and ((conn > 0) & (conn < 1)).any()           # saturated values and values in between
    # and the package's tree
    assert np.array_equal(res.tree.numpy(), ref.tree_ref(conn)) and ref.tree_edges(res.tree.numpy()) == chain
    assert paga.paga(g, torch.from_numpy(lab), num_groups=5, tree=False).tree is None
    # torch.unique relabels: any integer values, in ascending order
    relabelled = paga.paga(g, torch.from_numpy(10 * lab - 7))
    assert relabelled.num_groups == 5 and torch.equal(relabelled.connectivities, res.connectivities)
    assert torch.equal(relabelled.tree, res.tree)


def test_out_of_range_groups_are_no_part_of_n(chains):
    from clip_dplm_amd import paga
    _, lab, g, _ = chains[0]
    lab = lab.copy()
    lab[::7] = -1
    lab[3::11] = 5
    C = ref.counts_ref(g.indices.numpy(), lab, 5)
    ns, expected, conn = ref.paga_ref(C, lab, 5)
    res = paga.paga(g, torch.from_numpy(lab), num_groups=5, tree=False)
    assert int(res.sizes.sum()) == int(((lab >= 0) & (lab < 5)).sum()) < 600
    assert np.array_equal(res.counts.numpy(), C) and np.array_equal(res.sizes.numpy(), ns)
    assert np.array_equal(res.expected.numpy(), expected) and np.array_equal(res.connectivities.numpy(), conn)
    # a single labelled row: n - 1 = 0 divides nothing
    one = np.full(600, -1)
    one[17] = 2
    res = paga.paga(g, torch.from_numpy(one), num_groups=5)
    assert int(res.counts.sum()) == 0 and not res.expected.any() and not res.connectivities.any() and not res.tree.any()


# ------------------------------------------------------------------------------------------------ the forest
def test_tree_tie_rule_and_total_weight():
    from clip_dplm_amd import paga
    rng = np.random.default_rng(4)
    G = 9
    conn = np.triu(rng.uniform(0.05, 0.95, (G, G)), 1)
    conn[rng.uniform(size=(G, G)) < 0.3] = 0.0
    conn[0, 1] = conn[0, 2] = conn[1, 2] = conn[2, 3] = conn[1, 3] = conn[4, 5] = 1.0    # deliberate ties at the cap
    conn[6, 7] = conn[6, 8] = conn[7, 8] = 0.5                                             # and a tied triangle below it
    conn[:6, 6:] = 0.0                                                                     # two components: a forest
    conn = conn + conn.T
    want = ref.tree_ref(conn)
    got = paga.connectivities_tree(torch.from_numpy(conn))
    assert got.dtype == F64 and np.array_equal(got.numpy(), want) and np.array_equal(want, want.T)
    edges = ref.tree_edges(want)
    # the tie rule: among equal weights the pair that comes first in (a, b) order joins: (1, 2) closes a cycle, (1, 3)
    # comes before (2, 3) and takes node 3
    assert (0, 1) in edges and (0, 2) in edges and (1, 3) in edges and (1, 2) not in edges and (2, 3) not in edges
    assert (6, 7) in edges and (6, 8) in edges and (7, 8) not in edges
    assert len(edges) == G - 2                                             # two components
    scipy_graph = pytest.importorskip("scipy.sparse.csgraph")
    from scipy.sparse import csr_matrix
    inv = np.where(conn > 0, 1.0 / np.where(conn > 0, conn, 1.0), 0.0)
    mst = scipy_graph.minimum_spanning_tree(csr_matrix(np.triu(inv)))
    assert abs(sum(1.0 / want[a, b] for a, b in edges) - mst.sum()) <= 1e-12 * mst.sum()


# ------------------------------------------------------------------------------------------------ modularity
def test_modularity_on_host_graphs(chains):
    from clip_dplm_amd import diffusion, paga
    _, lab, g, _ = chains[0]
    sg = diffusion.connectivities(g)
    W = sg.to_dense().numpy()
    labels = torch.from_numpy(lab)
    # in_c, tot_c and W are sums of at most nnz non-negative weights in some order: each within nnz eps relative.  in_c / W
    # is then within (2 nnz + 1) eps and (tot_c / W)^2 within (4 nnz + 3) eps; the in_c / W sum to at most 1 and so do the
    # squares, so Q is within ((2 nnz + 1) + resolution (4 nnz + 3) + G) eps <= (10 nnz + 8 + G) eps for resolution <= 2.
    # The dense loops of the reference carry the same bound: twice that between the two.
    bound = 2 * (10 * sg.nnz + 8 + 5) * EPS
    for res in (1.0, 0.5, 2.0):
        q = paga.modularity(sg, labels, 5, resolution=res)
        assert q.dtype == F64 and q.dim() == 0
        assert abs(float(q) - ref.modularity_ref(W, lab, 5, res)) <= bound
    q = float(paga.modularity(sg, labels, 5))
    assert q > 0.05                                                        # positive, and outside the band of a random labelling
    perm = torch.from_numpy(np.random.default_rng(1).permutation(lab))
    assert abs(float(paga.modularity(sg, perm, 5))) < 0.05                 # a random labelling: about 0
    inside = W[lab[:, None] == lab[None, :]].sum() / W.sum()
    assert abs(float(paga.modularity(sg, labels, 5, resolution=0)) - inside) <= bound
    # labels outside [0, G) leave their rows and columns out
    cut = lab.copy()
    cut[::5] = 9
    assert abs(float(paga.modularity(sg, torch.from_numpy(cut), 5)) - ref.modularity_ref(W, cut, 5)) <= bound


# ------------------------------------------------------------------------------------------------ preservation
def test_preservation_of_a_graph_with_itself(chains):
    from clip_dplm_amd import paga
    _, lab, g, _ = chains[0]
    res = paga.paga_preservation(g, g, torch.from_numpy(lab))
    assert float(res.spearman) == 1.0 and float(res.tree_jaccard) == 1.0 and res.spearman.dtype == F64
    # against another cloud of the same chain the tree is the same chain; against a shuffled one it is not
    g1 = chains[1][2]
    res = paga.paga_preservation(g, g1, torch.from_numpy(lab), num_groups=5)
    assert float(res.tree_jaccard) == 1.0 and float(res.spearman) > 0.8
    with pytest.raises(ValueError, match="at least 3 groups"):
        paga.paga_preservation(g, g, torch.from_numpy(lab // 3))
