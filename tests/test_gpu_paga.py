"""GPU: clipk_knn_label_pairs against the loops of tests/paga_ref.py - exact equality on both paths and across the boundary
between them - and clip_dplm_amd.paga on device clouds: the counts of the device graph, the formulas against their
numpy restatement, the tree, graph capture, and modularity on a device SymGraph against the host."""
import numpy as np
import pytest
import torch

import paga_ref as ref
from clip_dplm_amd import diffusion, neighbors, ops, paga
from clip_dplm_amd.neighbors import KNNGraph

pytestmark = pytest.mark.gpu
F64 = torch.float64
EPS = 2.0 ** -52
I32 = (-2 ** 31, 2 ** 31 - 1)


def _labels(rng, n, G):
    """int32 [n] drawn from [-1, G], with the int32 extremes among them where there is room."""
    lab = rng.integers(-1, G + 1, n).astype(np.int32)
    if n >= 8:
        lab[rng.integers(0, n, 2)] = I32
    return lab


def _case(rng, M, k, G, separate):
    Ny = M // 2 + 3 if separate else M
    idx = rng.integers(-1, Ny + 1, (M, k))                                 # -1 and Ny: both invalid ends
    rl = _labels(rng, M, G)
    kl = _labels(rng, Ny, G) if separate else None
    return idx, rl, kl


# ------------------------------------------------------------------------------------------------ 1: the kernel, exactly
@pytest.mark.parametrize("G", [1, 2, 37, 128, 129, 1024])
def test_kernel_equals_the_loops(dev, G):
    """G <= 128 runs the LDS-table kernel, G >= 129 the wave-merging one; M and k around the wave, the workgroup's stride
    and the 64-column rounds of the graph, key labels of the rows and of another cloud of another length."""
    rng = np.random.default_rng(G)
    for M in (1, 63, 65, 1000):
        for k in (1, 14, 64, 65, 130):
            idx, rl, kl = _case(rng, M, k, G, separate=(M + k) % 2 == 1)
            want = ref.counts_ref(idx, rl, G, kl)
            got = ops.knn_label_pairs(torch.from_numpy(idx).to(dev), torch.from_numpy(rl).to(dev), G,
                                      None if kl is None else torch.from_numpy(kl).to(dev))
            assert got.dtype == torch.int64 and got.shape == (G, G)
            assert np.array_equal(got.cpu().numpy(), want), (M, k, G)
            if M == 1000:
                assert want.sum() > 0


@pytest.mark.parametrize("G", [37, 129])
def test_out_is_added_into_and_offset_operands(dev, G):
    rng = np.random.default_rng(5 + G)
    M, k = 1000, 14
    idx, rl, kl = _case(rng, M, k, G, separate=True)
    want = ref.counts_ref(idx, rl, G, kl)
    before = rng.integers(0, 2 ** 40, (G, G))
    out = torch.from_numpy(before.copy()).to(dev)
    d_idx, d_rl, d_kl = torch.from_numpy(idx).to(dev), torch.from_numpy(rl).to(dev), torch.from_numpy(kl).to(dev)
    got = ops.knn_label_pairs(d_idx, d_rl, G, d_kl, out=out)
    assert got is out and np.array_equal(out.cpu().numpy(), before + want)
    ops.knn_label_pairs(d_idx, d_rl, G, d_kl, out=out)
    assert np.array_equal(out.cpu().numpy(), before + 2 * want)
    # operands that start 4 bytes (the labels) and 8 bytes (the indices) into their buffers
    o_rl = torch.cat([d_rl[:1], d_rl])[1:]
    o_kl = torch.cat([d_kl[:3], d_kl])[3:]
    o_idx = torch.cat([d_idx.reshape(-1)[:1], d_idx.reshape(-1)])[1:].reshape(M, k)
    assert o_rl.data_ptr() % 8 == 4 and o_kl.data_ptr() % 8 == 4 and o_idx.data_ptr() % 16 == 8
    assert o_rl.is_contiguous() and o_idx.is_contiguous() and o_rl.storage_offset() == 1
    assert np.array_equal(ops.knn_label_pairs(o_idx, o_rl, G, o_kl).cpu().numpy(), want)


@pytest.mark.parametrize("G", [1, 37, 128, 129, 1024])
def test_one_label_takes_every_count(dev, G):
    """The worst contention: 4096 x 64 = 262144 counts into one bin."""
    M, k = 4096, 64
    idx = torch.from_numpy(np.random.default_rng(1).integers(0, M, (M, k))).to(dev)
    label = G // 2
    want = np.zeros((G, G), np.int64)
    want[label, label] = M * k
    got = ops.knn_label_pairs(idx, torch.full((M,), label, dtype=torch.int32, device=dev), G)
    assert np.array_equal(got.cpu().numpy(), want)


def test_no_dependence_on_the_path(dev):
    """Labels in [0, 100) counted with G = 128 (LDS table) and with G = 129 (wave merging): the same [100, 100] corner,
    zeros elsewhere; the blob order of a real graph (most neighbours share the row's label) and a random one."""
    rng = np.random.default_rng(7)
    M, k = 3000, 30
    clustered = np.sort(rng.integers(0, 100, M)).astype(np.int32)
    near = np.clip(np.arange(M)[:, None] + rng.integers(-40, 41, (M, k)), 0, M - 1)
    for lab, idx in ((clustered, near), (rng.integers(0, 100, M).astype(np.int32), rng.integers(0, M, (M, k)))):
        d_idx, d_lab = torch.from_numpy(idx).to(dev), torch.from_numpy(lab).to(dev)
        a, b = ops.knn_label_pairs(d_idx, d_lab, 128), ops.knn_label_pairs(d_idx, d_lab, 129)
        assert torch.equal(a[:100, :100], b[:100, :100]) and int(a.sum()) == int(b.sum()) == M * k
        assert int(a[:100, :100].sum()) == M * k and int(b[:100, :100].sum()) == M * k
        assert np.array_equal(a[:100, :100].cpu().numpy(), ref.counts_ref(idx, lab, 100))


# ------------------------------------------------------------------------------------------------ 2: paga on a device cloud
@pytest.fixture(scope="module")
def chain(dev):
    x, lab = ref.blob_chain(0)
    x, lab = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    return x, lab, neighbors.knn_graph(x, 14)


def _within_ulps(got, want, n):
    return (np.abs(got - want) <= n * np.spacing(np.abs(want))).all()


def test_paga_on_a_device_cloud(dev, chain):
    """The counts are those of the loops on the device graph's own indices.  expected and connectivities hold two f64
    divisions, each at most 1 ulp off if the device's division were not correctly rounded: within 2 ulp of numpy.  The
    division IS correctly rounded and equality is what is expected - the 2 ulp are what the test may claim without
    knowing that."""
    x, lab, g = chain
    res = paga.paga(x, lab, num_groups=5)
    C = ref.counts_ref(g.indices.cpu().numpy(), lab.cpu().numpy(), 5)
    ns, expected, conn = ref.paga_ref(C, lab.cpu().numpy(), 5)
    assert res.counts.is_cuda and np.array_equal(res.counts.cpu().numpy(), C) and int(C.sum()) == 600 * 14
    assert np.array_equal(res.sizes.cpu().numpy(), ns) and res.k == 14 and res.num_groups == 5
    assert _within_ulps(res.expected.cpu().numpy(), expected, 2)
    assert _within_ulps(res.connectivities.cpu().numpy(), conn, 2)
    assert torch.equal(res.connectivities, res.connectivities.T) and not res.connectivities.diagonal().any()
    assert res.tree.is_cuda and ref.tree_edges(res.tree.cpu().numpy()) == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert np.array_equal(res.tree.cpu().numpy(), ref.tree_ref(res.connectivities.cpu().numpy()))
    same = paga.paga(g, lab, num_groups=5)                                 # the graph given: the same bits
    relabelled = paga.paga(x, 3 * lab.cpu() - 4)                           # host labels, torch.unique
    for other in (same, relabelled):
        assert torch.equal(other.counts, res.counts) and torch.equal(other.expected, res.expected)
        assert torch.equal(other.connectivities, res.connectivities) and torch.equal(other.tree, res.tree)
    # the device graph through the kernel and its host copy through bincount
    host = paga.group_edge_counts(KNNGraph(g.indices.cpu(), g.sqdist.cpu()), lab.cpu(), 5)
    assert torch.equal(paga.group_edge_counts(g, lab, 5).cpu(), host)
    # label transfer against an atlas: the graph of x against a part of itself, key labels over that part
    gy = neighbors.knn_graph(x, 10, y=x[100:500].contiguous())
    got = paga.group_edge_counts(gy, lab, 5, key_labels=lab[100:500])
    assert np.array_equal(got.cpu().numpy(), ref.counts_ref(gy.indices.cpu().numpy(), lab.cpu().numpy(), 5, lab[100:500].cpu().numpy()))
    pres = paga.paga_preservation(x, g, lab)
    assert abs(float(pres.spearman) - 1.0) <= 4 * EPS and float(pres.tree_jaccard) == 1.0


# ------------------------------------------------------------------------------------------------ 3: graph capture
def test_graph_capture(dev, chain):
    _, lab, g = chain
    labels = lab.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        paga.paga(g, labels, num_groups=5, tree=False)
    torch.cuda.current_stream().wait_stream(side)
    graph, keep = torch.cuda.CUDAGraph(), []
    with ops.owned_by_capture(keep), torch.cuda.graph(graph):              # one stream, no parallel branches
        out = paga.paga(g, labels, num_groups=5, tree=False)
    assert out.tree is None
    perm = torch.from_numpy(np.random.default_rng(2).permutation(600)).to(dev)
    idx = g.indices.cpu().numpy()
    for new in (lab, lab[perm], (lab + 2) % 5):
        labels.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        C = ref.counts_ref(idx, new.cpu().numpy(), 5)
        ns, expected, conn = ref.paga_ref(C, new.cpu().numpy(), 5)
        assert np.array_equal(out.counts.cpu().numpy(), C) and np.array_equal(out.sizes.cpu().numpy(), ns)
        assert _within_ulps(out.expected.cpu().numpy(), expected, 2) and _within_ulps(out.connectivities.cpu().numpy(), conn, 2)


# ------------------------------------------------------------------------------------------------ 4: modularity
def test_modularity_device_against_host(dev, chain):
    _, lab, g = chain
    sg = diffusion.connectivities(g)
    host = diffusion.SymGraph(sg.indptr.cpu(), sg.indices.cpu(), sg.weights.cpu())
    # the order of a device bincount is not fixed: in_c, tot_c and W are sums of at most nnz non-negative weights, each
    # within nnz eps relative of exact in any order; Q is then within (10 nnz + 8 + G) eps for resolution <= 2 on either
    # side (tests/test_paga_host.py has the steps): twice that between the two
    bound = 2 * (10 * sg.nnz + 8 + 5) * EPS
    for labels in (lab, (lab * 7 + torch.arange(600, device=dev)) % 5, torch.where(lab == 2, torch.full_like(lab, -1), lab)):
        for resolution in (1.0, 0.0, 2.0):
            got = paga.modularity(sg, labels, 5, resolution=resolution)
            assert got.is_cuda and got.dtype == F64 and got.dim() == 0
            assert abs(float(got) - float(paga.modularity(host, labels.cpu(), 5, resolution=resolution))) <= bound
    assert float(paga.modularity(sg, lab, 5)) > 0.05
