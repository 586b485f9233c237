"""GPU: the resumable biased top-k walk (include/clipk.h: clipk_sim_knn), the distances of listed pairs
(clipk_pair_sqdist), the k-nearest-neighbour graph on top of them (clip_dplm_amd/neighbors.py) and the two scores on the
graph (mixing.kbet, mixing.lisi_knn), against the restatements of tests/knn_ref.py.

Order contract: z = fl(fl(scale s) + bias) descending, equal z by the lower key index; a key is eligible when it is not the
row's own (i + diag_offset) and lies strictly after the cursor in that order; unfilled slots are (-inf, -1)."""
import math

import numpy as np
import pytest
import torch

import knn_ref as ref
from clip_dplm_amd import mixing, neighbors, ops

pytestmark = pytest.mark.gpu
F64 = torch.float64


def _grid(n, P, g, dev):
    """Entries in {-3..3}/4: every f32 product, partial sum and -|y|^2 / 2 is exact, so z equals the f64 value."""
    return (torch.randint(-3, 4, (n, P), generator=g).float() / 4).to(dev)


def _window(full_s, full_i, start, k):
    """Columns [start_i, start_i + k) of each row of the full sorted lists, (-inf, -1) past their end."""
    M = full_s.shape[0]
    s = torch.cat([full_s, torch.full((M, k), -math.inf, dtype=full_s.dtype, device=full_s.device)], 1)
    i = torch.cat([full_i, torch.full((M, k), -1, dtype=full_i.dtype, device=full_i.device)], 1)
    cols = start[:, None] + torch.arange(k, device=full_s.device)[None, :]
    return s.gather(1, cols).float(), i.gather(1, cols)


# ------------------------------------------------------------------------------------------------ 1: grid inputs, bit for bit
@pytest.mark.parametrize("P", [4, 60, 512])
@pytest.mark.parametrize("Ny", [63, 65, 4097])
def test_grid_inputs_bit_for_bit(dev, kopt, P, Ny):
    g = torch.Generator().manual_seed(P * 11 + Ny)
    scale = 0.5                                                    # a power of two: fl(scale s) stays exact
    x_all, y = _grid(1000, P, g, dev), _grid(Ny, P, g, dev)
    src = torch.randint(0, Ny, (Ny // 8,), generator=g).to(dev)    # duplicated gallery rows: exact ties by construction
    dst = torch.randint(0, Ny, (Ny // 8,), generator=g).to(dev)
    y[dst] = y[src]
    bias_all = -0.5 * (y * y).sum(1)
    inside_a_run = 0
    for bias in (bias_all, None):
        z_all = ref.scores(x_all, y, scale, bias)
        for Mx in (1, 63, 65, 1000):
            x = x_all[:Mx].contiguous()
            for diag in sorted({-1, 0, Ny - Mx} - set(range(-Mx, -1))):
                full_s, full_i = ref.select(z_all[:Mx], Ny, diag)                 # every eligible key, in order
                n_elig = (full_i >= 0).sum(1)
                entry = torch.tensor([0, 5, 63], device=dev)[torch.arange(Mx, device=dev) % 3]
                entry = torch.minimum(entry, n_elig - 1)                           # Ny = 63: the last eligible key
                late = n_elig - 4                                                  # past all but 3 keys
                nxt = (entry + 1).clamp(max=Ny - 1)[:, None]
                inside_a_run += int((full_s.gather(1, entry[:, None]) == full_s.gather(1, nxt)).sum())
                cursors = [(None, torch.zeros(Mx, dtype=torch.int64, device=dev))]
                for e in (entry, late):
                    after = (full_s.gather(1, e[:, None])[:, 0].float().contiguous(), full_i.gather(1, e[:, None])[:, 0].contiguous())
                    cursors.append((after, e + 1))
                for k in (1, 7, 12, 30, 64):                        # 12, 30: the 16-slot lists; 17 .. 64 share the 64-slot ones
                    for after, start in cursors:
                        want_s, want_i = _window(full_s, full_i, start, k)
                        if after is cursors[2][0]:
                            assert (want_i[:, 3:] == -1).all() and (want_i[:, :min(k, 3)] >= 0).all()
                        for splits in (1, 2, 5, 1000):
                            kopt("retrieval_splits", splits)
                            s, i = ops.sim_knn(x, y, k, scale=scale, bias=bias, diag_offset=diag, after=after)
                            what = (P, Ny, Mx, k, diag, bias is not None, after is not None, splits)
                            assert torch.equal(i, want_i), what
                            assert torch.equal(s, want_s), what
    assert inside_a_run > 0                                        # some cursor sat inside a run of equal keys


# ------------------------------------------------------------------------------------------------ 2: the plain form
@pytest.mark.parametrize("k", [10, 64])
def test_plain_form_has_the_bits_of_sim_topk(dev, k):
    g = torch.Generator().manual_seed(k)
    x = torch.nn.functional.normalize(torch.randn(300, 120, generator=g), dim=1).to(dev)
    y = torch.nn.functional.normalize(torch.randn(5000, 120, generator=g), dim=1).to(dev)
    for scale in (None, 14.3):
        s0, i0 = ops.sim_topk(x, y, k, scale=scale)
        s1, i1 = ops.sim_knn(x, y, k, scale=scale)
        assert torch.equal(i0, i1) and torch.equal(s0, s1)


# ------------------------------------------------------------------------------------------------ 3: knn_graph, many equal points
@pytest.fixture(scope="module")
def grid_cloud(dev):
    g = torch.Generator().manual_seed(3)
    x = _grid(1000, 4, g, dev)                                     # 7^4 = 2401 possible points: equal rows and many ties
    y = _grid(1000, 4, g, dev)
    return x, y, ref.knn_graph(x, 200), ref.knn_graph(x[:300], 200, y)


@pytest.mark.parametrize("k", [64, 65, 130, 200])
def test_knn_graph_on_a_grid_cloud(dev, grid_cloud, k):
    x, y, (idx, d2, _), (idx_y, d2_y, _) = grid_cloud
    got = neighbors.knn_graph(x, k)
    assert got.indices.dtype == torch.int64 and got.sqdist.dtype == torch.float32
    assert torch.equal(got.indices, idx[:, :k])
    assert torch.equal(got.sqdist, d2[:, :k].float())              # exact sums: bit for bit
    assert torch.equal(got.distances, got.sqdist.sqrt())
    own = torch.arange(1000, device=dev)[:, None]
    assert not (got.indices == own).any()
    assert (got.indices.sort(1).values.diff(dim=1) > 0).all()      # no key twice
    blocked = neighbors.knn_graph(x, k, row_block=256)
    assert torch.equal(blocked.indices, got.indices) and torch.equal(blocked.sqdist, got.sqdist)
    two = neighbors.knn_graph(x[:300], k, y=y)
    assert torch.equal(two.indices, idx_y[:, :k]) and torch.equal(two.sqdist, d2_y[:, :k].float())


# ------------------------------------------------------------------------------------------------ 4: random clouds against f64
def _unit_cloud():
    g = torch.Generator().manual_seed(41)
    v = torch.randn(1500, 64, generator=g, dtype=F64)
    return (v / v.norm(dim=1, keepdim=True)).float(), 130


def _blob_cloud():
    g = torch.Generator().manual_seed(42)
    centres = torch.randn(4, 32, generator=g, dtype=F64)
    return (centres[torch.arange(1200) % 4] + 0.5 * torch.randn(1200, 32, generator=g, dtype=F64)).float(), 89


@pytest.mark.parametrize("cloud", [_unit_cloud, _blob_cloud])
def test_random_clouds_against_f64(dev, cloud):
    """A window test, every row: random inputs do have near-ties (rows whose k-th gap in f64 lies inside w_i), so set
    equality is not asked.  w_i = 2 (P + 2) 2^-24 (|x_i| max_j |x_j| + max_j |b_j|): the forward bound of the two roundings
    and a P-term f32 sum, on both sides of a comparison."""
    x, k = cloud()
    x = x.to(dev)
    N, P = x.shape
    got = neighbors.knn_graph(x, k)
    idx = got.indices
    own = torch.arange(N, device=dev)[:, None]
    assert not (idx == own).any() and (idx.sort(1).values.diff(dim=1) > 0).all() and ((idx >= 0) & (idx < N)).all()
    xd = x.double()
    b = -0.5 * (xd * xd).sum(1)
    z = xd @ xd.t() + b[None, :]
    norm = xd.norm(dim=1)
    w = 2 * (P + 2) * 2.0 ** -24 * (norm * norm.max() + b.abs().max())
    zr = z.gather(1, idx)
    left = z.clone()
    left.scatter_(1, idx, -math.inf)
    left.scatter_(1, own, -math.inf)
    slack_out = (left.max(1).values - zr.min(1).values) / w
    slack_up = (zr[:, 1:] - zr[:, :-1]).max(1).values / w
    d2 = ref.pair_sqdist(x, x, idx)
    rel = ((got.sqdist.double() - d2).abs() / d2).max()
    print(f"{cloud.__name__}: left-out over window {float(slack_out.max()):.3f}  rise over window {float(slack_up.max()):.3f}  "
          f"sqdist rel err {float(rel):.3e} (bound {(P + 3) * 2.0 ** -24:.3e})")
    assert (slack_out <= 1).all()                                  # no key left out beats the weakest returned one
    assert (slack_up <= 1).all()                                   # the returned z never rises by more than the window
    assert ((got.sqdist.double() - d2).abs() <= (P + 3) * 2.0 ** -24 * d2).all()


# ------------------------------------------------------------------------------------------------ 5: kBET and LISI on the device
@pytest.fixture(scope="module")
def two_blobs(dev):
    """Two grid blobs 100 apart along the first axis (all arithmetic exact, so the device graph is the reference's)."""
    g = torch.Generator().manual_seed(5)
    x = _grid(600, 8, g, "cpu")
    x[300:, 0] += 100.0
    k = 40
    idx, d2, _ = ref.knn_graph(x, k)
    return x.to(dev), k, idx, d2


def test_kbet_on_the_device(dev, two_blobs):
    x, k, idx, d2 = two_blobs
    graph = neighbors.knn_graph(x, k)
    assert torch.equal(graph.indices.cpu(), idx) and torch.equal(graph.sqdist.cpu(), d2.float())
    blob = (torch.arange(600) >= 300).long()
    r = mixing.kbet(x, blob.to(dev), k=k)
    stat, p, rate = ref.kbet_ref(idx, blob.numpy(), 2)
    np.testing.assert_allclose(r.pvalue.cpu().numpy(), p, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r.stat.cpu().numpy(), stat, rtol=1e-12, atol=1e-12)
    assert float(r.rejection_rate) == 1.0 == rate and float(r.acceptance) == 0.0 and r.k == k and int(r.dof) == 1
    alt = torch.arange(600) % 2
    r = mixing.kbet(x, (alt * 5 + 2).to(dev), graph=graph, generator=torch.Generator(device=dev).manual_seed(1))
    stat, p, rate = ref.kbet_ref(idx, alt.numpy(), 2)
    np.testing.assert_allclose(r.pvalue.cpu().numpy(), p, rtol=1e-12, atol=1e-12)
    assert float(r.rejection_rate) == rate and rate < 0.5 and 0.0 <= float(r.expected_rejection_rate) < 0.5
    auto = mixing.kbet(x, blob.to(dev))                            # k = floor(300 / 4) = 75
    assert auto.k == 75 and float(auto.rejection_rate) == 1.0


@pytest.mark.parametrize("perplexity", [5.0, 13.0])
def test_lisi_knn_on_the_device(dev, two_blobs, perplexity):
    x, k, idx, d2 = two_blobs
    kk = int(3 * perplexity) - 1
    for lab in ((torch.arange(600) >= 300).long(), torch.arange(600) % 3):
        got = mixing.lisi_knn(x, (lab * 2 + 1).to(dev), perplexity=perplexity)
        want = ref.lisi_knn_ref(d2[:, :kk].sqrt().numpy(), lab[idx[:, :kk]].numpy(), 3, perplexity)
        assert got.dtype == torch.float32 and got.shape == (600,)
        graph = neighbors.knn_graph(x, kk)
        got64 = mixing._lisi_knn_f64(graph, lab.to(dev)[graph.indices], 3, perplexity)
        err = float((got64.cpu() - torch.from_numpy(want)).abs().max())
        print(f"perplexity {perplexity}: max |LISI - reference| = {err:.3e}")
        assert err <= 1e-9
        np.testing.assert_allclose(got.double().cpu().numpy(), want, rtol=2.0 ** -24, atol=1e-9)     # + the f32 result's rounding
    assert float(want.min()) >= 1.0 and float(want.max()) > 2.0    # i % 3 mixes; the blob label above gave exactly 1


# ------------------------------------------------------------------------------------------------ 6: graph capture
def test_graph_capture(dev, grid_cloud):
    x = grid_cloud[0]
    lab = (torch.arange(1000) % 3).to(dev)
    eager = neighbors.knn_graph(x, 130)
    eager_lisi = mixing.lisi_knn(x, lab, perplexity=30.0, num_labels=3)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        neighbors.knn_graph(x, 130)
        mixing.lisi_knn(x, lab, perplexity=30.0, num_labels=3)
    torch.cuda.current_stream().wait_stream(side)
    graph, keep = torch.cuda.CUDAGraph(), []
    with ops.owned_by_capture(keep), torch.cuda.graph(graph):      # one stream, no parallel branches
        out = neighbors.knn_graph(x, 130)
        out_lisi = mixing.lisi_knn(x, lab, perplexity=30.0, num_labels=3)
    for _ in range(2):
        out.indices.fill_(-7)
        out.sqdist.fill_(-1.0)
        out_lisi.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.indices, eager.indices) and torch.equal(out.sqdist, eager.sqdist)
        assert torch.equal(out_lisi, eager_lisi)
