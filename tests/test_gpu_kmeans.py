"""GPU: the fused Lloyd step (include/clipk.h: clipk_kmeans_step; ops.kmeans_step) and clip_dplm_amd.cluster on top
of it against the restatement of tests/kmeans_ref.py.

Labels are compared exactly wherever the f64 restatement's decision is not a near-tie: a point whose f64 margin (best
score minus runner-up) is below tau_i = 4 (P + 2) 2^-24 (|x_i| c_max + c_max^2) - twice the rounding of one f32 score: a
P-term dot product, the f32 norm, one fma - may go either way; at most 1 % of a case's points may be excused so.
Real-valued outputs follow `_close`, the rule of tests/test_gpu_mmd.py: at most 8 x the deviation of the f32 restatement
from the f64 one, with a floor of 64 * 2^-24 x the quantity's magnitude.  Counts and sums are checked against the labels
THE KERNEL returned, so a flipped near-tie cannot hide a wrong sum.  Measured deviations are printed before each
assertion."""
import functools

import numpy as np
import pytest
import torch

from clip_dplm_amd import cluster, ops

import kmeans_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F64, F32 = torch.float64, torch.float32
SEP = 0.5                                           # one-step cases: blobs that overlap, so that margins of every size occur


def _close(name, got, r64, r32):
    got, r64, r32 = (torch.as_tensor(t).detach().double().cpu() for t in (got, r64, r32))
    assert got.shape == r64.shape, (name, got.shape, r64.shape)
    assert torch.isfinite(got).all(), name
    dev_k, dev_32 = float((got - r64).abs().max()), float((r32 - r64).abs().max())
    mag = float(r64.abs().max())
    bound = max(8 * dev_32, 64 * U * mag)
    print(f"{name}: kernel {dev_k:.3e}  f32 restatement {dev_32:.3e}  magnitude {mag:.3e}  bound {bound:.3e}  "
          f"ratio {dev_k / bound if bound else 0.0:.3f}")
    assert dev_k <= bound, (name, dev_k, bound)


@functools.lru_cache(maxsize=None)
def _step_case(N, K, P):
    """x [N, P] from K overlapping blobs and K distinct rows of the cloud as centroids (drawn from max(N, K) rows where
    the cloud is smaller than K), with the f64 / f32 restatement of the assignment.  Computed once per shape."""
    M = max(N, K)
    pts, _, _ = ref.blobs(M, P, K, SEP, 1000 * N + 10 * K + P)
    c = pts[np.random.default_rng(N + K + P).choice(M, K, replace=False)]
    x = pts[:N]
    l64, b64, m64 = ref.assign(x.astype(np.float64), c.astype(np.float64))
    _, b32, _ = ref.assign(x, c)
    c_max = float(np.sqrt((c.astype(np.float64) ** 2).sum(1)).max())
    tau = 4 * (P + 2) * U * (np.sqrt((x.astype(np.float64) ** 2).sum(1)) * c_max + c_max ** 2)
    return x, c, l64, b64, b32, m64 < tau


def _check_sums(name, x, K, labels_k, sums, counts):
    """counts == the bincount of the labels given, exactly; sums against the f64 segmented sums under those labels."""
    lab = labels_k.cpu().numpy().astype(np.int64)
    s64, n64 = ref.segmented(x.astype(np.float64), lab, K)
    s32, _ = ref.segmented(x, lab, K)
    assert counts.dtype == F32 and np.array_equal(counts.cpu().numpy().astype(np.int64), n64), name
    _close(name, sums, s64, s32)


# ------------------------------------------------------------------------------------------------ 1: one step, fused mode
@pytest.mark.parametrize("P", [4, 60, 512])
@pytest.mark.parametrize("K", [1, 2, 10, 64])
@pytest.mark.parametrize("N", [1, 63, 65, 4097])
def test_fused_step(dev, N, K, P):
    x, c, l64, b64, b32, near = _step_case(N, K, P)
    xd, cd = torch.from_numpy(x).to(dev), torch.from_numpy(c).to(dev)
    labels, best, sums, counts = ops.kmeans_step(xd, cd)
    assert labels.dtype == torch.int32 and labels.shape == (N,) and sums.shape == (K, P) and counts.shape == (K,)
    if N == 4097:
        assert ops.kmeans_step_plan(N, K)[1] > 1                    # the point range is split
    lab = labels.cpu().numpy().astype(np.int64)
    assert lab.min() >= 0 and lab.max() < K
    print(f"near-ties excused: {int(near.sum())} of {N}")
    assert near.sum() <= 0.01 * N
    assert np.array_equal(lab[~near], l64[~near])
    _close("best", best, b64, b32)
    _check_sums("sums", x, K, labels, sums, counts)
    again = ops.kmeans_step(xd, cd)                                 # two runs: the same bits
    for a, b in zip((labels, best, sums, counts), again):
        assert torch.equal(a, b)
    # the norms given equal the norms computed here
    given = ops.kmeans_step(xd, cd, nc=(cd * cd).sum(1))
    for a, b in zip((labels, best, sums, counts), given):
        assert torch.equal(a, b)


def test_fused_step_cosine_form(dev):
    """nc = zeros: the arg max of <x, c> alone."""
    x, c, *_ = _step_case(4097, 10, 60)
    xd, cd = torch.from_numpy(x).to(dev), torch.from_numpy(c).to(dev)
    labels, best, sums, counts = ops.kmeans_step(xd, cd, nc=torch.zeros(10, device=dev))
    zeros = np.zeros(10)
    l64, b64, m64 = ref.assign(x.astype(np.float64), c.astype(np.float64), zeros)
    _, b32, _ = ref.assign(x, c, zeros.astype(np.float32))
    c_max = float(np.sqrt((c.astype(np.float64) ** 2).sum(1)).max())
    near = m64 < 4 * 62 * U * np.sqrt((x.astype(np.float64) ** 2).sum(1)) * c_max
    assert near.sum() <= 0.01 * 4097
    assert np.array_equal(labels.cpu().numpy()[~near], l64[~near])
    _close("best (cosine form)", best, b64, b32)
    _check_sums("sums (cosine form)", x, 10, labels, sums, counts)


# ------------------------------------------------------------------------------------------------ 2: one step, labels given
def _given_labels(kind, N, K, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, K, N)
    if kind == "sparse":                            # every third cluster only: the others have no point
        return 3 * rng.integers(0, (K + 2) // 3, N) if K > 1 else np.zeros(N, dtype=np.int64)
    return np.full(N, K - 1)                        # all one cluster, the last


@pytest.mark.parametrize("kind", ["random", "sparse", "one"])
@pytest.mark.parametrize("P", [60, 512])
@pytest.mark.parametrize("K", [1, 64, 65, 200])
def test_labels_given_step(dev, K, P, kind):
    N = 1031
    x = _step_case(4097, 10, P)[0][:N]
    lab = np.minimum(_given_labels(kind, N, K, K + P), K - 1).astype(np.int32)
    xd, ld = torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev)
    cd = torch.zeros(K, P, device=dev)              # only its shape is used
    labels, best, sums, counts = ops.kmeans_step(xd, cd, labels=ld)
    assert labels is ld and best is None
    _check_sums(f"sums ({kind})", x, K, ld, sums, counts)
    if kind != "random" and K > 1:
        assert (counts == 0).any()                  # clusters without a point are among the cases
    again = ops.kmeans_step(xd, cd, labels=ld)
    assert torch.equal(sums, again[2]) and torch.equal(counts, again[3])


@pytest.mark.parametrize("K", [1, 10, 64])
@pytest.mark.parametrize("N", [63, 4097])
def test_labels_given_equals_fused(dev, N, K):
    """K <= 64: the same grid, the same one-hot tiles, the same order of every sum - the same bits."""
    x, c, *_ = _step_case(N, K, 60)
    xd, cd = torch.from_numpy(x).to(dev), torch.from_numpy(c).to(dev)
    labels, _, sums, counts = ops.kmeans_step(xd, cd)
    _, _, sums_g, counts_g = ops.kmeans_step(xd, cd, labels=labels)
    assert torch.equal(sums, sums_g) and torch.equal(counts, counts_g)


def test_labels_outside_the_range_join_no_cluster(dev):
    x = _step_case(63, 10, 60)[0]
    lab = np.arange(63, dtype=np.int32) % 12 - 1    # -1 and 10 among them
    xd = torch.from_numpy(x).to(dev)
    _, _, sums, counts = ops.kmeans_step(xd, torch.zeros(10, 60, device=dev), labels=torch.from_numpy(lab).to(dev))
    keep = (lab >= 0) & (lab < 10)
    s64, n64 = ref.segmented(x[keep].astype(np.float64), lab[keep].astype(np.int64), 10)
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), n64)
    _close("sums (labels outside the range dropped)", sums, s64, ref.segmented(x[keep], lab[keep].astype(np.int64), 10)[0])


# ------------------------------------------------------------------------------------------------ 3: exact ties, duplicates
@pytest.mark.parametrize("t", [0, 1, 15, 16, 17, 31, 32, 33, 48, 63])
def test_exact_ties_go_to_the_lower_index(dev, t):
    """64 centroids that differ in coordinate 0 only, points with x[0] = 0: the products <x, c_k> are the same bits for
    every k (the term of coordinate 0 is +-0), so the score depends on |c_k|^2 alone.  Centroids below t are longer
    (c[0] = +-2), the others (c[0] = +-1) tie exactly: every point goes to t, across the 16-centroid scan parts and the
    two lane halves."""
    rng = np.random.default_rng(t)
    N, P = 70, 8
    x = rng.standard_normal((N, P)).astype(np.float32)
    x[:, 0] = 0
    c = np.tile(rng.standard_normal((1, P)).astype(np.float32), (64, 1))
    c[:, 0] = np.where(np.arange(64) % 2 == 0, 1.0, -1.0) * np.where(np.arange(64) < t, 2.0, 1.0)
    labels, best, sums, counts = ops.kmeans_step(torch.from_numpy(x).to(dev), torch.from_numpy(c).to(dev))
    assert (labels == t).all()
    want = torch.zeros(64, device=dev)
    want[t] = N
    assert torch.equal(counts, want) and (sums[torch.arange(64, device=dev) != t] == 0).all()
    assert torch.isfinite(best).all()


def test_duplicate_centroid_stays_empty(dev):
    """Two identical centroids: the higher one gets no point, keeps its value, and is counted in n_empty.  Its twin's
    cluster is 20 copies of one point with small integer coordinates, whose mean is that point exactly - so the twin
    never moves away and the pair stays identical through the fit."""
    x, _, centres = ref.blobs(300, 8, 3, 4.0, 17)
    v = np.array([40, -40, 40, -40, 40, -40, 40, -40], dtype=np.float32)
    x = np.concatenate([x, np.tile(v, (20, 1))])
    init = np.stack([centres[0], v, centres[1], v, centres[2]])
    xd, cd = torch.from_numpy(x).to(dev), torch.from_numpy(init).to(dev)
    labels, _, _, counts = ops.kmeans_step(xd, cd)
    assert counts[3] == 0 and counts[1] == 20 and (labels[300:] == 1).all()
    res = cluster.kmeans(xd, 5, init=cd)
    assert torch.equal(res.centroids[3], cd[3]) and torch.equal(res.centroids[1], cd[1])
    assert res.n_empty == 1 and res.counts[3] == 0 and res.counts.sum() == 320 and res.converged
    assert not (res.labels == 3).any()


# ------------------------------------------------------------------------------------------------ 4: full fit
@functools.lru_cache(maxsize=None)
def _fit_case(N, P, K, seed):
    """Well-separated blobs (sep = 4), K distinct rows as the init, and the restatement's fit in f64 and f32."""
    x, truth, centres = ref.blobs(N, P, K, 4.0, seed)
    init = x[np.random.default_rng(seed + 1).choice(N, K, replace=False)]
    r64 = ref.fit(x.astype(np.float64), init.astype(np.float64))
    r32 = ref.fit(x, init)
    return x, truth, centres, init, r64, r32


@pytest.mark.parametrize("N,P,K", [(1000, 32, 10), (4133, 132, 10), (3001, 64, 200)])
def test_full_fit(dev, N, P, K):
    """tol = 0 stops at the fixed point only (no label changed, or no centroid moved), where the restatement stops too:
    the labels are compared exactly.  K = 200 takes the two-launch path."""
    x, truth, centres, init, r64, r32 = _fit_case(N, P, K, N + K)
    assert r64.converged and np.array_equal(r64.labels, r32.labels)  # the inputs are fit for an exact comparison
    xd = torch.from_numpy(x).to(dev)
    res = cluster.kmeans(xd, K, init=torch.from_numpy(init).to(dev), tol=0.0)
    assert res.converged and res.n_iter < 300
    assert res.labels.dtype == torch.int64 and np.array_equal(res.labels.cpu().numpy(), r64.labels)
    _close("centroids", res.centroids, r64.centroids, r32.centroids)
    _close("inertia", res.inertia, r64.inertia, r32.inertia)
    # inertia = the sum of d2_min = max(|x|^2 - best, 0) of a step against the returned centroids
    if K <= 64:
        _, best, _, _ = ops.kmeans_step(xd, res.centroids)
        d2 = ((xd * xd).sum(1) - best).clamp_min(0)
        _close("sum of d2_min", d2.sum(), r64.d2.sum(), r32.d2.sum())
    assert np.array_equal(res.counts.cpu().numpy(), r64.counts) and int(res.n_empty) == r64.n_empty
    assert torch.equal(res.predict(xd), res.labels)
    # the default stopping rule (tol = 1e-4 of the variance) converges as well
    assert cluster.kmeans(xd, K, init=torch.from_numpy(init).to(dev)).converged


def test_fit_from_the_true_centres(dev):
    x, truth, centres, *_ = _fit_case(1000, 32, 10, 1010)
    xd = torch.from_numpy(x).to(dev)
    res = cluster.kmeans(xd, 10, init=torch.from_numpy(centres).to(dev))
    assert res.converged and cluster.adjusted_rand_index(res.labels, torch.from_numpy(truth).to(dev)) == 1.0
    assert cluster.normalized_mutual_info(res.labels.cpu(), torch.from_numpy(truth)) > 1 - 1e-12
    # seeded k-means++ with restarts finds the same partition, and is reproducible
    a = cluster.kmeans(xd, 10, n_init=5, generator=torch.Generator().manual_seed(0))
    b = cluster.kmeans(xd, 10, n_init=5, generator=torch.Generator().manual_seed(0))
    assert torch.equal(a.labels, b.labels) and torch.equal(a.centroids, b.centroids)
    assert cluster.adjusted_rand_index(a.labels, res.labels) == 1.0 and float(a.inertia) <= float(res.inertia) * (1 + 1e-5)


def test_cosine_metric(dev):
    x, truth, centres, *_ = _fit_case(1000, 32, 10, 1010)
    xu = torch.nn.functional.normalize(torch.from_numpy(x), dim=1).to(dev)
    res = cluster.kmeans(xu, 10, init=torch.from_numpy(centres).to(dev), metric="cosine")
    assert res.converged and res.metric == "cosine"
    assert ((res.centroids.double().norm(dim=1) - 1).abs() <= 8 * U).all()
    assert cluster.adjusted_rand_index(res.labels, torch.from_numpy(truth).to(dev)) == 1.0
    assert torch.equal(res.predict(xu), res.labels)
    # the labels are the arg max of the cosine, and the inertia is sum |x - c|^2 on the unit sphere
    cos = xu.double() @ res.centroids.double().T
    assert torch.equal(cos.argmax(1), res.labels)
    want = (2 - 2 * cos.max(1).values).sum()
    assert abs(float(res.inertia) - float(want)) <= 64 * U * 2 * 1000


# ------------------------------------------------------------------------------------------------ 5: graph capture
def test_fixed_iteration_fit_is_capturable(dev):
    """tol=None: no host read anywhere, so five iterations and the final assignment are one chain of launches in a graph;
    replayed on new inputs copied into the captured buffers it gives the eager call's bits."""
    x0, _, _, i0, _, _ = _fit_case(1000, 32, 10, 1010)
    x1, _, _ = ref.blobs(1000, 32, 10, 4.0, 77)
    i1 = x1[:10].copy()
    sx, sc = torch.from_numpy(x0).to(dev), torch.from_numpy(i0).to(dev)

    def run():
        r = cluster.kmeans(sx, 10, init=sc, tol=None, max_iter=5)
        assert r.n_iter == 5 and r.converged is False
        return r.centroids, r.labels, r.inertia, r.counts, r.n_empty

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph, keep = torch.cuda.CUDAGraph(), []
    with ops.owned_by_capture(keep), torch.cuda.graph(graph):
        out = run()
    for xs, cs in ((x1, i1), (x0, i0)):
        sx.copy_(torch.from_numpy(xs).to(dev))
        sc.copy_(torch.from_numpy(cs).to(dev))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in out]
        e = cluster.kmeans(torch.from_numpy(xs).to(dev), 10, init=torch.from_numpy(cs).to(dev), tol=None, max_iter=5)
        for got, want in zip(replayed, (e.centroids, e.labels, e.inertia, e.counts, e.n_empty)):
            assert torch.equal(got, want)
    assert float(out[2]) > 0


# ------------------------------------------------------------------------------------------------ 6: cluster_agreement
def test_cluster_agreement(dev):
    """Two clouds from one latent labeling - the second a rotation of the first plus small noise - cluster alike; with
    the rows of the second shuffled the two labelings are independent."""
    x, truth, _ = ref.blobs(1200, 32, 6, 4.0, 23)
    rng = np.random.default_rng(24)
    q, _ = np.linalg.qr(rng.standard_normal((32, 32)))
    y = (x.astype(np.float64) @ q + 0.05 * rng.standard_normal(x.shape)).astype(np.float32)
    a, b = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    kw = dict(n_init=5, generator=torch.Generator().manual_seed(0))
    out = cluster.cluster_agreement(a, b, n_clusters=6, **kw)
    assert set(out) == {"ari", "nmi"} and all(isinstance(v, float) for v in out.values())
    assert out["ari"] > 0.99 and out["nmi"] > 0.99
    perm = torch.from_numpy(rng.permutation(1200)).to(dev)
    shuffled = cluster.cluster_agreement(a, b[perm], n_clusters=6, **kw)
    assert abs(shuffled["ari"]) < 0.05
    with_labels = cluster.cluster_agreement(a, b, n_clusters=6, labels=torch.from_numpy(truth), **kw)
    assert set(with_labels) == {"ari", "nmi", "ari_a_vs_labels", "nmi_a_vs_labels", "ari_b_vs_labels", "nmi_b_vs_labels"}
    assert with_labels["ari_a_vs_labels"] > 0.99 and with_labels["ari_b_vs_labels"] > 0.99
