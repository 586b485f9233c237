"""CPU: the restatement of tests/silhouette_ref.py against itself and against sklearn, the f64 glue of
clip_dplm_amd.cluster's centroid-based scores on host tensors, every argument error of the labeling scores and of
ops.label_dist_sums raised with no device present, and the C ABI of clipk_label_dist_sums as far as it goes without one."""
import numpy as np
import pytest
import torch

import kmeans_ref
import silhouette_ref as ref


def _labelings(N, seed):
    """(name, labels): blob labels, random labels, a singleton cluster, non-contiguous label values."""
    x, truth, _ = kmeans_ref.blobs(N, 8, 5, 2.0, seed)
    rng = np.random.default_rng(seed + 1)
    rand = rng.integers(0, 7, N)
    single = truth.copy()
    single[3] = 9                                   # a cluster of one point
    sparse = 10 * truth - 7                         # values -7, 3, 13, ...
    return x, (("blobs", truth), ("random", rand), ("singleton", single), ("non-contiguous", sparse))


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("metric", ref.METRICS)
def test_restated_sums_two_forms_agree(metric):
    x, _, _ = kmeans_ref.blobs(90, 12, 4, 1.0, 7)
    x = x.astype(np.float64)
    if metric == "cosine":
        x = ref.normalize(x)
    lab = np.random.default_rng(0).integers(-1, 6, 90)           # -1 and 5 belong to no column of G = 5
    for off, q in ((0, x), (-1, x), (20, x[20:50])):
        a = ref.label_dist_sums(q, x, lab, 5, metric, off)
        b = ref.label_dist_sums_direct(q, x, lab, 5, metric, off)
        assert a.shape == (len(q), 5) and np.abs(a - b).max() <= 1e-9 * np.abs(b).max()
    # the dropped term: with the diagonal kept the own column grows by exactly the formula's value at j == i
    keep = ref.label_dist_sums(x, x, lab, 5, metric, -1) - ref.label_dist_sums(x, x, lab, 5, metric, 0)
    own = np.where((lab >= 0) & (lab < 5))[0]
    assert np.abs(keep[own, lab[own]] - ref.diagonal_terms(x, metric)[own]).max() < 1e-9
    # a literal double loop at one row
    i, want = 11, np.zeros(5)
    for j in range(90):
        if j != i and 0 <= lab[j] < 5:
            want[lab[j]] += ref.distances_direct(x[i:i + 1], x[j:j + 1], metric)[0, 0]
    assert np.abs(ref.label_dist_sums_direct(x, x, lab, 5, metric, 0)[i] - want).max() < 1e-10


def test_restated_silhouette_by_hand():
    """Four points on a line, two clusters: a, b and s follow by hand."""
    x = np.array([[0.0], [1.0], [4.0], [6.0]])
    s = ref.silhouette_samples(x, [0, 0, 1, 1])
    a, b = np.array([1, 1, 2, 2.0]), np.array([5, 4, 3.5, 5.5])
    assert np.allclose(s, (b - a) / np.maximum(a, b), rtol=0, atol=1e-15)
    assert np.array_equal(ref.silhouette_samples(x, [0, 0, 0, 1])[3:], [0.0])        # alone in its cluster


@pytest.mark.parametrize("N", [40, 131])
def test_restatement_matches_sklearn(N):
    metrics = pytest.importorskip("sklearn.metrics")
    x, labelings = _labelings(N, N)
    x = x.astype(np.float64)
    for name, lab in labelings:
        for metric in ("euclidean", "sqeuclidean", "cosine"):
            want = metrics.silhouette_samples(x, lab, metric=metric)
            for direct in (False, True):
                got = ref.silhouette_samples(x, lab, metric, direct)
                assert np.abs(got - want).max() <= 1e-10, (name, metric, direct)
        assert abs(ref.davies_bouldin(x, lab) - metrics.davies_bouldin_score(x, lab)) <= 1e-10, name
        want = metrics.calinski_harabasz_score(x, lab)
        assert abs(ref.calinski_harabasz(x, lab) - want) <= 1e-10 * want, name
        values, means, counts = ref.silhouette_by_label(x, lab)
        s = metrics.silhouette_samples(x, lab)
        assert np.array_equal(values, np.unique(lab)) and counts.sum() == N
        assert all(abs(means[g] - s[lab == v].mean()) <= 1e-10 for g, v in enumerate(values))


# ------------------------------------------------------------------------------------------------ the f64 glue on host tensors
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_centroid_scores_on_host_tensors(dtype):
    from clip_dplm_amd import cluster
    x, labelings = _labelings(131, 3)
    xt = torch.from_numpy(x).to(dtype)
    x = x.astype(np.float64)                        # the glue works in f64 whatever the host dtype
    for name, lab in labelings:
        lt = torch.from_numpy(lab)
        db, ch = cluster.davies_bouldin_score(xt, lt), cluster.calinski_harabasz_score(xt, lt)
        assert isinstance(db, float) and isinstance(ch, float)
        assert abs(db - ref.davies_bouldin(x, lab)) <= 1e-12 * max(db, 1), name
        assert abs(ch - ref.calinski_harabasz(x, lab)) <= 1e-12 * ch, name
        assert cluster.davies_bouldin_score(xt, lt.int()) == db                      # any integer dtype


def test_centroid_scores_degenerate_conventions():
    """sklearn's: coincident centroids are left out of Davies-Bouldin's maximum, all-zero spreads give 0, a zero
    within-cluster dispersion gives Calinski-Harabasz 1."""
    from clip_dplm_amd import cluster
    x = torch.tensor([[0.0, 0], [2, 0], [1, 1], [1, -1], [9, 0], [11, 0]], dtype=torch.float64)
    lab = torch.tensor([0, 0, 1, 1, 2, 2])                      # clusters 0 and 1 share the centroid (1, 0)
    assert abs(cluster.davies_bouldin_score(x, lab) - ref.davies_bouldin(x.numpy(), lab.numpy())) < 1e-14
    assert abs(cluster.davies_bouldin_score(x, lab) - 2 / 9) < 1e-14                  # (1 + 1) / 9 for every cluster
    pts = torch.tensor([[0.0, 0], [0, 0], [3, 4], [3, 4], [3, 4]])
    two = torch.tensor([5, 5, 8, 8, 8])
    assert cluster.davies_bouldin_score(pts, two) == 0.0 and cluster.calinski_harabasz_score(pts, two) == 1.0


# ------------------------------------------------------------------------------------------------ argument errors, no device
def test_score_argument_errors():
    from clip_dplm_amd import cluster, ops
    x = torch.zeros(20, 8)
    lab = torch.arange(20) % 3
    for f in (cluster.silhouette_samples, cluster.silhouette_score, cluster.silhouette_by_label, cluster.label_separation):
        with pytest.raises(TypeError):
            f(x.double(), lab)                                      # wrong dtype
        with pytest.raises(TypeError):
            f(x.numpy(), lab)
        with pytest.raises(ValueError):
            f(torch.zeros(20, 6), lab)                              # P % 4
        with pytest.raises(ValueError):
            f(torch.zeros(20, 516), lab)                            # P > 512
        with pytest.raises(ValueError, match="distinct labels"):
            f(x, torch.zeros(20, dtype=torch.int64))                # G < 2
        with pytest.raises(ValueError, match="distinct labels"):
            f(x, torch.arange(20))                                  # G > N - 1
        with pytest.raises(ValueError):
            f(x, lab[:19])                                          # labels of the wrong length
        with pytest.raises(TypeError):
            f(x, lab.float())                                       # ... or dtype
        with pytest.raises(TypeError):
            f(x, lab.tolist())
        with pytest.raises(ValueError, match="metric"):
            f(x, lab, metric="manhattan")
        with pytest.raises(ValueError, match="device"):
            f(x, lab)                                               # host tensors: no CPU fallback
    with pytest.raises(ValueError):
        cluster.silhouette_samples(x, lab, row_block=0)
    with pytest.raises(ValueError):
        cluster.silhouette_score(x, lab, sample_size=21)
    with pytest.raises(ValueError):
        cluster.silhouette_score(x, lab, sample_size=0)
    with pytest.raises(ValueError, match="device"):
        cluster.silhouette_score(x, lab, sample_size=10, generator=torch.Generator().manual_seed(0))
    for f in (cluster.davies_bouldin_score, cluster.calinski_harabasz_score):
        with pytest.raises(ValueError, match="distinct labels"):
            f(x, torch.zeros(20, dtype=torch.int64))
        with pytest.raises(ValueError, match="distinct labels"):
            f(x, torch.arange(20))
        with pytest.raises(ValueError):
            f(x, lab[:19])
        with pytest.raises(TypeError):
            f(x, lab.float())
        with pytest.raises(TypeError):
            f(lab, lab)                                             # an integer cloud
    with pytest.raises(ValueError, match="criterion"):
        cluster.choose_n_clusters(x, criterion="gap")
    with pytest.raises(ValueError):
        cluster.choose_n_clusters(x, candidates=[1, 2])
    with pytest.raises(ValueError, match="device"):
        cluster.choose_n_clusters(x, candidates=[2, 3])
    with pytest.raises(ValueError, match="device"):
        cluster.cluster_agreement(x, x, 3, silhouette=True)
    assert (ops.LABEL_DIST_MAX_P, ops.LABEL_DIST_MAX_G) == (512, 512)


def test_label_dist_sums_wrapper_argument_errors():
    from clip_dplm_amd import ops
    x, y = torch.zeros(20, 8), torch.zeros(30, 8)
    lab = torch.zeros(30, dtype=torch.int32)
    f = ops.label_dist_sums
    with pytest.raises(TypeError):
        f(x.double(), y, lab, 4)
    with pytest.raises(TypeError):
        f(x, y.bfloat16(), lab, 4)
    with pytest.raises(ValueError):
        f(x, torch.zeros(30, 12), lab, 4)
    with pytest.raises(ValueError):
        f(torch.zeros(20, 6), torch.zeros(30, 6), lab, 4)           # P % 4
    with pytest.raises(ValueError, match="512"):
        f(torch.zeros(20, 516), torch.zeros(30, 516), lab, 4)       # P > 512
    with pytest.raises(TypeError):
        f(x, y, lab.long(), 4)
    with pytest.raises(TypeError):
        f(x, y, [0] * 30, 4)
    with pytest.raises(ValueError):
        f(x, y, lab[:20], 4)                                        # one label per KEY
    with pytest.raises(ValueError, match="65536"):
        f(x, y, lab, 0)
    with pytest.raises(ValueError, match="65536"):
        f(x, y, lab, 65537)
    with pytest.raises(TypeError):
        f(x, y, lab, 4.0)
    with pytest.raises(ValueError, match="metric"):
        f(x, y, lab, 4, metric="l1")
    with pytest.raises(ValueError):
        f(x, y, lab, 4, nx=torch.zeros(30))
    with pytest.raises(TypeError):
        f(x, y, lab, 4, ny=torch.zeros(30, dtype=torch.float64))
    with pytest.raises(ValueError):
        f(x, y, lab, 4, diag_offset=-2)
    with pytest.raises(ValueError, match="device"):
        f(x, y, lab, 4)                                             # host tensors
    with pytest.raises(ValueError, match="device"):
        f(x, y, lab, 600, metric="cosine")


def test_package_exports():
    import clip_dplm_amd as K
    from clip_dplm_amd import cluster
    for name in ("silhouette_samples", "silhouette_score", "silhouette_by_label", "davies_bouldin_score",
                 "calinski_harabasz_score", "label_separation", "choose_n_clusters"):
        assert getattr(K, name) is getattr(cluster, name) and name in K.__all__ and name in cluster.__all__


def test_cluster_agreement_default_is_unchanged(monkeypatch):
    """Without silhouette= the dict has today's keys (k-means replaced by a stand-in: no device here)."""
    from clip_dplm_amd import cluster
    x = torch.zeros(12, 8)
    fake = lambda t, k, **kw: cluster.KMeansResult(None, torch.arange(12) % k, None, 0, True, None, None)  # noqa: E731
    monkeypatch.setattr(cluster, "kmeans", fake)
    assert set(cluster.cluster_agreement(x, x, 3)) == {"ari", "nmi"}
    assert set(cluster.cluster_agreement(x, x, 3, silhouette=False, labels=torch.arange(12) % 2)) == {
        "ari", "nmi", "ari_a_vs_labels", "nmi_a_vs_labels", "ari_b_vs_labels", "nmi_b_vs_labels"}
    with pytest.raises(ValueError, match="device"):
        cluster.cluster_agreement(x, x, 3, silhouette=True)


# ------------------------------------------------------------------------------------------------ C ABI without a device
def _call(lib, Mx, Ny, P, G, mode=0, diag=-1, labels=None):
    return lib.clipk_label_dist_sums(None, Mx, None, Ny, P, labels, G, mode, None, None, diag, None, None, 0, None)


@pytest.mark.parametrize("Mx,Ny,P,G", [(0, 8, 8, 2), (8, 0, 8, 2), (8, 8, 0, 2), (8, 8, 8, 0), (-1, 8, 8, 2), (8, 8, 6, 2),
                                       (8, 8, 516, 2), (8, 8, 8, 513)])
def test_entry_point_refuses(Mx, Ny, P, G):
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    want = -2 if Mx > 0 and Ny > 0 and P > 0 and G > 0 else -1
    assert _call(lib, Mx, Ny, P, G) == want
    assert lib.clipk_label_dist_sums_workspace(Mx, Ny, P, G) == 0


def test_entry_point_limits_and_null_pointers():
    from clip_dplm_amd import _ffi, ops
    lib = _ffi.load()
    assert lib.clipk_version() == _ffi.ABI_VERSION == 7              # entry points were added, no signature changed
    for n in ("clipk_label_dist_sums", "clipk_label_dist_sums_workspace"):
        assert n in _ffi.SIGNATURES and hasattr(lib, n)
    assert len(_ffi.SIGNATURES["clipk_label_dist_sums"][1]) == 15
    assert len(_ffi.SIGNATURES["clipk_label_dist_sums_workspace"][1]) == 4
    # a supported shape with null pointers, a mode or an offset outside the range: a bad argument, not a launch
    assert _call(lib, 100, 100, 64, 10) == -1
    assert _call(lib, 100, 100, 64, 10, mode=3) == -1 and _call(lib, 100, 100, 64, 10, mode=-1) == -1
    assert _call(lib, 100, 100, 64, 10, diag=-2) == -1
    # the slabs of the split plan: ksplit * Mx * (G rounded up to 4) floats; 4097 keys split the range
    nqb, ks = ops.label_dist_sums_plan(4097, 4097)
    assert (nqb, ks) == ops.sim_lse_bias_plan(4097, 4097) and nqb == 65 and ks > 1
    assert lib.clipk_label_dist_sums_workspace(4097, 4097, 128, 10) == ks * 4097 * 12 * 4
    assert lib.clipk_label_dist_sums_workspace(4097, 4097, 512, 512) == ks * 4097 * 512 * 4
    assert lib.clipk_label_dist_sums_workspace(1, 1, 4, 1) == 16
