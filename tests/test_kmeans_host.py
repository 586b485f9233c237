"""CPU: the host side of clip_dplm_amd.cluster (contingency table, adjusted Rand index, normalised mutual information,
seeding, argument checks), the C ABI of clipk_kmeans_step as far as it goes without a device, and the restatement of
tests/kmeans_ref.py against literal loops and hand-derived tables."""
import math

import numpy as np
import pytest
import torch

import kmeans_ref as ref


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_restated_step_against_double_loop():
    x, _, _ = ref.blobs(23, 4, 3, 2.0, 5)
    x = x.astype(np.float64)
    c = x[[2, 7, 11, 11]].copy()                    # the last two are equal: the higher index stays empty
    labels, best, margin = ref.assign(x, c)
    for i in range(23):
        d2 = [sum((x[i, p] - c[k, p]) ** 2 for p in range(4)) for k in range(4)]
        k = min(range(4), key=lambda k: (d2[k], k))
        assert labels[i] == k and k != 3
        assert abs((x[i] @ x[i] - best[i]) - d2[k]) < 1e-12
        assert abs(margin[i] - (sorted(d2)[1] - d2[k])) < 1e-12
    new, counts = ref.update(x, c, labels)
    assert counts[3] == 0 and np.array_equal(new[3], c[3]) and counts.sum() == 23
    for k in range(3):
        assert np.allclose(new[k], x[labels == k].mean(0), rtol=0, atol=1e-13)
    # the f32 form gives the same labels on these separated points
    assert np.array_equal(ref.assign(x.astype(np.float32), c.astype(np.float32))[0], labels)


def test_restated_fit_reaches_a_fixed_point():
    x, truth, centres = ref.blobs(300, 8, 4, 4.0, 3)
    r = ref.fit(x.astype(np.float64), centres.astype(np.float64))
    assert r.converged and r.n_empty == 0
    labels, _, _ = ref.assign(x.astype(np.float64), r.centroids)
    assert np.array_equal(labels, r.labels) and np.array_equal(ref.update(x.astype(np.float64), r.centroids, labels)[0], r.centroids)
    assert ref.ari_pairs(r.labels[:80], truth[:80]) == 1.0
    assert abs(r.inertia - r.d2.sum()) == 0 and np.array_equal(ref.fit(x, centres).labels, r.labels)


# ------------------------------------------------------------------------------------------------ ARI / NMI
def _t(v):
    return torch.tensor(v, dtype=torch.int64)


def test_contingency_table():
    from clip_dplm_amd import cluster
    a, b = _t([0, 0, 1, 1, 2, 2, 2]), _t([1, 1, 0, 3, 3, 3, 0])
    t = cluster.contingency(a, b)
    assert t.dtype == torch.int64 and t.tolist() == [[0, 2, 0, 0], [1, 0, 0, 1], [1, 0, 0, 2]]
    assert cluster.contingency(a.int(), b.int()).equal(t)
    assert cluster.contingency(_t([]), _t([])).shape == (0, 0)
    with pytest.raises(TypeError):
        cluster.contingency(a.float(), b)
    with pytest.raises(TypeError):
        cluster.contingency(a.tolist(), b)
    with pytest.raises(ValueError):
        cluster.contingency(a, b[:-1])
    with pytest.raises(ValueError):
        cluster.contingency(a[None], b[None])
    with pytest.raises(ValueError):
        cluster.contingency(a - 1, b)


def test_ari_nmi_hand_derived():
    """a = 001122, b = 001112: the table is [[2, 0, 0], [0, 2, 0], [0, 1, 1]]; both scores worked by hand below."""
    from clip_dplm_amd import cluster
    a, b = _t([0, 0, 1, 1, 2, 2]), _t([0, 0, 1, 1, 1, 2])
    # pairs together in a: 3; in b: 1 + 3 = 4; in both: (0,1), (2,3) = 2; all pairs: 15
    # ARI = (2 - 3 * 4 / 15) / ((3 + 4) / 2 - 3 * 4 / 15) = 1.2 / 2.7 = 4 / 9
    assert abs(cluster.adjusted_rand_index(a, b) - 4.0 / 9.0) < 1e-15
    assert abs(ref.ari_pairs(a.numpy(), b.numpy()) - 4.0 / 9.0) < 1e-15
    # H(a) = ln 3;  H(b) = -(1/3 ln 1/3 + 1/2 ln 1/2 + 1/6 ln 1/6);  the joint has cells 1/3, 1/3, 1/6, 1/6
    ha = math.log(3)
    hb = -(math.log(1 / 3) / 3 + math.log(1 / 2) / 2 + math.log(1 / 6) / 6)
    hab = -(2 * math.log(1 / 3) / 3 + 2 * math.log(1 / 6) / 6)
    want = (ha + hb - hab) / (0.5 * (ha + hb))
    assert abs(cluster.normalized_mutual_info(a, b) - want) < 1e-14
    assert abs(ref.nmi_direct(a.numpy(), b.numpy()) - want) < 1e-14


def test_ari_nmi_identical_permuted_independent():
    from clip_dplm_amd import cluster
    rng = np.random.default_rng(7)
    a = rng.integers(0, 5, 200)
    perm = np.array([3, 0, 4, 1, 2])
    for b in (a, perm[a], perm[a] + 7):             # the same partition under other names (and with unused names)
        assert cluster.adjusted_rand_index(_t(a), _t(b)) == 1.0
        assert abs(cluster.normalized_mutual_info(_t(a), _t(b)) - 1.0) < 1e-14
    b = rng.integers(0, 4, 200)                     # independent of a
    ari, want = cluster.adjusted_rand_index(_t(a), _t(b)), ref.ari_pairs(a, b)
    assert abs(ari - want) < 1e-13 and abs(ari) < 0.05
    nmi = cluster.normalized_mutual_info(_t(a), _t(b))
    assert abs(nmi - ref.nmi_direct(a, b)) < 1e-13 and 0 <= nmi < 0.1
    # symmetric in its arguments
    assert abs(cluster.adjusted_rand_index(_t(b), _t(a)) - ari) < 1e-15
    # partial agreement against pair counting, several sizes
    for n, ka, kb in ((2, 2, 2), (3, 2, 3), (17, 3, 2), (60, 4, 6)):
        a, b = rng.integers(0, ka, n), rng.integers(0, kb, n)
        assert abs(cluster.adjusted_rand_index(_t(a), _t(b)) - ref.ari_pairs(a, b)) < 1e-13
        assert abs(cluster.normalized_mutual_info(_t(a), _t(b)) - ref.nmi_direct(a, b)) < 1e-13


def test_ari_nmi_degenerate():
    from clip_dplm_amd import cluster
    ari, nmi = cluster.adjusted_rand_index, cluster.normalized_mutual_info
    one, other = _t([0, 0, 0, 0]), _t([3, 3, 3, 3])
    assert ari(one, other) == 1.0 and nmi(one, other) == 1.0       # one cluster on both sides
    assert ari(_t([0]), _t([5])) == 1.0 and nmi(_t([0]), _t([5])) == 1.0          # n < 2
    assert ari(_t([]), _t([])) == 1.0 and nmi(_t([]), _t([])) == 1.0
    singles = _t([0, 1, 2, 3])
    assert ari(singles, _t([3, 2, 1, 0])) == 1.0                    # every point alone on both sides
    assert ari(one, _t([0, 0, 1, 1])) == 0.0 and nmi(one, _t([0, 0, 1, 1])) == 0.0   # one cluster on one side only
    assert ari(one, singles) == 0.0
    assert ari(_t([0, 0, 1, 1]), _t([0, 1, 0, 1])) < 0               # below chance


# ------------------------------------------------------------------------------------------------ seeding
@pytest.mark.parametrize("init", ["k-means++", "random"])
def test_init_rows_distinct_and_reproducible(init):
    from clip_dplm_amd import cluster
    x = torch.from_numpy(ref.blobs(500, 8, 6, 3.0, 1)[0])
    c = cluster.init_centroids(x, 12, init, generator=torch.Generator().manual_seed(3))
    assert c.shape == (12, 8) and c.dtype == torch.float32
    rows = [int((x == ci).all(1).nonzero()[0, 0]) for ci in c]      # every centroid is a row of x ...
    assert len(set(rows)) == 12                                     # ... and no row twice
    again = cluster.init_centroids(x, 12, init, generator=torch.Generator().manual_seed(3))
    assert torch.equal(c, again)
    other = cluster.init_centroids(x, 12, init, generator=torch.Generator().manual_seed(4))
    assert not torch.equal(c, other)
    c[0] = 0
    assert not (x == 0).all(1).any()                                # a copy, not a view of x
    with pytest.raises(ValueError):
        cluster.init_centroids(x, 3, "farthest")


def test_kmeanspp_spreads_over_separated_blobs():
    """With blobs 40 noise widths apart the D^2 draw takes one point of every blob before it takes a second of any."""
    from clip_dplm_amd import cluster
    xs, truth, _ = ref.blobs(400, 8, 5, 40.0, 2)
    c = cluster.init_centroids(torch.from_numpy(xs), 5, "k-means++", generator=torch.Generator().manual_seed(0))
    rows = [int((torch.from_numpy(xs) == ci).all(1).nonzero()[0, 0]) for ci in c]
    assert sorted(truth[rows]) == [0, 1, 2, 3, 4]
    # fewer distinct rows than centres: still K rows, no failing draw
    same = torch.ones(6, 4)
    assert cluster.init_centroids(same, 3, "k-means++", generator=torch.Generator().manual_seed(0)).equal(same[:3])


# ------------------------------------------------------------------------------------------------ arguments
def test_kmeans_argument_errors():
    from clip_dplm_amd import cluster, ops
    km = cluster.kmeans
    x = torch.zeros(20, 8)
    with pytest.raises(TypeError):
        km(x.numpy(), 3)
    with pytest.raises(TypeError):
        km(x.double(), 3)
    with pytest.raises(TypeError):
        km(x.bfloat16(), 3)
    with pytest.raises(ValueError):
        km(x[0], 3)                                                 # not 2-D
    with pytest.raises(ValueError):
        km(x[:0], 3)                                                # empty
    with pytest.raises(ValueError):
        km(torch.zeros(20, 6), 3)                                   # not a multiple of 4
    with pytest.raises(ValueError):
        km(torch.zeros(20, 516), 3)                                 # above 512
    with pytest.raises(TypeError):
        km(x, 3.0)
    with pytest.raises(TypeError):
        km(x, True)
    with pytest.raises(ValueError):
        km(x, 0)
    with pytest.raises(ValueError):
        km(x, 21)                                                   # more clusters than points
    with pytest.raises(ValueError):
        km(x, 3, metric="manhattan")
    with pytest.raises(ValueError):
        km(x, 3, init="farthest")
    with pytest.raises(ValueError):
        km(x, 3, init=torch.zeros(4, 8))                            # K rows
    with pytest.raises(ValueError):
        km(x, 3, init=torch.zeros(3, 12))
    with pytest.raises(TypeError):
        km(x, 3, init=torch.zeros(3, 8, dtype=torch.float64))
    with pytest.raises(ValueError):
        km(x, 3, n_init=0)
    with pytest.raises(TypeError):
        km(x, 3, n_init=1.5)
    with pytest.raises(ValueError):
        km(x, 3, max_iter=-1)
    with pytest.raises(ValueError):
        km(x, 3, check_every=0)
    with pytest.raises(ValueError):
        km(x, 3, tol=-1e-4)
    with pytest.raises(ValueError):
        km(x, 3, tol=float("nan"))
    with pytest.raises(ValueError, match="device"):
        km(x, 3)                                                    # host tensors: no CPU fallback
    with pytest.raises(ValueError, match="device"):
        km(x, 3, init=torch.zeros(3, 8), tol=None, metric="cosine")
    with pytest.raises(ValueError, match="device"):
        cluster.cluster_agreement(x, x, 3)
    with pytest.raises(ValueError):
        cluster.cluster_agreement(x, x[:10], 3)
    with pytest.raises(ValueError):
        cluster.cluster_agreement(x, x, 3, labels=torch.zeros(19, dtype=torch.int64))
    with pytest.raises(TypeError):
        cluster.cluster_agreement(x, x, 3, labels=torch.zeros(20))
    assert (ops.KMEANS_MAX_P, ops.KMEANS_MAX_K_FUSED, ops.KMEANS_MAX_K, ops.KMEANS_MAX_N) == (512, 64, 65536, 1 << 24)


def test_kmeans_step_wrapper_argument_errors():
    from clip_dplm_amd import ops
    x, c = torch.zeros(20, 8), torch.zeros(3, 8)
    lab = torch.zeros(20, dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.kmeans_step(x.double(), c)
    with pytest.raises(TypeError):
        ops.kmeans_step(x, c.bfloat16())
    with pytest.raises(ValueError):
        ops.kmeans_step(x, torch.zeros(3, 12))
    with pytest.raises(ValueError):
        ops.kmeans_step(torch.zeros(20, 6), torch.zeros(3, 6))
    with pytest.raises(ValueError):
        ops.kmeans_step(torch.zeros(20, 516), torch.zeros(3, 516))
    with pytest.raises(ValueError):
        ops.kmeans_step(x, torch.zeros(65, 8))                      # fused mode: K <= 64
    with pytest.raises(ValueError):
        ops.kmeans_step(x, torch.zeros(65537, 8), labels=lab)
    with pytest.raises(ValueError):
        ops.kmeans_step(x, c, nc=torch.zeros(4))
    with pytest.raises(TypeError):
        ops.kmeans_step(x, c, nc=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(TypeError):
        ops.kmeans_step(x, c, labels=lab.long())
    with pytest.raises(TypeError):
        ops.kmeans_step(x, c, labels=[0] * 20)
    with pytest.raises(ValueError):
        ops.kmeans_step(x, c, labels=lab[:19])
    with pytest.raises(ValueError, match="device"):
        ops.kmeans_step(x, c)                                       # host tensors
    with pytest.raises(ValueError, match="device"):
        ops.kmeans_step(x, torch.zeros(65, 8), labels=lab)


def test_package_exports():
    import clip_dplm_amd as K
    from clip_dplm_amd import cluster
    assert K.cluster is cluster and "cluster" in K.__all__
    for name in ("kmeans", "KMeansResult", "contingency", "adjusted_rand_index", "normalized_mutual_info", "cluster_agreement"):
        assert getattr(K, name) is getattr(cluster, name) and name in K.__all__ and name in cluster.__all__


# ------------------------------------------------------------------------------------------------ C ABI without a device
def _call(lib, N, K, P, labels_in=None):
    return lib.clipk_kmeans_step(None, N, None, K, P, None, labels_in, None, None, None, None, None, 0, None)


@pytest.mark.parametrize("N,K,P", [(0, 8, 8), (8, 0, 8), (-1, 8, 8), (8, 8, 0), (8, 8, 6), (8, 8, 516), (8, 65, 8),
                                   ((1 << 24) + 1, 8, 8)])
def test_entry_point_refuses(N, K, P):
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    want = -2 if N > 0 and K > 0 and P > 0 else -1
    assert _call(lib, N, K, P) == want
    if K != 65:                                     # 65 centroids: refused in fused mode only
        assert lib.clipk_kmeans_step_workspace(N, K, P) == 0


def test_entry_point_limits_and_null_pointers():
    import ctypes
    from clip_dplm_amd import _ffi, ops
    lib = _ffi.load()
    assert lib.clipk_version() == _ffi.ABI_VERSION == 7              # entry points were added, no signature changed
    for n in ("clipk_kmeans_step", "clipk_kmeans_step_workspace"):
        assert n in _ffi.SIGNATURES and hasattr(lib, n)
    assert len(_ffi.SIGNATURES["clipk_kmeans_step"][1]) == 14 and len(_ffi.SIGNATURES["clipk_kmeans_step_workspace"][1]) == 3
    assert lib.clipk_kmeans_step_workspace(1, 1, 4) > 0 and lib.clipk_kmeans_step_workspace(1 << 24, 65536, 512) > 0
    assert lib.clipk_kmeans_step_workspace(8, 65537, 8) == 0
    # a supported shape with null pointers is a bad argument, not a launch - in either mode
    assert _call(lib, 100, 10, 64) == -1
    some = (ctypes.c_int * 100)()
    assert _call(lib, 100, 200, 64, ctypes.cast(some, ctypes.c_void_p)) == -1
    assert _call(lib, 100, 65537, 64, ctypes.cast(some, ctypes.c_void_p)) == -2
    # the slabs and the count partials of the split plan: ksplit * K * (P + 1) floats; 4097 points split the range
    nqb, ks = ops.kmeans_step_plan(4097, 10)
    assert (nqb, ks) == ops.sim_lse_bias_plan(10, 4097) and nqb == 1 and ks > 1
    assert lib.clipk_kmeans_step_workspace(4097, 10, 128) == ks * 10 * 129 * 4
    nqb, ks = ops.kmeans_step_plan(3001, 200)
    assert nqb == 4 and lib.clipk_kmeans_step_workspace(3001, 200, 64) == ks * 200 * 65 * 4
