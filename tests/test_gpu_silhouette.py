"""GPU: the per-label distance sums (include/clipk.h: clipk_label_dist_sums; ops.label_dist_sums) and the labeling scores
of clip_dplm_amd.cluster on top of them against the restatement of tests/silhouette_ref.py.

Real-valued outputs follow `_close`, the rule of tests/test_gpu_kmeans.py: at most 8 x the deviation of the f32
restatement from the f64 one, with a floor of 64 * 2^-24 x the quantity's magnitude.  The measured deviation and its
ratio to the bound are printed before each assertion.

Clouds: kmeans_ref.blobs(N, P, min(G, 10), 0.5, 1000 N + P).  The sums use random labels (every label present where
G <= N); the silhouettes use the blob's own labels or k-means labels.  Every Euclidean / squared-Euclidean case asserts on
the f64 side that no two distinct rows are closer than 10 sqrt(e2), e2 = 4 (P + 2) 2^-24 * 2 max|x|^2: below that the
square root amplifies the product's rounding and the generic rule does not apply (the duplicate-row test covers that
ground with its own bound).  The cosine distance has no square root and needs no such guard."""
import functools

import numpy as np
import pytest
import torch

from clip_dplm_amd import cluster, ops

import kmeans_ref
import silhouette_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SEP = 0.5


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


def _e2(P, n2):
    """The rounding of one f32 d2 = nx + ny - 2 <x, y> whose norms sum to n2: a P-term product, the norms, one fma."""
    return 4 * (P + 2) * U * n2


@functools.lru_cache(maxsize=None)
def _cloud(N, P, G, metric):
    """x f32 [N, P] (cosine: unit rows) with its blob labels, and the separation guard."""
    x, truth, _ = kmeans_ref.blobs(N, P, min(G, 10), SEP, 1000 * N + P)
    if metric == "cosine":
        x = ref.normalize(x.astype(np.float64)).astype(np.float32)
    else:
        x64 = x.astype(np.float64)
        need = 10 * np.sqrt(_e2(P, 2 * float((x64 * x64).sum(1).max())))
        sep = ref.min_separation(x)
        print(f"separation guard {N} x {P}: closest pair {sep:.3e}, needed {need:.3e} ({sep / need * 10:.0f} x sqrt(e2))")
        assert sep >= need
    return x, truth


def _random_labels(N, G, seed):
    rng = np.random.default_rng(seed)
    if G > N:
        return rng.choice(G, N, replace=False).astype(np.int32)
    lab = np.concatenate([np.arange(G), rng.integers(0, G, N - G)])
    return rng.permutation(lab).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _sums_case(N, P, G, metric):
    x, _ = _cloud(N, P, G, metric)
    lab = _random_labels(N, G, N + P + G)
    r64 = ref.label_dist_sums(x.astype(np.float64), x.astype(np.float64), lab, G, metric, 0)
    r32 = ref.label_dist_sums(x, x, lab, G, metric, 0)
    return x, lab, r64, r32


def _dev(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


# ------------------------------------------------------------------------------------------------ 1: the sums
# every N, P and G of the issue, both forms of the second product on either side of G = 32, one and several label tiles
# per wave; not the full product
SUM_SHAPES = [(2, 4, 1), (65, 4, 2), (63, 60, 2), (65, 60, 10), (193, 4, 32), (193, 60, 33), (193, 60, 64), (193, 512, 65),
              (63, 512, 512), (4097, 60, 10), (4097, 512, 512)]


@pytest.mark.parametrize("metric", ref.METRICS)
@pytest.mark.parametrize("N,P,G", SUM_SHAPES)
def test_label_dist_sums(dev, N, P, G, metric):
    x, lab, r64, r32 = _sums_case(N, P, G, metric)
    xd, ld = _dev(dev, x, lab)
    out = ops.label_dist_sums(xd, xd, ld, G, metric, diag_offset=0)
    assert out.dtype == torch.float32 and out.shape == (N, G)
    if N == 4097:
        assert ops.label_dist_sums_plan(N, N)[1] > 1                # the key range is split
    _close(f"sums {N} x {P} x {G} {metric}", out, r64, r32)
    assert torch.equal(out, ops.label_dist_sums(xd, xd, ld, G, metric, diag_offset=0))     # two runs: the same bits
    # the norms given equal the norms computed here
    n = (xd * xd).sum(1)
    assert torch.equal(out, ops.label_dist_sums(xd, xd, ld, G, metric, nx=n, ny=n, diag_offset=0))


@pytest.mark.parametrize("metric", ref.METRICS)
def test_rectangular_call_equals_the_square_calls_rows(dev, metric):
    x, lab, r64, r32 = _sums_case(193, 60, 10, metric)
    xd, ld = _dev(dev, x, lab)
    out = ops.label_dist_sums(xd[64:130], xd, ld, 10, metric, diag_offset=64)
    assert out.shape == (66, 10)
    _close(f"rows 64..130 {metric}", out, r64[64:130], r32[64:130])
    # two clouds, nothing skipped
    y = _cloud(65, 60, 10, metric)[0]
    yd, = _dev(dev, y)
    out = ops.label_dist_sums(yd, xd, ld, 10, metric)
    _close(f"two clouds {metric}", out, ref.label_dist_sums(y.astype(np.float64), x.astype(np.float64), lab, 10, metric),
           ref.label_dist_sums(y, x, lab, 10, metric))


@pytest.mark.parametrize("metric", ref.METRICS)
def test_kept_diagonal_adds_the_diagonal_term(dev, metric):
    """diag_offset = -1: the own column gains the formula's value at j == i - 0 up to the product's rounding against the
    norms, e2_ii (cosine: the rounding of <x, x> against 1), or its square root; every other entry keeps its bits."""
    N, P, G = 193, 60, 10
    x, lab, r64, r32 = _sums_case(N, P, G, metric)
    xd, ld = _dev(dev, x, lab)
    dropped = ops.label_dist_sums(xd, xd, ld, G, metric, diag_offset=0)
    kept = ops.label_dist_sums(xd, xd, ld, G, metric, diag_offset=-1)
    own = torch.zeros(N, G, dtype=torch.bool, device=dev)
    own[torch.arange(N, device=dev), ld.long()] = True
    assert torch.equal(kept[~own], dropped[~own])
    n2 = 2 * (x.astype(np.float64) ** 2).sum(1)
    term = _e2(P, n2)
    if metric == "euclidean":
        term = np.sqrt(term)
    diff = (kept[own].double() - dropped[own].double()).cpu().numpy()     # (row-major: one own entry per row, in row order)
    slack = 64 * U * r64[np.arange(N), lab]         # one more term early in an f32 sum moves every later rounding: the floor
    print(f"diagonal term {metric}: largest {diff.max():.3e}, allowed {(term + slack).max():.3e}; restatement's own "
          f"{ref.diagonal_terms(x, metric).max():.3e}")
    assert (diff >= -slack).all() and (diff <= term + slack).all()
    assert (ref.diagonal_terms(x, metric) <= term).all()                  # the restatement's diagonal obeys the same bound


def test_labels_outside_the_range_join_no_column(dev):
    x, _ = _cloud(193, 60, 10, "euclidean")
    lab = (np.arange(193) % 12 - 1).astype(np.int32)                      # -1 and 10 among them
    xd, ld = _dev(dev, x, lab)
    out = ops.label_dist_sums(xd, xd, ld, 10, diag_offset=0)
    assert out.shape == (193, 10)                                         # the two padding columns sliced off
    x64 = x.astype(np.float64)
    _close("labels outside the range dropped", out, ref.label_dist_sums(x64, x64, lab, 10, "euclidean", 0),
           ref.label_dist_sums(x, x, lab, 10, "euclidean", 0))


def test_more_labels_than_one_launch(dev):
    """n_labels = 513: two walks, the second with one column."""
    x, _ = _cloud(193, 60, 10, "euclidean")
    lab = _random_labels(193, 513, 9)
    lab[:3] = (511, 512, 0)
    xd, ld = _dev(dev, x, lab)
    out = ops.label_dist_sums(xd, xd, ld, 513, diag_offset=0)
    assert out.shape == (193, 513)
    x64 = x.astype(np.float64)
    _close("513 labels", out, ref.label_dist_sums(x64, x64, lab, 513, "euclidean", 0),
           ref.label_dist_sums(x, x, lab, 513, "euclidean", 0))


def test_duplicate_rows(dev):
    """Three copies of one row over two labels.  The f64 distance of a coincident pair is 0; the kernel's is the square
    root of its d2's rounding, at most sqrt(e2_ij), e2_ij = 4 (P + 2) 2^-24 (nx_i + ny_j).  With those pairs taken out of
    the restatement the rest of every sum follows the rule."""
    N, P, G = 193, 60, 4
    x = _cloud(N, P, 10, "euclidean")[0].copy()
    dup = [5, 70, 150]
    x[70] = x[150] = x[5]
    lab = _random_labels(N, G, 3)
    lab[5], lab[70], lab[150] = 0, 0, 1
    x64 = x.astype(np.float64)
    d64, d32 = ref.distances_direct(x, x, "euclidean"), ref.distances(x, x, "euclidean")
    extra = np.zeros((N, G))
    for i in dup:
        for j in dup:
            if i != j:
                assert d64[i, j] == 0
                d32[i, j] = 0
                extra[i, lab[j]] += np.sqrt(_e2(P, 2 * float((x64[i] ** 2).sum())))
    r64, r32 = ref.sums_of(d64, lab, G, 0), ref.sums_of(d32, lab, G, 0)
    xd, ld = _dev(dev, x, lab)
    out = ops.label_dist_sums(xd, xd, ld, G, diag_offset=0).double().cpu().numpy()
    rest = np.ones((N, G), dtype=bool)
    rest[dup] = False
    _close("rows without a twin", out[rest], r64[rest], r32[rest])
    bound = max(8 * np.abs(r32 - r64).max(), 64 * U * r64.max())
    over = out[dup] - r64[dup]
    print(f"coincident pairs: kernel adds at most {over.max():.3e}, allowed {extra[dup].max():.3e} + {bound:.3e}")
    assert (over >= -bound).all() and (over <= extra[dup] + bound).all()


# ------------------------------------------------------------------------------------------------ 2: the Python layer
@functools.lru_cache(maxsize=None)
def _sil_ref(N, P, G, metric, singleton=False):
    x, truth = _cloud(N, P, G, "euclidean")         # (cosine: silhouette_samples normalises, as the restatement does)
    lab = truth.copy()
    if singleton:
        lab[N // 2] = 77                            # a cluster of one point, a label value out of sequence
    return x, lab, ref.silhouette_samples(x.astype(np.float64), lab, metric), ref.silhouette_samples(x, lab, metric)


@pytest.mark.parametrize("N,P,metric,singleton", [(193, 60, "euclidean", False), (1030, 128, "euclidean", True),
                                                  (193, 60, "cosine", False), (193, 60, "sqeuclidean", False)])
def test_silhouette_samples(dev, N, P, metric, singleton):
    x, lab, s64, s32 = _sil_ref(N, P, 10, metric, singleton)
    assert s64.min() < -0.01 and s64.max() > 0.05                         # values of both signs, away from 0
    xd, ld = _dev(dev, x, lab)
    s = cluster.silhouette_samples(xd, ld, metric=metric)
    assert s.dtype == torch.float32 and s.shape == (N,) and s.device == xd.device
    _close(f"silhouette {N} x {P} {metric}", s, s64, s32)
    if singleton:
        assert float(s[N // 2]) == 0.0
    _close("row_block=100", cluster.silhouette_samples(xd, ld, metric=metric, row_block=100), s64, s32)
    assert torch.equal(s, cluster.silhouette_samples(xd, ld.cpu().int(), metric=metric))   # host labels, any integer dtype


def test_silhouette_samples_under_kmeans_labels(dev):
    """4097 x 512 with 64 k-means clusters: the key range is split, two label rows per wave."""
    N, P, K = 4097, 512, 64
    x, _ = _cloud(N, P, K, "euclidean")
    xd, = _dev(dev, x)
    labels = cluster.kmeans(xd, K, init="random", max_iter=5, tol=None, generator=torch.Generator().manual_seed(1)).labels
    lab = labels.cpu().numpy()
    assert len(np.unique(lab)) > 32
    s64, s32 = ref.silhouette_samples(x.astype(np.float64), lab), ref.silhouette_samples(x, lab)
    _close("silhouette under k-means labels", cluster.silhouette_samples(xd, labels), s64, s32)


def test_silhouette_score_and_by_label(dev):
    N = 1030
    x, lab, s64, s32 = _sil_ref(N, 128, 10, "euclidean", True)
    xd, ld = _dev(dev, x, lab)
    _close("score", cluster.silhouette_score(xd, ld), s64.mean(), s32.astype(np.float64).mean())
    values, means, counts = cluster.silhouette_by_label(xd, ld)
    v64, m64, c64 = ref.silhouette_by_label(x.astype(np.float64), lab)
    _, m32, _ = ref.silhouette_by_label(x, lab)
    assert np.array_equal(values.cpu().numpy(), v64) and np.array_equal(counts.cpu().numpy(), c64) and 77 in v64
    _close("silhouette by label", means, m64, m32)
    # sample_size: the score of that subset, queries and keys alike
    got = cluster.silhouette_score(xd, ld, sample_size=400, generator=torch.Generator().manual_seed(5))
    idx = torch.randperm(N, generator=torch.Generator().manual_seed(5))[:400]
    assert got == cluster.silhouette_score(xd[idx.to(dev)], ld[idx.to(dev)])
    sub = idx.numpy()
    _close("score of a sample", got, ref.silhouette_samples(x[sub].astype(np.float64), lab[sub]).mean(),
           ref.silhouette_samples(x[sub], lab[sub]).astype(np.float64).mean())
    assert got != cluster.silhouette_score(xd, ld)


def test_label_separation(dev):
    N = 1030
    x, lab, s64, s32 = _sil_ref(N, 128, 10, "euclidean", True)
    xd, ld = _dev(dev, x, lab)
    out = cluster.label_separation(xd, ld)
    assert set(out) == {"silhouette", "davies_bouldin", "calinski_harabasz", "silhouette_by_label"}
    assert all(isinstance(out[k], float) for k in ("silhouette", "davies_bouldin", "calinski_harabasz"))
    x64 = x.astype(np.float64)
    _close("silhouette", out["silhouette"], s64.mean(), s32.astype(np.float64).mean())
    _close("davies_bouldin", out["davies_bouldin"], ref.davies_bouldin(x64, lab), ref.davies_bouldin(x, lab))
    _close("calinski_harabasz", out["calinski_harabasz"], ref.calinski_harabasz(x64, lab), ref.calinski_harabasz(x, lab))
    values, means, counts = out["silhouette_by_label"]
    _close("silhouette_by_label", means, ref.silhouette_by_label(x64, lab)[1], ref.silhouette_by_label(x, lab)[1])
    # the centroid-based scores on the device equal the host glue on the same data
    assert abs(out["davies_bouldin"] - cluster.davies_bouldin_score(xd.cpu(), ld.cpu())) <= 64 * U * out["davies_bouldin"]
    # (f64 index_add_ on the device adds in an order of its own: equal to rounding, not to the bit)
    assert abs(out["davies_bouldin"] - cluster.davies_bouldin_score(xd, ld)) <= 1e-12 * out["davies_bouldin"]


def test_choose_n_clusters_finds_four_blobs(dev):
    x, truth, _ = kmeans_ref.blobs(2000, 32, 4, 4.0, 11)
    xd, = _dev(dev, x)
    for criterion in ("silhouette", "calinski_harabasz", "davies_bouldin"):
        k, scores, res = cluster.choose_n_clusters(xd, range(2, 8), criterion=criterion, n_init=3,
                                                   generator=torch.Generator().manual_seed(0))
        print(criterion, scores)
        assert k == 4 and sorted(scores) == list(range(2, 8)) and res.centroids.shape == (4, 32)
        assert cluster.adjusted_rand_index(res.labels.cpu(), torch.from_numpy(truth)) == 1.0


def test_cluster_agreement_with_silhouettes(dev):
    x, truth, _ = kmeans_ref.blobs(1200, 32, 6, 4.0, 23)
    rng = np.random.default_rng(24)
    q, _ = np.linalg.qr(rng.standard_normal((32, 32)))
    y = (x.astype(np.float64) @ q + 0.05 * rng.standard_normal(x.shape)).astype(np.float32)
    a, b = _dev(dev, x, y)
    kw = dict(n_init=5, generator=torch.Generator().manual_seed(0))
    out = cluster.cluster_agreement(a, b, n_clusters=6, silhouette=True, **kw)
    assert set(out) == {"ari", "nmi", "silhouette_a", "silhouette_b"} and all(isinstance(v, float) for v in out.values())
    assert out["ari"] > 0.99 and out["silhouette_a"] > 0.3 and abs(out["silhouette_a"] - out["silhouette_b"]) < 0.01
    full = cluster.cluster_agreement(a, b, n_clusters=6, labels=torch.from_numpy(truth), silhouette=True, **kw)
    assert set(full) == {"ari", "nmi", "silhouette_a", "silhouette_b", "ari_a_vs_labels", "nmi_a_vs_labels",
                         "ari_b_vs_labels", "nmi_b_vs_labels", "silhouette_a_vs_labels", "silhouette_b_vs_labels"}
    s64 = ref.silhouette_samples(x.astype(np.float64), truth).mean()
    _close("silhouette_a_vs_labels", full["silhouette_a_vs_labels"], s64, ref.silhouette_samples(x, truth).astype(np.float64).mean())
    assert set(cluster.cluster_agreement(a, b, n_clusters=6, **kw)) == {"ari", "nmi"}
