"""CPU: host side of the diagnostics API (clip_dplm_amd/diagnostics.py) - argument checks before any launch, the f64
reductions of SimilarityStats, confusion counting, the C entry points' refusals, the restatement's binning rule - and
no CPU fallback."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import clip_dplm_amd
from clip_dplm_amd import _ffi, diagnostics, ops

import sim_stats_ref as ref


def test_exported():
    assert clip_dplm_amd.diagnostics is diagnostics
    for name in ("similarity_stats", "SimilarityStats", "evaluate_embeddings"):
        assert getattr(clip_dplm_amd, name) is getattr(diagnostics, name)


def test_argument_errors_before_any_launch():
    x, y = torch.zeros(3, 8), torch.zeros(100, 8)
    with pytest.raises(ValueError, match="nbins"):
        ops.sim_stats(x, y, nbins=0)
    with pytest.raises(ValueError, match="nbins"):
        ops.sim_stats(x, y, nbins=257)
    with pytest.raises(ValueError, match="lo < hi"):
        ops.sim_stats(x, y, lo=1.0, hi=1.0)
    with pytest.raises(ValueError, match="lo < hi"):
        ops.sim_stats(x, y, lo=2.0, hi=-2.0)
    with pytest.raises(ValueError, match="lo < hi"):
        ops.sim_stats(x, y, scale=0.0)                          # the default range collapses
    with pytest.raises(ValueError, match="both sides"):
        ops.sim_stats(x, y, cls_x=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="both sides"):
        ops.sim_stats(x, y, cls_y=torch.zeros(100, dtype=torch.int64))
    with pytest.raises(ValueError, match="cls_y"):
        ops.sim_stats(x, y, cls_x=torch.zeros(3, dtype=torch.int64), cls_y=torch.zeros(99, dtype=torch.int64))
    with pytest.raises(ValueError, match="cls_x"):
        ops.sim_stats(x, y, cls_x=torch.zeros(3, dtype=torch.int32), cls_y=torch.zeros(100, dtype=torch.int64))
    with pytest.raises(ValueError, match="labels"):
        ops.sim_stats(x, y, labels=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="labels"):
        ops.sim_stats(x, y, labels=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="outside"):
        ops.sim_stats(torch.zeros(200, 8), y)
    with pytest.raises(TypeError):
        ops.sim_stats(x.double(), y)
    with pytest.raises(ValueError, match="columns"):
        ops.sim_stats(x, torch.zeros(100, 12))
    with pytest.raises(ValueError, match="P % 4"):
        ops.sim_stats(torch.zeros(3, 6), torch.zeros(100, 6))
    with pytest.raises(ValueError):
        ops.sim_stats(torch.zeros(3, 8, 1), y)
    with pytest.raises(ValueError, match="bins"):
        diagnostics.similarity_stats(x, y, bins=300)
    with pytest.raises(ValueError, match="range"):
        diagnostics.similarity_stats(x, y, range=(1.0, 0.0))
    with pytest.raises(ValueError, match="both sides"):
        diagnostics.similarity_stats(x, y, class_ids=(torch.zeros(3, dtype=torch.int64), None))
    with pytest.raises(ValueError, match="class_ids"):
        diagnostics.similarity_stats(x, y, class_ids=torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError, match="labels"):
        diagnostics.similarity_stats(x, y, labels=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(TypeError):
        diagnostics.similarity_stats(x.half(), y)
    with pytest.raises(ValueError, match="two rows"):
        diagnostics.uniformity(torch.zeros(1, 8))


def test_cpu_tensors_raise_without_fallback():
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(3, 8, generator=g), torch.randn(100, 8, generator=g)
    with pytest.raises(_ffi.ClipkError):
        ops.sim_stats(x, y)
    with pytest.raises(_ffi.ClipkError):
        diagnostics.similarity_stats(x, y)
    with pytest.raises(_ffi.ClipkError):
        diagnostics.uniformity(x)
    with pytest.raises(_ffi.ClipkError):
        diagnostics.alignment(x, y[:3])
    with pytest.raises(_ffi.ClipkError):
        diagnostics.group_similarity(x, torch.tensor([0, 1, 0]))


def _hand_made():
    # 4 queries, bins = 2 over [-1, 1): slots [below, [-1, 0), [0, 1), at or above]
    return diagnostics.SimilarityStats(
        labels=torch.tensor([0, 1, 2, 3]),
        pos=torch.tensor([0.5, 0.25, -0.5, 0.75]),
        best=torch.tensor([0.5, 0.5, 0.25, 0.75]),
        best_idx=torch.tensor([0, 3, 0, 3]),
        hard=torch.tensor([0.25, 0.5, 0.25, 0.75]),
        hard_idx=torch.tensor([2, 3, 0, 1]),
        lse=torch.tensor([1.5, 1.5, 1.25, 1.75]),
        neg_sum=torch.tensor([0.25, 0.5, 0.0, 1.0], dtype=torch.float64),
        neg_sumsq=torch.tensor([0.375, 0.5, 0.25, 0.75], dtype=torch.float64),
        hist_neg=torch.tensor([1, 4, 6, 1]), hist_pos=torch.tensor([0, 1, 3, 0]),
        range=(-1.0, 1.0), scale=1.0, n_keys=4)


def test_summary_hand_computed_in_f64():
    st = _hand_made()
    assert st.correct.tolist() == [True, False, False, True]
    assert torch.equal(st.margin, torch.tensor([0.25, -0.25, -0.75, 0.0]))
    assert st.bins == 2 and st.bin_edges.tolist() == [-1.0, 0.0, 1.0]
    s = st.summary()
    assert s["n"] == 4 and s["top1"] == 0.5
    assert s["pos_mean"] == 0.25
    assert s["pos_std"] == pytest.approx(math.sqrt((0.25 ** 2 + 0 + 0.75 ** 2 + 0.5 ** 2) / 4), rel=1e-15)
    assert s["neg_mean"] == 1.75 / 12                             # the exact negative count: the histogram's total
    assert s["neg_std"] == pytest.approx(math.sqrt(1.875 / 12 - (1.75 / 12) ** 2), rel=1e-15)
    assert s["margin_mean"] == -0.1875 and s["margin_min"] == -0.75
    assert s["violations"] == 0.75                                # hard >= pos: rows 1, 2 and the tie of row 3
    conf = [math.exp(-1.0), math.exp(-1.0), math.exp(-1.0), math.exp(-1.0)]
    assert s["confidence_mean"] == pytest.approx(sum(conf) / 4, rel=1e-7)
    assert s["confidence_on_failures"] == pytest.approx(math.exp(-1.0), rel=1e-7)
    assert s["p_pos_mean"] == pytest.approx((2 * math.exp(-1.0) + math.exp(-1.25) + math.exp(-1.75)) / 4, rel=1e-7)
    assert s["out_of_range"] == 2 / 16
    rows, pred, c = diagnostics.failures(st)
    assert rows.tolist() == [1, 2] and pred.tolist() == [3, 0]
    assert torch.equal(c, st.confidence[rows])


def test_summary_reduces_in_f64():
    # 2^24 + 1 is not an f32: an f32 mean of these positives would lose the ones
    n = 4096
    pos = torch.full((n,), 1.0)
    pos[0] = 2.0 ** 24
    z, zi = torch.zeros(n), torch.zeros(n, dtype=torch.int64)
    st = diagnostics.SimilarityStats(labels=zi, pos=pos, best=pos, best_idx=zi, hard=z, hard_idx=zi, lse=pos,
                                     neg_sum=torch.full((n,), 0.1, dtype=torch.float64),
                                     neg_sumsq=torch.full((n,), 0.01, dtype=torch.float64),
                                     hist_neg=torch.tensor([0, n, 0]), hist_pos=torch.tensor([0, n, 0]),
                                     range=(-1.0, 1.0), scale=1.0, n_keys=2)
    s = st.summary()
    assert s["pos_mean"] == (2.0 ** 24 + (n - 1)) / n
    assert s["neg_mean"] == float(np.full(n, 0.1).sum()) / n
    assert s["confidence_on_failures"] != s["confidence_on_failures"]          # NaN: no failures


def test_confusion_matrix_and_rates_hand_made():
    st = _hand_made()                                             # predictions 0, 3, 0, 3
    conf = diagnostics.confusion_matrix(st, torch.tensor([0, 0, 1, 2]))
    assert conf.dtype == torch.int64
    assert conf.tolist() == [[1, 0, 1], [1, 0, 0], [0, 0, 1]]
    conf = diagnostics.confusion_matrix(st, torch.tensor([0, 0, 1, 1]), torch.tensor([1, 1, 1, 0]), num_groups=3)
    assert conf.tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 0]]
    rates = diagnostics.confusion_rates(conf, [(0, 1), (1, 0), (2, 0)])
    assert rates[(0, 1)] == 0.5 and rates[(1, 0)] == 0.5 and rates[(2, 0)] != rates[(2, 0)]
    with pytest.raises(ValueError, match="outside"):
        diagnostics.confusion_matrix(st, torch.tensor([0, 0, 1, 5]), num_groups=3)
    with pytest.raises(ValueError, match="groups_b"):
        diagnostics.confusion_matrix(st, torch.tensor([0, 0, 1, 1]), torch.tensor([0, 1]))
    st.best_idx = torch.tensor([0, -1, 0, 3])                     # a row without a prediction is skipped
    assert int(diagnostics.confusion_matrix(st, torch.tensor([0, 0, 1, 2])).sum()) == 3


def test_c_entry_points_refuse_bad_arguments():
    lib = _ffi.load()
    assert lib.clipk_version() == 7
    assert lib.clipk_sim_stats_workspace(10, 100, 64, 0) == 0
    assert lib.clipk_sim_stats_workspace(10, 100, 64, 257) == 0
    assert lib.clipk_sim_stats_workspace(0, 100, 64, 64) == 0
    assert lib.clipk_sim_stats_workspace(10, 0, 64, 64) == 0
    assert lib.clipk_sim_stats_workspace(10, 100, 62, 64) == 0
    assert lib.clipk_sim_stats_workspace(10, 100, 64, 64) > 0
    fake, ws = C.c_void_p(4096), C.c_void_p(8192)
    big = 1 << 30
    BAD, UNSUP = -1, -2
    outs = [fake] * 10

    def call(X=fake, Mx=4, Y=fake, Ny=100, P=8, labels=None, off=0, cx=None, cy=None, nbins=64, lo=-1.0, hi=1.0,
             o=outs, w=ws, wb=big):
        return lib.clipk_sim_stats(X, Mx, Y, Ny, P, 1.0, labels, off, cx, cy, nbins, lo, hi, *o, w, wb, None)

    assert call(X=None) == BAD
    assert call(Mx=0) == BAD
    assert call(P=6) == UNSUP
    assert call(off=97) == BAD and call(off=-1) == BAD
    assert call(cx=fake) == BAD and call(cy=fake) == BAD          # ids on one side only
    assert call(nbins=0) == BAD and call(nbins=257) == BAD
    assert call(lo=1.0, hi=1.0) == BAD and call(lo=float("nan")) == BAD and call(hi=float("inf")) == BAD
    assert call(X=C.c_void_p(4100)) == BAD
    assert call(wb=16) == BAD
    assert call(o=[fake] * 9 + [None]) == BAD
    assert call(o=[None] + [fake] * 9) == BAD


def test_split_option_changes_workspace():
    lib = _ffi.load()
    try:
        ops.set_option("retrieval_splits", 1)
        one = lib.clipk_sim_stats_workspace(64, 64 * 100, 64, 64)
        ops.set_option("retrieval_splits", 7)
        seven = lib.clipk_sim_stats_workspace(64, 64 * 100, 64, 64)
        assert seven == 7 * one
    finally:
        ops.reset_options()


def test_restated_binning_rule():
    # 4 bins over [-1, 1): width 0.5, every edge dyadic
    S = torch.tensor([-1.5, -1.0, -0.75, -0.5, -0.25, 0.0, 0.49999997, 0.5, 0.99999994, 1.0, 3.0])
    # 0.49999997 - lo rounds to 1.5 in f32: the rule bins the rounded difference, so the value sits in the upper bin;
    # 0.99999994 - lo rounds to 2.0, the product is nbins and the min keeps it in the last bin
    assert ref.slots(S, 4, -1.0, 1.0).tolist() == [0, 1, 1, 2, 2, 3, 4, 4, 4, 5, 5]
    assert float(ref.inv_width(4, -1.0, 1.0)) == 2.0
    # a non-dyadic width: the product may round up to nbins, the min keeps the value in the last bin
    lo, hi, n = -14.2857, 14.2857, 64
    top = torch.tensor([np.nextafter(np.float32(hi), np.float32(0))])
    assert ref.slots(top, n, lo, hi).tolist() == [n]
    S64 = torch.tensor([[0.5, 0.25, -0.5], [0.25, 0.75, 0.75]], dtype=torch.float64)
    r = ref.sim_stats(S64, torch.tensor([0, 1]), nbins=4)
    assert r["best_idx"].tolist() == [0, 1] and r["hard_idx"].tolist() == [1, 2]
    assert r["hist_neg"].tolist() == [0, 0, 1, 2, 1, 0] and r["hist_pos"].tolist() == [0, 0, 0, 0, 2, 0]
    assert r["neg_sum"].tolist() == [-0.25, 1.0] and r["n_neg"].tolist() == [2, 2]
    r = ref.sim_stats(S64, torch.tensor([0, 1]), torch.tensor([7, 8]), torch.tensor([7, 7, 8]), nbins=4)
    assert r["hard_idx"].tolist() == [2, 0] and r["n_neg"].tolist() == [1, 1]     # key 1 / key 2 excluded
    assert r["best_idx"].tolist() == [0, 1]


def _golden():
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "embedding_diagnostics.npz")
    return {k: v for k, v in np.load(path).items()}


def test_restatement_against_the_reference_fixture():
    """tests/golden/embedding_diagnostics.npz holds what the reference's own evaluate, compute_confusion_matrix,
    analyze_embedding_collapse and analyze_failure_cases (run1/full.py) return on a 96 x 32 case with 6 groups
    (tools/make_golden.py: gen_embedding_diagnostics); the f64 restatement must reproduce each of them."""
    z = _golden()
    a, b = torch.from_numpy(z["a"]), torch.from_numpy(z["b"])
    n, scale, G = a.shape[0], float(z["scale"]), 6
    assert a.shape == (96, 32) and z["cosine_sims"].shape == (96, 96)
    lab = torch.arange(n)
    S = scale * (a.double() @ b.double().t())
    r = ref.sim_stats(S, lab)
    assert int((r["best_idx"] == lab).sum()) / n == float(z["accuracy"])           # evaluate's accuracy
    conf = torch.from_numpy(z["confusion"])
    assert torch.equal(r["best_idx"], conf.argmax(1)) and int(conf.sum()) == n      # compute_confusion_matrix
    wrong = torch.nonzero(r["best_idx"] != lab).flatten()                           # analyze_failure_cases
    assert len(wrong) >= 10
    assert np.array_equal(wrong.numpy(), z["fail_rows"]) and np.array_equal(r["best_idx"][wrong].numpy(), z["fail_pred"])
    assert np.abs(torch.exp(r["best"] - r["lse"])[wrong].numpy() - z["fail_confidence"]).max() <= 1e-5
    cos = torch.from_numpy(z["cosine_sims"]).double()                               # evaluate's cosine_sims
    assert abs(float((r["neg_sum"].sum() + r["pos"].sum()) / n / n / scale) - float(cos.mean())) <= 1e-6
    assert float((r["pos"] / scale - cos.diag()).abs().max()) <= 1e-6
    off = ~torch.eye(n, dtype=torch.bool)
    assert float((r["hard"] / scale - cos.masked_fill(~off, float("-inf")).max(1).values).abs().max()) <= 1e-6
    # the histogram of the negatives at scale 1 against the fixture's matrix, up to values within 1e-6 of an edge
    r1 = ref.sim_stats(a.double() @ b.double().t(), lab, nbins=16)
    vals = torch.sort(cos[off]).values
    edges = torch.linspace(-1, 1, 17, dtype=torch.float64)
    allow = torch.searchsorted(vals, edges + 1e-6, right=True) - torch.searchsorted(vals, edges - 1e-6)
    cum = torch.cumsum(r1["hist_neg"], 0)[:17]
    assert ((cum - torch.searchsorted(vals, edges)).abs() <= allow).all() and int(r1["hist_neg"].sum()) == n * (n - 1)
    g = torch.from_numpy(z["groups"])                                               # analyze_embedding_collapse
    gs = ref.group_similarity(a, g, a, g, G)
    assert np.abs(gs.diag().numpy() - z["collapse"]).max() <= 1e-6
    # confusion counting of the package on the reference's predictions (CPU tensors: no kernel involved)
    st = _hand_made()
    st.best_idx, st.labels, st.n_keys = conf.argmax(1), lab, n
    assert torch.equal(diagnostics.confusion_matrix(st, lab, num_groups=n), conf)
    grouped = diagnostics.confusion_matrix(st, g, num_groups=G)
    want = torch.zeros(G, G, dtype=torch.int64)
    for t in range(n):
        want[g[t], g[conf[t].argmax()]] += 1
    assert torch.equal(grouped, want)
