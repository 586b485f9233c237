"""GPU: the fused similarity statistics (include/clipk.h: clipk_sim_stats, ops.sim_stats) and the diagnostics API on
top of them (clip_dplm_amd/diagnostics.py) against the f64 restatement of tests/sim_stats_ref.py.

Measured figures of the last run on an MI355X are printed before every assertion that has a tolerance."""
import pytest
import torch

from clip_dplm_amd import diagnostics, ops, retrieval

import sim_stats_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _grid_inputs(n, P, g, dev):
    """Entries in {-3..3}/4: every f32 product and partial sum is exact, so S equals the f64 product."""
    return (torch.randint(-3, 4, (n, P), generator=g).float() / 4).to(dev)


def _unit(n, P, g, dev, shared=0.0):
    v = torch.randn(n, P, generator=g, dtype=torch.float64)
    if shared:
        v = v + shared * P ** 0.5 * torch.eye(1, P, dtype=torch.float64)     # a common direction: negatives off zero
    return (v / v.norm(dim=1, keepdim=True)).float().to(dev)


def _check_exact(st, r, nbins, tag):
    for name in ("pos", "best", "hard", "neg_sum", "neg_sumsq"):
        assert torch.equal(getattr(st, name).double(), r[name]), (name, tag)
    for name in ("best_idx", "hard_idx", "hist_neg", "hist_pos"):
        assert torch.equal(getattr(st, name), r[name]), (name, tag)
    assert int(st.hist_neg.sum()) == int(r["n_neg"].sum()), tag
    assert int(st.hist_pos.sum()) == st.pos.numel(), tag
    assert st.hist_neg.numel() == nbins + 2


@pytest.mark.parametrize("P", [4, 60, 512, 1028])
@pytest.mark.parametrize("Ny", [1, 63, 4097, 100003])
def test_exact_inputs_bit_for_bit(dev, P, Ny):
    """Grid inputs, scale and bin edges dyadic: every S, every S - lo and every (S - lo) * inv_w is exact in f32, the
    sums are integers / 64 (squares / 4096) far below 2^53, and a lane's tile partial of 16 squares stays below 2^24
    units while |S| < 16 (8 standard deviations at P = 1028).  Everything but lse equals the f64 restatement."""
    g = torch.Generator().manual_seed(P * 11 + Ny)
    scale = 0.25
    x_all = _grid_inputs(1000, P, g, dev)
    y = _grid_inputs(Ny, P, g, dev)
    if Ny > 8:                                                     # duplicated gallery rows: exact ties
        src = torch.randint(0, Ny, (Ny // 8,), generator=g).to(dev)
        dst = torch.randint(0, Ny, (Ny // 8,), generator=g).to(dev)
        y[dst] = y[src]
    S = (x_all.double() @ y.double().t()) * scale
    labels_all = torch.randint(0, Ny, (1000,), generator=g).to(dev)
    cls_y = torch.randint(0, 10, (Ny,), generator=g).to(dev)
    cls_x_rand = torch.randint(0, 10, (1000,), generator=g).to(dev)
    for Mx in (1, 63, 65, 1000):
        x = x_all[:Mx].contiguous()
        modes = [("labels", labels_all[:Mx].contiguous(), 0)]
        if Mx <= Ny:
            off = (Ny - Mx) // 2
            modes.append(("offset", None, off))
        for mode, labels, off in modes:
            lab = labels if labels is not None else torch.arange(off, off + Mx, device=dev)
            for ids in (False, True):
                cx = cy = None
                if ids:                                            # the positive's class, or unrelated ids
                    cx, cy = (cls_y[lab].contiguous() if mode == "labels" else cls_x_rand[:Mx].contiguous()), cls_y
                for nbins, lo, hi in ((64, -8.0, 8.0), (8, -0.5, 0.5)):      # the second: most values in the outer slots
                    if (nbins, ids) == (8, True) and Mx not in (65, 1000):
                        continue
                    tag = (Mx, Ny, P, mode, ids, nbins)
                    st = ops.sim_stats(x, y, scale=scale, labels=labels, label_offset=off, cls_x=cx, cls_y=cy,
                                       nbins=nbins, lo=lo, hi=hi)
                    r = ref.sim_stats(S[:Mx], lab, cx, cy, nbins, lo, hi)
                    _check_exact(st, r, nbins, tag)
                    if nbins == 8 and Ny > 63 and P >= 60:
                        assert int(st.hist_neg[0]) > 0 and int(st.hist_neg[-1]) > 0, tag
                    del r
                if not ids:                                        # the entry points it subsumes: the same bits
                    s1, i1 = ops.sim_topk(x, y, 1, scale=scale)
                    assert torch.equal(st.best, s1[:, 0]) and torch.equal(st.best_idx, i1[:, 0]), tag
                    _, pos = ops.sim_rank(x, y, labels=labels, label_offset=off, scale=scale)
                    assert torch.equal(st.pos, pos), tag


PLAN_FREE = ("pos", "best", "best_idx", "hard", "hard_idx", "hist_neg", "hist_pos")


@pytest.mark.parametrize("ids", [False, True])
def test_split_plans_and_runs(dev, kopt, ids):
    g = torch.Generator().manual_seed(21)
    x, y = _unit(300, 128, g, dev), _unit(30011, 128, g, dev)
    labels = torch.randint(0, 30011, (300,), generator=g).to(dev)
    cy = torch.randint(0, 10, (30011,), generator=g).to(dev) if ids else None
    cx = cy[labels].contiguous() if ids else None
    kw = dict(scale=14.2857, labels=labels, cls_x=cx, cls_y=cy)
    base = ops.sim_stats(x, y, **kw)
    xg, yg = _grid_inputs(130, 60, g, dev), _grid_inputs(5000, 60, g, dev)
    base_g = ops.sim_stats(xg, yg, scale=0.25, nbins=64, lo=-8.0, hi=8.0)
    for s in (1, 3, 8):
        kopt("retrieval_splits", s)
        a = ops.sim_stats(x, y, **kw)
        b = ops.sim_stats(x, y, **kw)
        for name, ta, tb in zip(a._fields, a, b):
            assert torch.equal(ta, tb), (name, s)                  # two runs of one plan: every output
        for name in PLAN_FREE:
            assert torch.equal(getattr(a, name), getattr(base, name)), (name, s)
        print(f"splits={s}: max |lse - lse_auto| = {float((a.lse - base.lse).abs().max()):.3e}")
        assert float((a.lse - base.lse).abs().max()) <= 4e-5       # each within 2e-5 of the f64 value (test below)
        ag = ops.sim_stats(xg, yg, scale=0.25, nbins=64, lo=-8.0, hi=8.0)
        for name in PLAN_FREE + ("neg_sum", "neg_sumsq"):          # exact inputs: the sums are plan-free too
            assert torch.equal(getattr(ag, name), getattr(base_g, name)), (name, s)


@pytest.mark.parametrize("ids", [False, True])
@pytest.mark.parametrize("P", [120, 128, 512])
def test_random_unit_vectors_against_f64(dev, P, ids):
    g = torch.Generator().manual_seed(P + 1)
    Mx, Ny, scale, nbins = 300, 30011, 14.2857, 64
    x, y = _unit(Mx, P, g, dev), _unit(Ny, P, g, dev)
    labels = torch.randint(0, Ny, (Mx,), generator=g).to(dev)
    cy = torch.randint(0, 10, (Ny,), generator=g).to(dev) if ids else None
    cx = cy[labels].contiguous() if ids else None
    st = ops.sim_stats(x, y, scale=scale, labels=labels, cls_x=cx, cls_y=cy, nbins=nbins)
    S = scale * (x.double() @ y.double().t())
    r = ref.sim_stats(S, labels, cx, cy, nbins, -scale, scale)
    tol = 2e-5 * scale                                             # the per-logit bar of test_gpu_retrieval.py
    rows = torch.arange(Mx, device=dev)
    for name in ("pos", "best", "hard"):
        err = float((getattr(st, name).double() - r[name]).abs().max())
        print(f"P={P} ids={ids} {name}: max err {err:.3e} (bar {tol:.3e})")
        assert err <= tol, name
    # indices: valid members of their set, and the reference value there is within the window of the reference maximum
    assert r["keep_mask"][rows, st.best_idx].all() and r["neg_mask"][rows, st.hard_idx].all()
    assert (S[rows, st.best_idx] >= r["best"] - tol).all()
    assert (S[rows, st.hard_idx] >= r["hard"] - tol).all()
    err = float((st.lse.double() - r["lse"]).abs().max())
    print(f"P={P} ids={ids} lse: max err {err:.3e} (bar 2e-5)")
    assert err <= 2e-5
    # histogram: cumulative counts at every edge, allowed to differ by the reference logits within tol of the edge
    vals = torch.sort(S[r["neg_mask"]]).values
    edges = torch.linspace(-scale, scale, nbins + 1, dtype=torch.float64, device=dev)
    cum_ref = torch.searchsorted(vals, edges, right=False)
    allow = torch.searchsorted(vals, edges + tol, right=True) - torch.searchsorted(vals, edges - tol, right=False)
    cum_gpu = torch.cumsum(st.hist_neg, 0)[:nbins + 1]             # slots 0 .. b lie below edge b
    share = float(allow.sum()) / (Mx * Ny)
    worst = float(((cum_gpu - cum_ref).abs().double() / allow.clamp(min=1)).max())
    print(f"P={P} ids={ids} histogram: allowances are {100 * share:.3f} % of Mx Ny, "
          f"max |cum_gpu - cum_ref| / allowance = {worst:.3f}, max diff {int((cum_gpu - cum_ref).abs().max())}")
    assert share < 0.01                                            # the cap is a real one for these inputs
    assert ((cum_gpu - cum_ref).abs() <= allow).all()
    assert int(st.hist_neg.sum()) == int(r["n_neg"].sum()) and int(st.hist_pos.sum()) == Mx
    pv = torch.sort(r["pos"]).values                               # the positives: the same rule
    allow_p = torch.searchsorted(pv, edges + tol, right=True) - torch.searchsorted(pv, edges - tol, right=False)
    cum_p = torch.searchsorted(pv, edges, right=False)
    assert ((torch.cumsum(st.hist_pos, 0)[:nbins + 1] - cum_p).abs() <= allow_p).all()
    # the f64 sums against the bounds of include/clipk.h, evaluated from the f64 reference and used as they are:
    # (1) the guaranteed ones over Sabs = |scale| <|x|, |y|>, (2) the same constants over |S| (the form the sums are
    # specified in; no cancellation to speak of in these rows)
    neg = r["neg_mask"]
    Sabs = scale * (x.double().abs() @ y.double().abs().t())
    e1, e2 = (st.neg_sum - r["neg_sum"]).abs(), (st.neg_sumsq - r["neg_sumsq"]).abs()
    g1, g2 = (P + 18) * U * (Sabs * neg).sum(1), (2 * P + 24) * U * (Sabs * Sabs * neg).sum(1)
    w1, w2 = (P + 18) * U * (S.abs() * neg).sum(1), (2 * P + 24) * U * (S * S * neg).sum(1)
    print(f"P={P} ids={ids} neg_sum: max err / guaranteed {float((e1 / g1).max()):.3e}, / working {float((e1 / w1).max()):.3e}; "
          f"neg_sumsq: / guaranteed {float((e2 / g2).max()):.3e}, / working {float((e2 / w2).max()):.3e}")
    assert (e1 <= g1).all() and (e2 <= g2).all()
    assert (e1 <= w1).all() and (e2 <= w2).all()


def test_sums_accumulate_in_f64_above_the_tile(dev):
    """Rows with a shared direction: every logit is positive, the row sum grows like Ny.  include/clipk.h: with the
    roundings of a logit and of a tile's 16 additions as independent errors bounded by (P + 18) u |S_ij|, the error of a
    row sum stays below 6 (P + 18) u sqrt(sum_j S_ij^2) (Hoeffding, 2 exp(-18) per row); the squares likewise with
    (2 P + 24) u S_ij^2.  A running f32 sum above the tile would add, per lane, Ny / 64 roundings of size up to
    u * (sum so far): about u sum_j S_ij sqrt(Ny / 192) / 4 over the four lanes of a query.  At Ny = 2^20, P = 64 and
    logits near their mean m that is ~ 2e7 u m against the asserted 5e5 u m: the assertion separates the two by a
    factor of about 40, which the test prints from its own inputs before asserting."""
    g = torch.Generator().manual_seed(77)
    Mx, Ny, P, scale = 64, 1 << 20, 64, 14.2857
    x, y = _unit(Mx, P, g, dev, shared=2.0), _unit(Ny, P, g, dev, shared=2.0)
    st = ops.sim_stats(x, y, scale=scale)
    S = scale * (x.double() @ y.double().t())
    lab = torch.arange(Mx, device=dev)
    s_min = float(S.min())
    S[lab, lab] = 0.0                                              # the positives are not negatives
    want1, want2 = S.sum(1), (S * S).sum(1)
    e1, e2 = (st.neg_sum - want1).abs(), (st.neg_sumsq - want2).abs()
    b1 = 6 * (P + 18) * U * (S * S).sum(1).sqrt()
    b2 = 6 * (2 * P + 24) * U * (S ** 4).sum(1).sqrt()
    f32_running = U * want1.abs() * (Ny / 192) ** 0.5 / 4
    assert s_min > 0 and float((f32_running / b1).min()) > 10       # the inputs separate the two
    print(f"shared direction, Ny = 2^20: neg_sum max err / bound {float((e1 / b1).max()):.3e}, neg_sumsq "
          f"{float((e2 / b2).max()):.3e}; an f32 running sum would sit at {float((f32_running / b1).min()):.1f}"
          f" .. {float((f32_running / b1).max()):.1f} of the bound; err / (2^-24 sum |S|) {float((e1 / (U * want1)).max()):.3e}")
    assert (e1 <= b1).all() and (e2 <= b2).all()
    assert (e1 <= (P + 18) * U * want1).all() and (e2 <= (2 * P + 24) * U * want2).all()
    assert int(st.hist_neg.sum()) == Mx * (Ny - 1)


def test_out_of_range_device_labels(dev):
    g = torch.Generator().manual_seed(4)
    x, y = _unit(70, 64, g, dev), _unit(300, 64, g, dev)
    labels = torch.randint(0, 300, (70,), generator=g).to(dev)
    good = ops.sim_stats(x, y, labels=labels, nbins=16)
    bad = labels.clone()
    bad[3], bad[40] = -1, 300
    st = ops.sim_stats(x, y, labels=bad, nbins=16)
    ok = torch.ones(70, dtype=torch.bool, device=dev)
    ok[3] = ok[40] = False
    assert torch.isnan(st.pos[~ok]).all() and (st.best_idx[~ok] == -1).all() and (st.hard_idx[~ok] == -1).all()
    for name in ("pos", "best", "best_idx", "hard", "hard_idx", "lse", "neg_sum", "neg_sumsq"):
        assert torch.equal(getattr(st, name)[ok], getattr(good, name)[ok]), name
    only = ops.sim_stats(x[ok], y, labels=labels[ok], nbins=16)    # the two rows contribute to no histogram
    assert torch.equal(st.hist_neg, only.hist_neg) and torch.equal(st.hist_pos, only.hist_pos)
    assert int(st.hist_pos.sum()) == 68 and int(st.hist_neg.sum()) == 68 * 299
    s = diagnostics.similarity_stats(x, y, labels=bad, bins=16).summary()
    assert s["n"] == 68


def test_single_key_gallery_has_no_negatives(dev):
    x = torch.ones(5, 4, device=dev) / 2
    st = ops.sim_stats(x, torch.ones(1, 4, device=dev) / 2, labels=torch.zeros(5, dtype=torch.int64, device=dev))
    assert (st.hard == float("-inf")).all() and (st.hard_idx == -1).all() and int(st.hist_neg.sum()) == 0
    assert torch.equal(st.pos, torch.ones(5, device=dev)) and torch.equal(st.lse, st.pos) and (st.neg_sum == 0).all()


# ------------------------------------------------------------------------------------------------ API level
def _api_case(dev):
    g = torch.Generator().manual_seed(31)
    n, P, G = 2000, 128, 12
    a = _unit(n, P, g, dev, shared=0.25)
    noise = torch.randn(n, P, generator=g).to(dev) / P ** 0.5
    b = a + 3.0 * noise
    b = (b.double() / b.double().norm(dim=1, keepdim=True)).float()
    groups = torch.randint(0, G, (n,), generator=g).to(dev)
    return a, b, groups, G


def _neg_tolerances(a, b, scale, mask, want):
    """Bounds of neg_mean and neg_std from the header's bounds of the two sums."""
    Sabs = scale * (a.double().abs() @ b.double().abs().t())
    n = float(mask.sum())
    b1 = float((128 + 18) * U * (Sabs * mask).sum()) / n
    b2 = float((2 * 128 + 24) * U * (Sabs * Sabs * mask).sum()) / n
    dvar = b2 + 2 * abs(want["neg_mean"]) * b1 + b1 * b1
    return max(b1, 1e-6 * abs(want["neg_mean"])), max(dvar / (2 * want["neg_std"]), 1e-6 * want["neg_std"])


@pytest.mark.parametrize("ids", [False, True])
def test_summary_failures_confusion(dev, ids):
    a, b, groups, G = _api_case(dev)
    scale = 14.2857
    cls = groups if ids else None                                  # pairs of one group: not each other's negatives
    st = diagnostics.similarity_stats(a, b, scale=scale, class_ids=cls)
    S = scale * (a.double() @ b.double().t())
    lab = torch.arange(2000, device=dev)
    r = ref.sim_stats(S, lab, cls, cls)
    want = ref.summary(S, lab, cls, cls)
    got = st.summary()
    bar = 2e-5 * scale
    t_mean, t_std = _neg_tolerances(a, b, scale, r["neg_mask"], want)
    for k in sorted(want):
        print(f"ids={ids} {k}: got {got[k]!r} want {want[k]!r}")
    assert got["n"] == 2000
    assert 0.05 < want["top1"] < 0.999                             # the case has failures and successes
    assert got["top1"] == want["top1"] and got["violations"] == want["violations"]      # counts: exact
    for k in ("pos_mean", "pos_std"):
        assert abs(got[k] - want[k]) <= 1e-6 * abs(want[k]), k
    # a difference of two means, 1e-6 relative each
    assert abs(got["margin_mean"] - want["margin_mean"]) <= 1e-6 * (abs(want["pos_mean"]) + abs(float(r["hard"].mean())))
    assert abs(got["neg_mean"] - want["neg_mean"]) <= t_mean
    assert abs(got["neg_std"] - want["neg_std"]) <= t_std
    assert abs(got["margin_min"] - want["margin_min"]) <= 2 * bar
    for k in ("confidence_mean", "confidence_on_failures", "p_pos_mean"):     # exp(v - lse): both bars, values <= 1
        assert abs(got[k] - want[k]) <= bar + 2e-5, k
    assert got["out_of_range"] == 0.0
    # failures
    rows, pred, conf = diagnostics.failures(st)
    wrong = torch.nonzero(r["best_idx"] != lab).flatten()
    assert torch.equal(rows, wrong) and torch.equal(pred, r["best_idx"][wrong])
    assert ((conf.double() - torch.exp(r["best"] - r["lse"])[wrong]).abs() <= bar + 2e-5).all()
    # confusion matrix: integer counting of (group of the query, group of the predicted key)
    cm = diagnostics.confusion_matrix(st, groups, num_groups=G)
    want_cm = torch.bincount(groups * G + groups[r["best_idx"]], minlength=G * G).reshape(G, G)
    assert torch.equal(cm, want_cm) and int(cm.sum()) == 2000
    rates = diagnostics.confusion_rates(cm, [(0, 1), (3, 3)])
    assert rates[(0, 1)] == float(want_cm[0, 1]) / float(want_cm[0].sum())
    with pytest.raises(ValueError, match="but b on"):
        diagnostics.similarity_stats(a, b.cpu())


def test_uniformity_alignment_group_similarity(dev):
    a, b, groups, G = _api_case(dev)
    u, want = diagnostics.uniformity(a), ref.uniformity(a)
    print(f"uniformity: got {u!r} want {want!r}")
    assert abs(u - want) <= 2e-4                                   # lse (2e-5) and pos (2e-5 * 4) bars, conditioning ~1
    al = diagnostics.alignment(a, b)
    want_al = float((a.double() - b.double()).pow(2).sum(1).mean())
    print(f"alignment: got {al!r} want {want_al!r}")
    assert abs(al - want_al) <= 1e-6
    raw_a, raw_b = a * 3.0, b * torch.linspace(0.5, 2.0, 2000, device=dev)[:, None]     # not unit rows: normalised inside
    gb = torch.randint(0, G, (2000,), generator=torch.Generator().manual_seed(5)).to(dev)
    for got, want_gs in ((diagnostics.group_similarity(raw_a, groups), ref.group_similarity(a, groups, a, groups, G)),
                         (diagnostics.group_similarity(raw_a, groups, raw_b, gb, num_groups=G),
                          ref.group_similarity(a, groups, b, gb, G))):
        err = float((got.double() - want_gs).abs().max())
        print(f"group_similarity: max err {err:.3e}")
        assert got.dtype == torch.float32 and got.shape == (G, G) and err <= 1e-6
    assert torch.equal(diagnostics.group_similarity(raw_a, groups), diagnostics.group_similarity(raw_a, groups))


def test_evaluate_embeddings_on_a_model(dev):
    import clip_dplm_amd as K
    torch.manual_seed(8)
    m = K.RNARBPCLIPModel(rna_dim=40, rbp_dim=128, projection_dim=64, dropout=0.0).to(dev)
    g = torch.Generator().manual_seed(9)
    loader = [tuple(torch.randn(96, *sh, generator=g).to(dev) for sh in [(5, 40), (5, 128)]) for _ in range(3)]
    out = diagnostics.evaluate_embeddings(m, loader)
    assert set(out) == {"a_to_b", "b_to_a", "a", "b", "alignment", "modality_gap"}
    assert set(out["a"]) == {"uniformity", "self_neg_mean"} and set(out["b"]) == set(out["a"])
    want = retrieval.evaluate_retrieval(m, loader)
    assert out["a_to_b"]["top1"] == want["a_to_b"]["top1"] and out["b_to_a"]["top1"] == want["b_to_a"]["top1"]
    assert out["a_to_b"]["n"] == 288
    m.eval()
    with torch.no_grad():
        pairs = [retrieval.default_embed_fn(m, bt) for bt in loader]
    a, b = torch.cat([p[0] for p in pairs]).double(), torch.cat([p[1] for p in pairs]).double()
    assert abs(out["alignment"] - float((a - b).pow(2).sum(1).mean())) <= 1e-5
    assert abs(out["modality_gap"] - float((a.mean(0) - b.mean(0)).norm())) <= 1e-6
    assert abs(out["a"]["uniformity"] - ref.uniformity(a)) <= 2e-4
    C = a @ a.t()
    assert abs(out["a"]["self_neg_mean"] - float((C.sum() - C.diag().sum()) / (288 * 287))) <= 1e-6
    ids_fn = lambda batch: torch.arange(batch[0].shape[0]) % 7      # class ids per batch row
    out2 = diagnostics.evaluate_embeddings(m, loader, class_ids_fn=ids_fn, scale=10.0, bins=16)
    assert out2["a_to_b"]["top1"] >= out["a_to_b"]["top1"]


def test_package_against_the_reference_fixture(dev):
    """The package on the inputs of tests/golden/embedding_diagnostics.npz against what the reference's evaluate,
    compute_confusion_matrix, analyze_embedding_collapse and analyze_failure_cases returned for them."""
    import os
    import numpy as np
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "embedding_diagnostics.npz"))
    a, b = torch.from_numpy(z["a"]).to(dev), torch.from_numpy(z["b"]).to(dev)
    g = torch.from_numpy(z["groups"]).to(dev)
    n, scale, G = 96, float(z["scale"]), 6
    st = diagnostics.similarity_stats(a, b, scale=scale)
    assert st.summary()["top1"] == float(z["accuracy"])
    conf = torch.from_numpy(z["confusion"]).to(dev)
    assert torch.equal(diagnostics.confusion_matrix(st, torch.arange(n, device=dev), num_groups=n), conf)
    want = torch.bincount(g * G + g[conf.argmax(1)], minlength=G * G).reshape(G, G)
    assert torch.equal(diagnostics.confusion_matrix(st, g, num_groups=G), want)
    rows, pred, confid = diagnostics.failures(st)
    assert np.array_equal(rows.cpu().numpy(), z["fail_rows"]) and np.array_equal(pred.cpu().numpy(), z["fail_pred"])
    err = float(np.abs(confid.double().cpu().numpy() - z["fail_confidence"]).max())
    print(f"fixture confidence: max err {err:.3e}")
    assert err <= 2e-5 * scale + 2e-5                              # the logit and lse bars; values <= 1
    cos = torch.from_numpy(z["cosine_sims"]).double().to(dev)
    s1 = diagnostics.similarity_stats(a, b, scale=1.0, bins=16)
    mean_cos = float((s1.neg_sum.sum() + s1.pos.double().sum()) / n / n)
    print(f"fixture mean cosine: got {mean_cos!r} want {float(cos.mean())!r}")
    assert abs(mean_cos - float(cos.mean())) <= 1e-6
    off = ~torch.eye(n, dtype=torch.bool, device=dev)
    assert float((s1.pos.double() - cos.diag()).abs().max()) <= 2e-5
    assert float((s1.hard.double() - cos.masked_fill(~off, float("-inf")).max(1).values).abs().max()) <= 2e-5
    vals = torch.sort(cos[off]).values
    edges = torch.linspace(-1, 1, 17, dtype=torch.float64, device=dev)
    allow = torch.searchsorted(vals, edges + 2e-5, right=True) - torch.searchsorted(vals, edges - 2e-5)
    assert ((torch.cumsum(s1.hist_neg, 0)[:17] - torch.searchsorted(vals, edges)).abs() <= allow).all()
    gs = diagnostics.group_similarity(a, g, num_groups=G)
    assert float(np.abs(gs.diag().double().cpu().numpy() - z["collapse"]).max()) <= 1e-6
