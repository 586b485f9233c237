"""CPU: tests/simce_ref.py, the yardstick of tests/test_gpu_simce.py, checked before anything is compared with it.

  * the reference agrees with torch.autograd of F.cross_entropy in f64 on every data family, and with
    class_aware_ref / hard_negative_ref where they overlap (distinct ids with eps 0; beta 0);
  * a numpy-f32 stand-in written here - an fma-ordered f32 dot product, f32 exp / log, the online-softmax merge in 64-key
    tiles and key splits, an f32 gradient - stays inside every bound on every family;
  * each seeded fault, applied to the stand-in, falls OUTSIDE the bound on the inputs the GPU file uses: the bounds
    discriminate;
  * the plan restatement gives the tiles per split and split counts the shapes were chosen for.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import class_aware_ref as CA  # noqa: E402
import hard_negative_ref as HN  # noqa: E402
import simce_ref as R  # noqa: E402

F32 = np.float32
W_ROW, W_COL = 0.5, 0.5


# ---------------------------------------------------------------------------------------------- plans
def test_plan_numbers_of_the_shape_table():
    two, three, many = (R.SHAPES[k] for k in ("two-tile", "three-tile", "many-splits"))
    # (nqb, ntiles, tiles per split, splits)
    assert R.tiled_plan(two[0], two[1] + two[2]) == (24, 25, 2, 13)
    assert R.tiled_plan(three[0], three[1] + three[2]) == (32, 33, 3, 11)
    assert R.tiled_plan(many[0], many[1] + many[2]) == (2, 67, 1, 67)
    assert R.tiled_plan(R.BATCHED_B, R.BATCHED_B, 6) == (10, 10, 2, 5)
    for P in R.SHAPE_P["two-tile"]:
        assert R.first_gen_plan(two[0], two[1] + two[2], P)[:4] == (47, 50, 5, 10)
    assert R.first_gen_plan(three[0], three[1] + three[2], 20)[:4] == (64, 66, 9, 8)
    for P in R.SHAPE_P["many-splits"]:
        assert R.first_gen_plan(many[0], many[1] + many[2], P)[:4] == (3, 133, 1, 133)
    assert R.first_gen_plan(R.BATCHED_PLAIN_B, R.BATCHED_PLAIN_B, R.BATCHED_PLAIN_P)[:4] == (25, 25, 2, 13)
    # two-tile: the batch / cache boundary (1510) inside the second tile of split 11; the last split one tile of 34 keys
    assert 1510 // 64 == 23 and 23 // 2 == 11 and 23 % 2 == 1 and 1570 - 24 * 64 == 34
    # the first-generation gradient pass itself at P = 32; P = 36 (Pw = 40) is rerouted to the tiled pass
    assert R.first_gen_plan(1500, 1570, 32)[4:] == (1, 32) and not R.grad_takes_tiled(1500, 1570, 32, 1)
    assert R.first_gen_plan(1500, 1570, 36)[4:] == (1, 40) and R.grad_takes_tiled(1500, 1570, 36, 1)
    Mx, Ny, Nc, _ = R.SHAPES["sweep"]
    # waves and slices of the sweep: ragged last waves at 132, 260, 516, 956; full ones at 960
    assert [R.first_gen_plan(Mx, Ny + Nc, P)[4:] for P in R.SWEEP_P_FIRST_LSE] == \
        [(1, 8), (2, 72), (4, 72), (8, 72), (8, 120), (8, 120)]
    assert [R.first_gen_plan(Mx, Ny + Nc, P)[4:] for P in R.SWEEP_P_FIRST_GRAD] == \
        [(1, 32), (1, 96), (2, 96), (4, 96), (8, 96)]
    assert all(not R.grad_takes_tiled(Mx, Ny + Nc, P, 1) for P in R.SWEEP_P_FIRST_GRAD)
    # forced reroutes; 508 and 512 give four full-width slices (the last one ragged at 508) and stay on the first pass
    assert [R.grad_takes_tiled(Mx, Ny + Nc, P, 1) for P in R.SWEEP_P_TILED] == [True, True, True, True, False, False]
    # refused by the first plan: more than 1024, not a multiple of 4, or 8 waves of 128 columns (LDS)
    assert all(R.first_gen_plan(Mx, Ny + Nc, P) is None for P in (6, 1028, 964, 1020, 1024))
    # tiled gradient: p-tiles per wave ceil(P / 128) = 1 .. 4, ragged at 132, 260, 388, 508
    assert [-(-P // 128) for P in R.SWEEP_P_TILED] == [1, 2, 3, 4, 4, 4]
    # tiny shapes: one tile on the tiled pass, one or two on the first
    for Mx, Ny, Nc, _ in R.TINY:
        assert R.tiled_plan(Mx, Ny + Nc)[1] in (1, 2) and R.first_gen_plan(Mx, Ny + Nc, 4)[1] in (1, 2, 3)


def test_the_loss_module_has_the_slice_rule_of_the_plan():
    """clip_dplm_amd.loss._tri_plain_slice_ok (which gradient pass the plain tri-modal loss takes) against the
    restatement of make_plan, at every width the first plan accepts."""
    from clip_dplm_amd.loss import _tri_plain_slice_ok
    for P in range(4, 961, 4):
        assert _tri_plain_slice_ok(P) == (R.first_gen_plan(100, 100, P)[5] % 32 == 0), P
    assert all(_tri_plain_slice_ok(P) for P in (28, 32, 64, 128, 192, 508, 512, 768))
    assert not any(_tri_plain_slice_ok(P) for P in (4, 16, 36, 48, 160, 320, 516, 640))


def test_planted_keys_reach_every_merge_level():
    Mx, Ny, Nc, off = R.SHAPES["two-tile"]
    tps = R.tiled_plan(Mx, Ny + Nc)[2]
    pl = R.plant_keys(Mx, Ny, Nc, off, tps)
    rows, keys = [r for r, _ in pl], [j for _, j in pl]
    assert len(set(rows)) == len(rows) and len(set(keys)) == len(keys) and len(pl) >= 9
    split = lambda j: j // (64 * tps)
    assert any(j == off + r for r, j in pl)                                              # the diagonal
    assert any(split(j) != split(off + r) and (j // 64) % tps == 0 for r, j in pl)       # first tile, another split
    assert any(split(j) != split(off + r) and (j // 64) % tps == 1 for r, j in pl)       # second tile: rescaled
    assert any(j % 64 >= 32 and j % 8 >= 4 for j in keys)                                # key-wave 1, lane half 1
    assert any(j % 64 < 32 and j % 8 >= 4 for j in keys)
    assert any(Ny <= j < Ny + Nc - 1 for j in keys) and Ny + Nc - 1 in keys              # cache, the last key
    a, b, cache, scale = R.pair_batch("B", Mx, Ny, Nc, off, 36, 1, tps)
    L = R.Logits(a[off:off + Mx], b, cache, scale)
    for r, j in pl:                                             # cos = 1: logit 100 (to f32 rounding), the row's maximum
        assert abs(L.S[r, j].item() - 100.0) < 1e-4 and L.S[r].argmax().item() == j


# ---------------------------------------------------------------------------------------------- reference
def _case(family, shape="two-tile", P=36, seed=11):
    Mx, Ny, Nc, off = R.SHAPES[shape] if isinstance(shape, str) else shape
    tps = R.tiled_plan(Mx, Ny + Nc)[2]
    a, b, cache, scale = R.pair_batch(family, Mx, Ny, Nc, off, P, seed, tps)
    return Mx, Ny, Nc, off, a, b, cache, scale, tps


def _autograd_G(a, b, cache, scale, off, Mx):
    """dL/dZ on the logits Z = scale a_g [b_g | cache]^T of the whole batch, L = w_row sum_{rows} CE + w_col sum_keys CE."""
    K = b if cache is None else torch.cat([b, cache])
    Ny = b.shape[0]
    Z = (scale * a.double() @ K.double().t()).requires_grad_(True)
    rows = torch.arange(off, off + Mx)
    L = W_ROW * F.cross_entropy(Z[rows], rows, reduction="sum") \
        + W_COL * F.cross_entropy(Z[:, :Ny].t(), torch.arange(Ny), reduction="sum")
    G, = torch.autograd.grad(L, Z)
    return Z.detach(), G[rows], K.double()


@pytest.mark.parametrize("family", ["A", "B", "C"])
def test_reference_agrees_with_autograd(family):
    Mx, Ny, Nc, off, a, b, cache, scale, _ = _case(family)
    Z, G, K = _autograd_G(a, b, cache, scale, off, Mx)
    lse_y = torch.logsumexp(Z[:, :Ny], 0)
    x = a[off:off + Mx]
    ref = R.simce_ref(x, b, cache, scale, off, torch.logsumexp(Z[off:off + Mx], 1), lse_y, W_ROW, W_COL, 1.0 / Ny)
    ce = F.cross_entropy(Z[off:off + Mx], torch.arange(off, off + Mx), reduction="none")
    assert torch.allclose(ref["lse"] - ref["pos"], ce, rtol=0, atol=1e-11)
    D = x.double() @ K.t()
    assert torch.allclose(ref["dX"], scale * G @ K / Ny, rtol=1e-12, atol=1e-15)
    assert torch.allclose(ref["dscale"], (G * D).sum(1) / Ny, rtol=1e-12, atol=1e-15)
    up = R.simce_ref(x, b, cache, scale, off, torch.logsumexp(Z[off:off + Mx], 1), lse_y, W_ROW, W_COL, 1.0 / Ny,
                     upstream=torch.tensor(-1.75))
    assert torch.allclose(up["dX"], -1.75 * ref["dX"], rtol=1e-12, atol=1e-18)
    assert torch.allclose(up["b_dX"], 1.75 * ref["b_dX"], rtol=1e-12, atol=0)
    for k in ("b_lse", "b_pos", "b_dX", "b_dscale"):
        assert bool((ref[k] > 0).all()) and bool(torch.isfinite(ref[k]).all())


@pytest.mark.parametrize("family", ["A", "B"])
def test_reference_agrees_with_the_variants_where_they_overlap(family):
    Mx, Ny, Nc, off, a, b, cache, scale, _ = _case(family)
    x = a[off:off + Mx]
    L = R.Logits(x, b, cache, scale)
    Lc = R.Logits(b, a, None, scale)
    lse, pos, _, _ = R.plain_stats(L, off)
    lse_y = R.plain_stats(Lc, 0)[0]
    dX, dsc, _, _ = R.plain_grad(L, off, lse, lse_y, W_ROW, W_COL, 1.0 / Ny)
    ids = R.class_ids("distinct", Ny)
    for cls in (None, ids):                                     # distinct ids, eps 0: the plain loss
        cx = None if cls is None else cls[off:off + Mx]
        st = R.cls_stats(L, off, cx, cls, "mask", 0.0)
        assert torch.equal(st["lse"], lse) and torch.equal(st["tgt"], pos) and bool((st["cnt"] == 1).all())
        one = torch.ones(Ny)
        g = R.cls_grad(L, off, lse, lse_y, one[:Mx], one, cx, cls, "mask", 0.0, Ny, W_ROW, W_COL, 1.0 / Ny)
        assert torch.allclose(g[0], dX, rtol=1e-13, atol=0) and torch.allclose(g[1], dsc, rtol=1e-13, atol=1e-18)
        hs = R.hard_stats(L, off, cx, cls, 0.0)                                    # beta 0: the plain loss
        assert torch.allclose(hs["lse_h"], lse, rtol=0, atol=1e-11) and torch.equal(hs["pos"], pos)
        hc = R.hard_stats(Lc, 0, cls, cls, 0.0)
        hg = R.hard_grad(L, off, hs["coef"], hc["coef"], cx, cls, 0.0, W_ROW, W_COL, 1.0 / Ny)
        assert torch.allclose(hg[0], dX, rtol=1e-9, atol=1e-15)
    # with classes and beta 0.5: hard_grad is hard_negative_ref.simce_grad_hard
    cls = R.class_ids("runs", Ny)
    cx = cls[off:off + Mx]
    hs, hc = R.hard_stats(L, off, cx, cls, 0.5), R.hard_stats(Lc, 0, cls, cls, 0.5)
    got = R.hard_grad(L, off, hs["coef"], hc["coef"], cx, cls, 0.5, W_ROW, W_COL, 1.0 / Ny, upstream=-1.75)
    want = HN.simce_grad_hard(x.double(), b.double(), torch.tensor(scale, dtype=R.F64), 0.5, hs["coef"], hc["coef"], W_ROW,
                              W_COL, 1.0 / Ny, cls_x=cx, cls_y=cls, label_offset=off,
                              cache=None if cache is None else cache.double(), upstream=torch.tensor(-1.75, dtype=R.F64))
    assert torch.allclose(got[0], want[0], rtol=1e-11, atol=1e-16) and torch.allclose(got[1], want[1], rtol=1e-11, atol=1e-16)
    assert bool((got[2] > 0).all()) and bool(torch.isfinite(got[2]).all()) and bool(torch.isfinite(got[3]).all())
    # with classes: cls_grad is class_aware_ref.simce_grad_cls
    ids = R.class_ids("runs", Ny)
    for mode, eps in (("mask", 0.1), ("positive", 0.1), ("positive", 0.0)):
        st, sc = R.cls_stats(L, off, ids[off:off + Mx], ids, mode, eps), R.cls_stats(Lc, 0, ids, ids, mode, eps)
        got = R.cls_grad(L, off, st["lse"], sc["lse"], st["cnt"], sc["cnt"], ids[off:off + Mx], ids, mode, eps, Ny, W_ROW,
                         W_COL, 1.0 / Ny)
        K = b if cache is None else torch.cat([b, cache])
        want = CA.simce_grad_cls(x.double(), b.double(), torch.tensor(scale, dtype=R.F64), st["lse"], sc["lse"],
                                 st["cnt"], sc["cnt"], W_ROW, W_COL, 1.0 / Ny, Ny, ids[off:off + Mx], ids, mode, eps, off,
                                 None if cache is None else cache.double())
        assert torch.allclose(got[0], want[0], rtol=1e-12, atol=1e-16)
        assert torch.allclose(got[1], want[1], rtol=1e-12, atol=1e-16)
        assert bool((st["b_tgt"] > 0).all()) and bool(torch.isfinite(st["b_tgt"]).all())


# ---------------------------------------------------------------------------------------------- f32 stand-in
def _dots_f32(x, K):
    """<x_i, K_j> as an f32 fma chain over p: the product of two f32 is exact in f64, the sum rounds once per step."""
    x, K = x.numpy().astype(np.float64), K.numpy().astype(np.float64)
    acc = np.zeros((x.shape[0], K.shape[0]), F32)
    for p in range(x.shape[1]):
        acc = (acc.astype(np.float64) + x[:, p, None] * K[None, :, p]).astype(F32)
    return acc


def _lse_f32(S, tps, fault=None):
    """The online-softmax merge over 64-key tiles, tps tiles per split, then the splits: f32 throughout."""
    Mx, Nk = S.shape
    ntiles = -(-Nk // 64)
    parts = []
    with np.errstate(invalid="ignore", over="ignore"):
        for t0 in range(0, ntiles, tps):
            m_run, l_run = np.full(Mx, -np.inf, F32), np.zeros(Mx, F32)
            for t in range(t0, min(t0 + tps, ntiles)):
                sv = np.full((Mx, 64), -np.inf, F32)
                n = min(64, Nk - 64 * t)
                sv[:, :n] = S[:, 64 * t:64 * t + n]
                if fault == "padding" and n < 64:
                    sv[:, n:] = S[:, Nk - 1:Nk]                                   # the clamped rows of the staging
                m_new = np.maximum(m_run, sv.max(1))
                acc = np.exp(sv - m_new[:, None], dtype=F32).sum(1, dtype=F32)
                resc = np.where(m_run > -np.inf, np.exp(m_run - m_new, dtype=F32), F32(0))
                l_run = (l_run if fault == "no-rescale" else l_run * resc) + acc
                m_run = m_new
            parts.append((m_run, l_run))
    if fault == "split-left-out":
        parts = parts[:3] + parts[4:]
    m = np.max([p[0] for p in parts], 0)
    l = np.zeros(Mx, F32)
    for ms, ls in parts:
        l = l + ls * np.exp(ms - m, dtype=F32)
    return (m + np.log(l, dtype=F32)).astype(F32)


_DOTS = {}


def _standin(Mx, Ny, Nc, off, a, b, cache, scale, tps, fault=None):
    """f32 lse, pos, dX, dscale rows of the row problem; the column LSE (its own keys: all of a) by the same code."""
    K = b if cache is None else torch.cat([b, cache])
    x = a[off:off + Mx]
    # the faults leave the dot products alone: one computation per input set
    memo = (Mx, off, tuple(a.shape), tuple(K.shape), a.double().sum().item(), K.double().sum().item(), scale)
    if memo not in _DOTS:
        _DOTS[memo] = (_dots_f32(x, K), _dots_f32(b, a))
    Dn, Dcol = _DOTS[memo]
    S = (F32(scale) * Dn).astype(F32)
    Sl = S.copy()
    if fault == "key-dropped":
        Sl[:, 7] = -np.inf
    lse = _lse_f32(Sl, tps, fault)
    label = off + np.arange(Mx) + (1 if fault == "label-shifted" else 0)
    pos = S[np.arange(Mx), label]
    lse_y = _lse_f32((F32(scale) * Dcol).astype(F32), tps)
    ibg = F32(1.0 / Ny)
    g = F32(W_ROW) * np.exp(S - lse[:, None], dtype=F32)
    if fault == "lse_y-by-query":
        col = np.exp(S[:, :Ny] - lse_y[off:off + Mx, None], dtype=F32)
    else:
        col = np.exp(S[:, :Ny] - lse_y[None, :], dtype=F32)
    g[:, :Ny] += F32(W_COL) * col
    if fault == "cache-column-term":
        g[:, Ny:] += F32(W_COL) * np.exp(S[:, Ny:] - lse_y[None, :Nc], dtype=F32)
    g[np.arange(Mx), off + np.arange(Mx)] -= F32(W_ROW + W_COL)
    g = (g * ibg).astype(F32)
    Kn = K.numpy()
    dX = (F32(scale) * np.einsum("ij,jp->ip", g, Kn, dtype=F32, optimize=False)).astype(F32)
    if fault == "rows-overlap":
        dX[1:, :20] = dX[:-1, :20].copy()
    dsc = (g * Dn).sum(1, dtype=F32)
    return dict(lse=lse, pos=pos, dX=dX, dscale=dsc, lse_y=lse_y)


def _ratios(case, got):
    """worst |error| / bound per quantity of a stand-in result against the reference formed from ITS f32 LSE vectors."""
    Mx, Ny, Nc, off, a, b, cache, scale, tps = case
    t = lambda v: torch.from_numpy(np.asarray(v))
    ref = R.simce_ref(a[off:off + Mx], b, cache, scale, off, t(got["lse"]), t(got["lse_y"]), W_ROW, W_COL, 1.0 / Ny)
    out = {}
    for k, bk in (("lse", "b_lse"), ("pos", "b_pos"), ("dX", "b_dX"), ("dscale", "b_dscale")):
        bound = ref[bk]
        if case[7] == R.SCALE_A:
            bound = R.cap_dx(bound, ref[k]) if k == "dX" else (R.cap_stat(bound) if k != "dscale" else bound)
        out[k] = ((t(got[k]).double() - ref[k]).abs() / bound).max().item()
    return out


_CASES = {}


def _cached(family):
    if family not in _CASES:
        case = _case(family)
        _CASES[family] = (case, _standin(*case))
    return _CASES[family]


@pytest.mark.parametrize("family", ["A", "B", "C"])
def test_f32_standin_is_inside_every_bound(family):
    case, got = _cached(family)
    r = _ratios(case, got)
    print(f"family {family}: worst |err| / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    assert all(v <= 1.0 for v in r.values()), r
    if family == "C":                                           # exact logits: pos equals the reference
        Mx, Ny, Nc, off, a, b, cache, scale, _ = case
        ref = R.simce_ref(a[off:off + Mx], b, cache, scale, off)
        assert np.array_equal(got["pos"].astype(np.float64), ref["pos"].numpy())


@pytest.mark.parametrize("shape,P", [("three-tile", 20), ("many-splits", 12), ("sweep", 132), ((65, 65, 1, 0), 4),
                                     ((1, 65, 0, 64), 4)])
@pytest.mark.parametrize("family", ["A", "B"])
def test_f32_standin_is_inside_every_bound_at_the_other_shapes(family, shape, P):
    case = _case(family, shape, P)
    r = _ratios(case, _standin(*case))
    assert all(v <= 1.0 for v in r.values()), r


FAULTS = {"key-dropped": "lse", "padding": "lse", "no-rescale": "lse", "split-left-out": "lse", "label-shifted": "pos",
          "lse_y-by-query": "dX", "cache-column-term": "dX", "rows-overlap": "dX"}


@pytest.mark.parametrize("fault", list(FAULTS))
@pytest.mark.parametrize("family", ["A", "B"])
def test_seeded_faults_fall_outside_the_bounds(family, fault):
    case, clean = _cached(family)
    bad = _standin(*case, fault=fault)
    if FAULTS[fault] == "dX":                                   # a gradient fault: judged with the clean LSE vectors
        bad["lse"], bad["lse_y"] = clean["lse"], clean["lse_y"]
    r = _ratios(case, bad)
    print(f"family {family} fault {fault}: {FAULTS[fault]} at {r[FAULTS[fault]]:.3g} x bound")
    assert r[FAULTS[fault]] > 1.0, (fault, r)


def test_combine_and_hard_tolerances():
    v, bnd = R.combine(torch.tensor([3.0, 5.0]), torch.tensor([1.0, 1.0]), torch.tensor([2.0, 2.0]), torch.tensor([0.0, 1.0]),
                       0.5, 0.25, 2.0)
    assert v.item() == (0.5 * 6 + 0.25 * 3) / 2 and 0 < bnd.item() < 1e-5
    L = R.Logits(R.unit_rows(8, 4, 1), R.unit_rows(8, 4, 2), None, R.SCALE_B)
    f = R.hard_factor(L)
    assert 1.0 <= f <= 100.0 / R.SCALE_A + 1e-9
    assert R.hard_tol(L, 0.5, "lse_h", torch.zeros(3))[0].item() == pytest.approx(2e-5 * 2 * f)
    assert R.hard_tol(L, 0.5, "q", torch.zeros(3))[0].item() == pytest.approx(2e-5 * 2 * f)
    assert R.hard_cap_dx(torch.ones(3), torch.ones(3), 0.5)[0].item() == pytest.approx(1.5e-6 + 1e-4)
