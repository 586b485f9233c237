"""GPU: the fused similarity + cross-entropy kernels (csrc/simce.hip, simce_tiled.hip, simce_hard.hip and simce_tile.h,
cloud_tile.h, key_sum_tile.h, sim_tile.h), branch by branch against the f64 yardstick of tests/simce_ref.py (itself
pinned on the CPU by tests/test_simce_ref_host.py, where its bounds are derived and shown to discriminate).

What the shapes reach (tests/simce_ref.py: SHAPES; every test asserts its plan numbers first, so a shape can never
silently miss its branch): two, three and one tile per key split on the tiled passes (5, 9 and 1 on the first-generation
pass), with the batch / cache boundary inside a split's second tile and a ragged last split; 67 and 133 key splits, so the
finalize kernels' lanes wrap; six batched problems of two tiles per split; every wave count and ragged slice of the
contraction width P on both generations; one-tile and one-row problems.  Families: A generic unit rows at scale 14.2849,
B peaked (scale 100, a bitwise copy of the query planted as a key so that the row's maximum arrives at every level of the
merge: simce_ref.plant_keys), C exact (entries of {-1, 0, 1} / 8 at scale 16: pos, sim_logits, cnt and the "mask" target
must EQUAL the reference).  Inputs come from seeded CPU generators; nothing is masked out or skipped.

Every comparison goes through _within, which records the worst |error| / bound per kernel and quantity; on family A the
bound is the smaller of the derived one and the project's existing bar (simce_ref.cap_stat / cap_dx).

Bit-for-bit promises pinned here, each stated in the code:
  * every entry is reproducible run to run (simce.hip:18-19 "merges in a fixed order: deterministic, no float atomics",
    simce_tiled.hip:13-14, simce_hard.hip:9) - at the two-tile and many-splits shapes;
  * upstream = 1 gives the bits of no upstream (simce.hip:106, simce_tiled.hip:198: ibg = inv_bg * upstream[0]);
  * class-aware with distinct ids and eps 0 gives the plain tiled LSE bits (simce.hip:286-288 "the same arithmetic, so the
    same bits"; simce_tiled.hip:20 "CLS = false is the plain kernel").

Worst |error| / bound of one run on an MI355X (the table the module prints at its end; "first" / "tiled": the
generation that computed the quantity, "batched": the six-problem launches):
                     lse     pos     tgt     q       k1      k2      dX      dscale
  first plain        0.3271  0.2760                                  0.3830  0.0812
  tiled plain        0.3271  0.2760                                  0.6980  0.1841
  tiled cls          0.3449          0.1758                          0.6172  0.1889
  tiled hard         0.1646  0.2760          0.0253  0.2422  0.1732  0.2229  0.2006
  batched plain      0.1023  0.0985                                  0.0960  0.0794
  batched cls        0.0923          0.0754                          0.1031  0.0897
  batched hard       0.2554  0.0757          0.0134  0.4058  0.2561  0.0823  0.0807
  sim_logits S 0.4034, ce_combine loss 0.3674.
(The hard-negative lse_h, q, k1 and k2 are held to the tolerance of tests/test_gpu_hard_negative_loss.py scaled by the
logit range, an assumption; everything else to derived bounds, with C_EXP = C_LOG = 2 assumed: tests/simce_ref.py.)
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simce_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

W_ROW, W_COL, BETA = 0.5, 0.5, 0.5
RATIOS = {}                             # kernel and quantity -> worst |error| / bound seen in this run
UNSUPPORTED, BAD_ARG = r"(?i)unsupported", r"\(status -1\)"


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    print("\nworst |error| / bound per kernel and quantity:")
    for k, v in sorted(RATIOS.items()):
        print(f"  {k:34s} {v:.4f}")


def _within(got, ref, bound, key, what=""):
    """|got - ref| <= bound per element; records the worst ratio under `key`."""
    got = torch.as_tensor(got).detach().cpu().to(R.F64).reshape(ref.shape)
    bound = torch.as_tensor(bound, dtype=R.F64).expand_as(ref)
    assert bool(torch.isfinite(got).all()), f"{key} {what}: non-finite output"
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), err)).max().item()
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
    assert ratio <= 1.0, f"{key} {what}: worst |err| / bound = {ratio:.3f} (max |err| {err.max().item():.3e})"


def _exact(got, ref, key, what=""):
    assert torch.equal(got.detach().cpu().to(R.F64).reshape(ref.shape), ref), f"{key} {what}: not exact"


class Problem:
    """One pair batch on the CPU (f32 inputs, f64 logits of the row and the column problem) and on the device."""
    _cache = {}

    def __init__(self, family, shape, P, dev):
        self.family, self.P = family, P
        self.Mx, self.Ny, self.Nc, self.off = shape
        self.tps = R.tiled_plan(self.Mx, self.Ny + self.Nc)[2]
        a, b, cache, self.scale = R.pair_batch(family, self.Mx, self.Ny, self.Nc, self.off, P, 100 + P, self.tps)
        self.rows = slice(self.off, self.off + self.Mx)
        self.L = R.Logits(a[self.rows], b, cache, self.scale)              # rows of a over [b | cache]
        self.Lc = R.Logits(b, a, None, self.scale)                          # every batch key's own direction
        self.a, self.b = a.to(dev), b.to(dev)
        self.x = self.a[self.rows].contiguous()
        self.cache = None if cache is None else cache.to(dev)
        self.sc = torch.tensor([self.scale], device=dev)
        self.square = self.off + self.Mx <= self.Ny                         # every row has its diagonal key
        # the gradient's 1 / (global batch).  The project's bars on dX (rtol 1e-4, atol 1e-7) were set at batches of 32
        # pairs and more, and dX is linear in this factor: a tiny shape keeps 1 / 32
        self.inv_bg = 1.0 / max(self.Ny, 32)

    @classmethod
    def get(cls, family, shape, P, dev):
        shape = R.SHAPES[shape] if isinstance(shape, str) else shape
        key = (family, shape, P)
        if key not in cls._cache:
            if len(cls._cache) >= 4:                                        # the f64 logits of a few problems at most
                cls._cache.pop(next(iter(cls._cache)))
            cls._cache[key] = cls(family, shape, P, dev)
        return cls._cache[key]

    def stat_bound(self, b):
        return R.cap_stat(b) if self.family == "A" else b

    def dx_bound(self, b, ref):
        return R.cap_dx(b, ref) if self.family == "A" else b

    def ids(self, pattern, dev):
        ids = R.class_ids(pattern, self.Ny, seed=3)
        return ids, (None if ids is None else ids.to(dev)), (None if ids is None else ids[self.rows].contiguous()), \
            (None if ids is None else ids[self.rows].contiguous().to(dev))


def _ops():
    from clip_dplm_amd import ops
    return ops


def _split_count(entry, Mx, Nk, P, floats_per_row):
    """The key-split count behind a workspace size that determines it: bytes / (4 Mx floats_per_row)."""
    n = getattr(_ops()._lib(), entry)(Mx, Nk, P)
    assert n % (4 * Mx * floats_per_row) == 0
    return n // (4 * Mx * floats_per_row)


# ---------------------------------------------------------------------------------------------- the checks
def check_plain(p, kernel, what, repro=False):
    """simce_lse both directions, simce_grad without / with upstream and ce_combine of one problem under simce_kernel =
    kernel; the ratios go under the generation that computes each quantity at this shape."""
    ops = _ops()
    off, Ny = p.off, p.Ny
    key = ("tiled" if R.lse_takes_tiled(p.Mx, p.Ny + p.Nc, kernel) else "first") + " plain"
    gkey = ("tiled" if R.grad_takes_tiled(p.Mx, p.Ny + p.Nc, p.P, kernel) else "first") + " plain"
    lse, pos = ops.simce_lse(p.x, p.b, p.sc, label_offset=off, cache=p.cache)
    lse_y, pos_y = ops.simce_lse(p.b, p.a, p.sc)
    r_lse, r_pos, b_lse, b_pos = R.plain_stats(p.L, off)
    c_lse, c_pos, cb_lse, cb_pos = R.plain_stats(p.Lc, 0)
    _within(lse, r_lse, p.stat_bound(b_lse), f"{key} lse", what)
    _within(pos, r_pos, p.stat_bound(b_pos), f"{key} pos", what)
    ckey = ("tiled" if R.lse_takes_tiled(p.Ny, p.a.shape[0], kernel) else "first") + " plain"
    _within(lse_y, c_lse, p.stat_bound(cb_lse), f"{ckey} lse", what + " columns")
    _within(pos_y, c_pos, p.stat_bound(cb_pos), f"{ckey} pos", what + " columns")
    if p.family == "C":
        _exact(pos, r_pos, f"{key} pos", what)
        _exact(pos_y, c_pos, f"{key} pos", what + " columns")
    args = (p.x, p.b, p.sc, lse, lse_y, W_ROW, W_COL, p.inv_bg)
    kw = dict(label_offset=off, cache=p.cache)
    dX, dsc = ops.simce_grad(*args, **kw)
    r_dX, r_dsc, b_dX, b_dsc = R.plain_grad(p.L, off, lse, lse_y, W_ROW, W_COL, p.inv_bg)
    _within(dX, r_dX, p.dx_bound(b_dX, r_dX), f"{gkey} dX", what)
    _within(dsc, r_dsc, b_dsc, f"{gkey} dscale", what)
    one, up = torch.ones(1, device=dX.device), torch.tensor([-1.75], device=dX.device)
    d1, s1 = ops.simce_grad(*args, upstream=one, **kw)
    assert torch.equal(d1, dX) and torch.equal(s1, dsc), f"{key} {what}: upstream = 1 changes bits"
    du, su = ops.simce_grad(*args, upstream=up, **kw)
    r_dX, r_dsc, b_dX, b_dsc = R.plain_grad(p.L, off, lse, lse_y, W_ROW, W_COL, p.inv_bg, upstream=-1.75)
    _within(du, r_dX, p.dx_bound(b_dX, r_dX), f"{gkey} dX", what + " upstream")
    _within(su, r_dsc, b_dsc, f"{gkey} dscale", what + " upstream")
    if p.square:
        cols = (lse_y[p.rows].contiguous(), pos_y[p.rows].contiguous())
    else:
        cols = (None, None)
    loss = ops.ce_combine(lse, pos, *cols, W_ROW, W_COL, Ny)
    r_loss, b_loss = R.combine(lse, pos, *cols, W_ROW, W_COL, Ny)
    _within(loss, r_loss, b_loss, "ce_combine loss", what)
    if repro:
        assert torch.equal(ops.ce_combine(lse, pos, *cols, W_ROW, W_COL, Ny), loss), f"{what}: ce_combine not reproducible"
        again = ops.simce_lse(p.x, p.b, p.sc, label_offset=off, cache=p.cache) + ops.simce_grad(*args, **kw)
        for u, v in zip(again, (lse, pos, dX, dsc)):
            assert torch.equal(u, v), f"{key} {what}: not reproducible"
    return lse


def check_logits(p, what):
    S = _ops().sim_logits(p.x, p.b, p.sc)
    ref = p.L.S[:, :p.Ny]
    _within(S, ref, p.L.bS[:, :p.Ny], "sim_logits S", what)
    if p.family == "C":
        _exact(S, ref, "sim_logits S", what)
    assert torch.equal(_ops().sim_logits(p.x, p.b, p.sc), S), f"{what}: sim_logits not reproducible"


def check_cls(p, mode, eps, pattern, what, dev, repro=False, plain_lse=None):
    ops = _ops()
    off, Ny = p.off, p.Ny
    ids, ids_d, cx, cx_d = p.ids(pattern, dev)
    key = "tiled cls"
    kw = dict(cls_x=cx_d, cls_y=ids_d, same_class=mode, eps=eps, label_offset=off, cache=p.cache)
    lse, tgt, cnt = ops.simce_lse_cls(p.x, p.b, p.sc, **kw)
    lse_y, tgt_y, cnt_y = ops.simce_lse_cls(p.b, p.a, p.sc, cls_x=ids_d, cls_y=ids_d, same_class=mode, eps=eps)
    for got, L, o, c, side in (((lse, tgt, cnt), p.L, off, cx, ""), ((lse_y, tgt_y, cnt_y), p.Lc, 0, ids, " columns")):
        st = R.cls_stats(L, o, c, ids, mode, eps)
        _within(got[0], st["lse"], p.stat_bound(st["b_lse"]), f"{key} lse", what + side)
        _within(got[1], st["tgt"], p.stat_bound(st["b_tgt"]), f"{key} tgt", what + side)
        _exact(got[2], st["cnt"], f"{key} cnt", what + side)
        if p.family == "C" and mode == "mask" and eps == 0.0:
            _exact(got[1], st["tgt"], f"{key} tgt", what + side)
    if plain_lse is not None:
        assert torch.equal(lse, plain_lse), f"{what}: distinct ids, eps 0 is not the plain tiled LSE bit for bit"
    args = (p.x, p.b, p.sc, lse, lse_y, cnt, cnt_y, W_ROW, W_COL, p.inv_bg, Ny)
    dX, dsc = ops.simce_grad_cls(*args, **kw)
    ref = R.cls_grad(p.L, off, lse, lse_y, cnt, cnt_y, cx, ids, mode, eps, Ny, W_ROW, W_COL, p.inv_bg)
    _within(dX, ref[0], p.dx_bound(ref[2], ref[0]), f"{key} dX", what)
    _within(dsc, ref[1], ref[3], f"{key} dscale", what)
    d1, s1 = ops.simce_grad_cls(*args, upstream=torch.ones(1, device=dev), **kw)
    assert torch.equal(d1, dX) and torch.equal(s1, dsc), f"{key} {what}: upstream = 1 changes bits"
    du, su = ops.simce_grad_cls(*args, upstream=torch.tensor([-1.75], device=dev), **kw)
    ref = R.cls_grad(p.L, off, lse, lse_y, cnt, cnt_y, cx, ids, mode, eps, Ny, W_ROW, W_COL, p.inv_bg, upstream=-1.75)
    _within(du, ref[0], p.dx_bound(ref[2], ref[0]), f"{key} dX", what + " upstream")
    _within(su, ref[1], ref[3], f"{key} dscale", what + " upstream")
    if repro:
        again = ops.simce_lse_cls(p.x, p.b, p.sc, **kw) + ops.simce_grad_cls(*args, **kw)
        for u, v in zip(again, (lse, tgt, cnt, dX, dsc)):
            assert torch.equal(u, v), f"{key} {what}: not reproducible"


def check_coef(got, ref, L, key, what):
    """The three rows simce_lse_hard leaves for the gradient pass, q, k1, k2, against the f64 coefficients: the -inf
    pattern (rows without negatives; k2 at beta = 0) exactly, the finite entries within simce_ref.hard_tol."""
    got = got.detach().cpu().to(R.F64)
    assert not bool(torch.isnan(got).any()), f"{key} {what}: NaN coefficient"
    for n, name in enumerate(("q", "k1", "k2")):
        fin = torch.isfinite(ref[n])
        assert torch.equal(torch.isneginf(got[n]), torch.isneginf(ref[n])) and bool(torch.isfinite(got[n][fin]).all()), \
            f"{key} {name} {what}: -inf pattern"
        if bool(fin.any()):
            _within(got[n][fin], ref[n][fin], R.hard_tol(L, BETA, name, ref[n][fin]), f"{key} {name}", what)


def check_hard(p, pattern, what, dev, repro=False):
    ops = _ops()
    off, Ny = p.off, p.Ny
    ids, ids_d, cx, cx_d = p.ids(pattern, dev)
    key = "tiled hard"
    kw = dict(cls_x=cx_d, cls_y=ids_d, label_offset=off, cache=p.cache)
    lse, pos, coef = ops.simce_lse_hard(p.x, p.b, p.sc, BETA, **kw)
    lse_y, pos_y, coef_y = ops.simce_lse_hard(p.b, p.a, p.sc, BETA, cls_x=ids_d, cls_y=ids_d)
    for got, L, o, c, side in (((lse, pos, coef), p.L, off, cx, ""), ((lse_y, pos_y, coef_y), p.Lc, 0, ids, " columns")):
        st = R.hard_stats(L, o, c, ids, BETA)
        _within(got[0], st["lse_h"], R.hard_tol(L, BETA, "lse_h", st["lse_h"]), f"{key} lse_h", what + side)
        _within(got[1], st["pos"], p.stat_bound(st["b_pos"]), f"{key} pos", what + side)
        check_coef(got[2], st["coef"], L, key, what + side)
        if p.family == "C":
            _exact(got[1], st["pos"], f"{key} pos", what + side)
    args = (p.x, p.b, p.sc, BETA, coef, coef_y, W_ROW, W_COL, p.inv_bg)
    dX, dsc = ops.simce_grad_hard(*args, **kw)
    hard_dx = (lambda b, r: R.hard_cap_dx(b, r, BETA)) if p.family == "A" else (lambda b, r: b)
    r_dX, r_dsc, b_dX, b_dsc = R.hard_grad(p.L, off, coef, coef_y, cx, ids, BETA, W_ROW, W_COL, p.inv_bg)
    _within(dX, r_dX, hard_dx(b_dX, r_dX), f"{key} dX", what)
    _within(dsc, r_dsc, b_dsc, f"{key} dscale", what)
    d1, s1 = ops.simce_grad_hard(*args, upstream=torch.ones(1, device=dev), **kw)
    assert torch.equal(d1, dX) and torch.equal(s1, dsc), f"{key} {what}: upstream = 1 changes bits"
    du, su = ops.simce_grad_hard(*args, upstream=torch.tensor([-1.75], device=dev), **kw)
    r_dX, r_dsc, b_dX, b_dsc = R.hard_grad(p.L, off, coef, coef_y, cx, ids, BETA, W_ROW, W_COL, p.inv_bg, upstream=-1.75)
    _within(du, r_dX, hard_dx(b_dX, r_dX), f"{key} dX", what + " upstream")
    _within(su, r_dsc, b_dsc, f"{key} dscale", what + " upstream")
    if repro:
        again = ops.simce_lse_hard(p.x, p.b, p.sc, BETA, **kw) + ops.simce_grad_hard(*args, **kw)
        for u, v in zip(again, (lse, pos, coef, dX, dsc)):
            assert torch.equal(u, v), f"{key} {what}: not reproducible"


# ---------------------------------------------------------------------------------------------- single problems
PLAIN_CASES = [("two-tile", 36, "A"), ("two-tile", 36, "B"), ("two-tile", 36, "C"), ("two-tile", 32, "A"),
               ("two-tile", 32, "B"), ("three-tile", 20, "A"), ("three-tile", 20, "B"), ("many-splits", 12, "A"),
               ("many-splits", 12, "B"), ("many-splits", 32, "A"), ("many-splits", 32, "B")]
TILED_PLAN = {"two-tile": (24, 25, 2, 13), "three-tile": (32, 33, 3, 11), "many-splits": (2, 67, 1, 67)}
FIRST_PLAN = {"two-tile": (47, 50, 5, 10), "three-tile": (64, 66, 9, 8), "many-splits": (3, 133, 1, 133)}
_id = lambda c: "-".join(map(str, c))


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("case", PLAIN_CASES, ids=_id)
def test_plain_multi_tile(dev, kopt, case, kernel):
    shape, P, fam = case
    Mx, Ny, Nc, off = R.SHAPES[shape]
    assert R.tiled_plan(Mx, Ny + Nc) == TILED_PLAN[shape] and R.first_gen_plan(Mx, Ny + Nc, P)[:4] == FIRST_PLAN[shape]
    assert R.lse_takes_tiled(Mx, Ny + Nc, kernel) == (kernel == 2)
    assert R.grad_takes_tiled(Mx, Ny + Nc, P, kernel) == (kernel == 2 or P != 32)      # P = 32: the first pass itself
    kopt("simce_kernel", kernel)
    p = Problem.get(fam, shape, P, dev)
    check_plain(p, kernel, f"{_id(case)} k{kernel}", repro=shape != "three-tile")
    if kernel == 1:                     # clipk_sim_logits does not read the option (simce.hip: one launch<MODE_LOGITS>)
        check_logits(p, _id(case))


CLS_CASES = [("two-tile", 36, "A", "mask", 0.1, "random"), ("two-tile", 36, "A", "positive", 0.0, None),
             ("two-tile", 36, "B", "mask", 0.0, "runs"), ("two-tile", 36, "B", "positive", 0.1, "runs"),
             ("two-tile", 36, "C", "mask", 0.0, "random"), ("three-tile", 20, "A", "positive", 0.1, "random"),
             ("three-tile", 20, "B", "mask", 0.0, "runs"), ("many-splits", 12, "A", "mask", 0.0, "random"),
             ("many-splits", 12, "B", "positive", 0.1, "runs"), ("many-splits", 32, "B", "mask", 0.1, "runs")]


@pytest.mark.parametrize("case", CLS_CASES, ids=_id)
def test_class_aware_multi_tile(dev, case):
    shape, P, fam, mode, eps, pattern = case
    Mx, Ny, Nc, off = R.SHAPES[shape]
    assert R.tiled_plan(Mx, Ny + Nc) == TILED_PLAN[shape]
    assert _split_count("clipk_simce_cls_workspace", Mx, Ny + Nc, P, P + 1) == TILED_PLAN[shape][3]
    check_cls(Problem.get(fam, shape, P, dev), mode, eps, pattern, _id(case), dev, repro=shape != "three-tile")


HARD_CASES = [("two-tile", 36, "A", "random"), ("two-tile", 36, "B", "runs"), ("two-tile", 36, "B", None),
              ("two-tile", 36, "C", "random"), ("three-tile", 20, "A", None), ("three-tile", 20, "B", "runs"),
              ("many-splits", 12, "A", "random"), ("many-splits", 12, "B", "runs")]


@pytest.mark.parametrize("case", HARD_CASES, ids=_id)
def test_hard_negative_multi_tile(dev, case):
    shape, P, fam, pattern = case
    Mx, Ny, Nc, off = R.SHAPES[shape]
    assert R.tiled_plan(Mx, Ny + Nc) == TILED_PLAN[shape]
    assert _split_count("clipk_simce_hard_workspace", Mx, Ny + Nc, P, P + 1) == TILED_PLAN[shape][3]
    check_hard(Problem.get(fam, shape, P, dev), pattern, _id(case), dev, repro=shape != "three-tile")


@pytest.mark.parametrize("fam", ["A", "B"])
def test_distinct_ids_without_smoothing_are_the_plain_tiled_bits(dev, kopt, fam):
    kopt("simce_kernel", 2)
    for shape, P in (("two-tile", 36), ("many-splits", 12)):
        p = Problem.get(fam, shape, P, dev)
        plain = _ops().simce_lse(p.x, p.b, p.sc, label_offset=p.off, cache=p.cache)[0]
        check_cls(p, "mask", 0.0, "distinct", f"{shape} {fam} distinct", dev, plain_lse=plain)


# ---------------------------------------------------------------------------------------------- the P sweep
SWEEP = sorted(set(R.SWEEP_P_TILED + R.SWEEP_P_FIRST_LSE + R.SWEEP_P_FIRST_GRAD))


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("P", SWEEP)
def test_plain_p_sweep(dev, kopt, P, kernel):
    """Every wave count and ragged slice of P: NW = 1, 2, 4, 8 waves of the first pass (P = 132, 260, 516, 956 leave
    the last wave a ragged slice), 1 .. 4 p-tiles per wave of the tiled gradient (ragged at 132, 260, 388, 508).  With
    simce_kernel = 1 the gradient at a slice that is no multiple of 32 is rerouted to the tiled pass (P <= 512) or
    refused (above)."""
    Mx, Ny, Nc, off = R.SHAPES["sweep"]
    plan = R.first_gen_plan(Mx, Ny + Nc, P)
    assert plan is not None and plan[4] == min(8, 1 << max(0, (P - 1) // 128).bit_length())
    kopt("simce_kernel", kernel)
    ops = _ops()
    tiled_grad = R.grad_takes_tiled(Mx, Ny + Nc, P, kernel)
    for fam in ("A", "B"):
        p = Problem.get(fam, "sweep", P, dev)
        what = f"sweep P={P} {fam} k{kernel}"
        if tiled_grad or plan[5] % 32 == 0:
            check_plain(p, kernel, what)
        else:                                           # P > 512 with a ragged slice: LSE runs, the gradient refuses
            lse, pos = ops.simce_lse(p.x, p.b, p.sc, label_offset=off, cache=p.cache)
            r_lse, r_pos, b_lse, b_pos = R.plain_stats(p.L, off)
            key = "tiled plain" if kernel == 2 else "first plain"
            _within(lse, r_lse, p.stat_bound(b_lse), f"{key} lse", what)
            _within(pos, r_pos, p.stat_bound(b_pos), f"{key} pos", what)
            with pytest.raises(ops._ffi.ClipkError, match=r"\(status -2\)"):
                ops.simce_grad(p.x, p.b, p.sc, lse, lse, W_ROW, W_COL, 1.0 / Ny, label_offset=off, cache=p.cache)
        if kernel == 1:                 # (sim_logits: one kernel whatever the option, as above)
            check_logits(p, what)


@pytest.mark.parametrize("P", R.SWEEP_P_TILED)
def test_variants_p_sweep(dev, P):
    p = Problem.get("A", "sweep", P, dev)
    check_cls(p, "mask", 0.1, "random", f"sweep P={P}", dev)
    check_hard(p, "random", f"sweep P={P}", dev)
    p = Problem.get("B", "sweep", P, dev)
    check_cls(p, "positive", 0.0, "random", f"sweep P={P} B", dev)
    check_hard(p, None, f"sweep P={P} B", dev)


# ---------------------------------------------------------------------------------------------- tiny shapes
@pytest.mark.parametrize("fam", ["A", "B", "C"])
@pytest.mark.parametrize("shape", R.TINY, ids=_id)
def test_tiny(dev, kopt, shape, fam):
    Mx, Ny, Nc, off = shape
    assert R.tiled_plan(Mx, Ny + Nc)[2:] == (1, R.tiled_plan(Mx, Ny + Nc)[1]) and R.tiled_plan(Mx, Ny + Nc)[1] <= 2
    p = Problem.get(fam, shape, 4, dev)
    what = f"tiny {_id(shape)} {fam}"
    for kernel in (1, 2):
        kopt("simce_kernel", kernel)
        check_plain(p, kernel, what + f" k{kernel}")
    check_logits(p, what)
    if p.square:
        check_cls(p, "mask", 0.1, "random", what, dev)
        check_cls(p, "positive", 0.0, "random", what, dev)
        check_hard(p, "random", what, dev)
    else:                                                       # a row without its diagonal key: refused
        ops = _ops()
        z = torch.zeros(Mx, device=dev)
        with pytest.raises(ops._ffi.ClipkError, match=BAD_ARG):
            ops.simce_lse_cls(p.x, p.b, p.sc)
        with pytest.raises(ops._ffi.ClipkError, match=BAD_ARG):
            ops.simce_lse_hard(p.x, p.b, p.sc, BETA)
        with pytest.raises(ops._ffi.ClipkError, match=BAD_ARG):
            ops.simce_grad_cls(p.x, p.b, p.sc, z, z[:Ny], z + 1, z[:Ny] + 1, W_ROW, W_COL, 1.0, Ny)
        with pytest.raises(ops._ffi.ClipkError, match=BAD_ARG):
            ops.simce_grad_hard(p.x, p.b, p.sc, BETA, torch.zeros(3, Mx, device=dev), torch.zeros(3, Ny, device=dev), W_ROW,
                                W_COL, 1.0)


# ---------------------------------------------------------------------------------------------- batched problems
def _tri_batch(fam, B, P, tps):
    """E [3, B, P] and the scale; B: copies of modality 0's rows planted in modality 1 and 2, of modality 1's in 2."""
    if fam == "C":
        return torch.stack([R.eighths(B, P, 300 + m) for m in range(3)]), R.SCALE_C
    E = torch.stack([R.unit_rows(B, P, 200 + m) for m in range(3)])
    if fam == "A":
        return E, R.SCALE_A
    for r, j in R.plant_keys(B, B, 0, 0, tps):
        E[1, j] = E[0, r]
        E[2, (j + 64) % B] = E[0, r]
    for r, j in R.plant_keys(B, B, 0, 0, tps)[1::2]:
        E[2, (j + 131) % B] = E[1, r]
    return E, R.SCALE_B


def _tri_ids(dev, B, fam):
    """Per problem (both directions of a pair share the tensor): runs of 300, random, none."""
    cp, ce = R.class_ids("runs", B), R.class_ids("random", B, seed=5)
    cpu = (cp, cp, ce, ce, None, None)
    d = {id(t): t.to(dev) for t in (cp, ce)}
    return cpu, tuple(None if t is None else d[id(t)] for t in cpu)


UPSTREAM = (1.0, 1.0, -0.5, -0.5, 2.25, 2.25)      # per problem; a pair's two directions belong to one loss


@pytest.mark.parametrize("fam", ["A", "B"])
@pytest.mark.parametrize("P", R.BATCHED_P)
def test_batched_variants_two_tiles_per_split(dev, P, fam):
    ops = _ops()
    B = R.BATCHED_B
    nqb, ntiles, tps, ks = R.tiled_plan(B, B, 6)
    assert (nqb, ntiles, tps, ks) == (10, 10, 2, 5)
    lib = ops._lib()
    assert lib.clipk_simce_pairs_cls_workspace(6, B, P) == 6 * ks * B * (P + 1) * 4
    assert lib.clipk_simce_pairs_hard_workspace(6, B, P) == 6 * ks * B * (P + 1) * 4
    E, scale = _tri_batch(fam, B, P, tps)
    Ls = [R.Logits(E[a], E[b], None, scale) for a, b in R.TRI_PAIRS]
    rev = [R.TRI_PAIRS.index((b, a)) for a, b in R.TRI_PAIRS]
    Ed, sc = E.to(dev), torch.tensor([scale], device=dev)
    ids, ids_d = _tri_ids(dev, B, fam)
    up = torch.tensor(UPSTREAM, device=dev)
    cap_s = (lambda b: R.cap_stat(b)) if fam == "A" else (lambda b: b)
    cap_d = (lambda b, r: R.cap_dx(b, r)) if fam == "A" else (lambda b, r: b)
    what = f"batched P={P} {fam}"
    for mode, eps in (("mask", 0.1), ("positive", 0.0)):
        run = lambda: ops.simce_lse_pairs_cls(Ed, R.TRI_PAIRS, sc, ids=ids_d, same_class=mode, eps=eps)
        lse, tgt, cnt = run()
        grad = lambda u: ops.simce_grad_pairs_cls(Ed, R.TRI_PAIRS, sc, lse, cnt, W_ROW, W_COL, 1.0 / B, ids=ids_d,
                                                  same_class=mode, eps=eps, upstream=u)
        dX, dsc = grad(up)
        for z, L in enumerate(Ls):
            st = R.cls_stats(L, 0, ids[z], ids[z], mode, eps)
            _within(lse[z], st["lse"], cap_s(st["b_lse"]), "batched cls lse", what)
            _within(tgt[z], st["tgt"], cap_s(st["b_tgt"]), "batched cls tgt", what)
            _exact(cnt[z], st["cnt"], "batched cls cnt", what)
            ref = R.cls_grad(L, 0, lse[z], lse[rev[z]], cnt[z], cnt[rev[z]], ids[z], ids[z], mode, eps, B, W_ROW, W_COL,
                             1.0 / B, upstream=UPSTREAM[z])
            _within(dX[z], ref[0], cap_d(ref[2], ref[0]), "batched cls dX", what)
            _within(dsc[z], ref[1], ref[3], "batched cls dscale", what)
        for u, v in zip(run() + grad(up), (lse, tgt, cnt, dX, dsc)):
            assert torch.equal(u, v), f"{what}: not reproducible"
        d1, s1 = grad(torch.ones(6, device=dev))
        d0, s0 = grad(None)
        assert torch.equal(d1, d0) and torch.equal(s1, s0), f"{what}: upstream = 1 changes bits"
    lse, pos, coef = ops.simce_lse_pairs_hard(Ed, R.TRI_PAIRS, sc, BETA, ids=ids_d)
    dX, dsc = ops.simce_grad_pairs_hard(Ed, R.TRI_PAIRS, sc, BETA, coef, W_ROW, W_COL, 1.0 / B, ids=ids_d, upstream=up)
    for z, L in enumerate(Ls):
        st = R.hard_stats(L, 0, ids[z], ids[z], BETA)
        _within(lse[z], st["lse_h"], R.hard_tol(L, BETA, "lse_h", st["lse_h"]), "batched hard lse_h", what)
        _within(pos[z], st["pos"], cap_s(st["b_pos"]), "batched hard pos", what)
        check_coef(coef[z], st["coef"], L, "batched hard", what)
        r_dX, r_dsc, b_dX, b_dsc = R.hard_grad(L, 0, coef[z], coef[rev[z]], ids[z], ids[z], BETA, W_ROW, W_COL, 1.0 / B,
                                               upstream=UPSTREAM[z])
        _within(dX[z], r_dX, R.hard_cap_dx(b_dX, r_dX, BETA) if fam == "A" else b_dX, "batched hard dX", what)
        _within(dsc[z], r_dsc, b_dsc, "batched hard dscale", what)
    hgrad = lambda u: ops.simce_grad_pairs_hard(Ed, R.TRI_PAIRS, sc, BETA, coef, W_ROW, W_COL, 1.0 / B, ids=ids_d,
                                                upstream=u)
    for u, v in zip(ops.simce_lse_pairs_hard(Ed, R.TRI_PAIRS, sc, BETA, ids=ids_d) + hgrad(up), (lse, pos, coef, dX, dsc)):
        assert torch.equal(u, v), f"{what}: not reproducible"
    d1, s1 = hgrad(torch.ones(6, device=dev))
    d0, s0 = hgrad(None)
    assert torch.equal(d1, d0) and torch.equal(s1, s0), f"{what}: upstream = 1 changes bits"


@pytest.mark.parametrize("fam", ["A", "B"])
def test_batched_plain_two_tiles_per_split(dev, fam):
    """clipk_simce_{lse,grad}_pairs: the first-generation kernel with a problem index, 25 tiles in 13 splits."""
    ops = _ops()
    B, P = R.BATCHED_PLAIN_B, R.BATCHED_PLAIN_P
    plan = R.first_gen_plan(B, B, P)
    assert plan[:4] == (25, 25, 2, 13) and plan[5] % 32 == 0
    assert ops._lib().clipk_simce_pairs_workspace(6, B, P) == 6 * plan[3] * B * (P + 2) * 4
    E, scale = _tri_batch(fam, B, P, 2)
    Ed, sc = E.to(dev), torch.tensor([scale], device=dev)
    rev = [R.TRI_PAIRS.index((b, a)) for a, b in R.TRI_PAIRS]
    lse, pos = ops.simce_lse_pairs(Ed, R.TRI_PAIRS, sc)
    dX, dsc = ops.simce_grad_pairs(Ed, R.TRI_PAIRS, sc, lse, W_ROW, W_COL, 1.0 / B)
    what = f"batched plain {fam}"
    for z, (a, b) in enumerate(R.TRI_PAIRS):
        L = R.Logits(E[a], E[b], None, scale)
        r_lse, r_pos, b_lse, b_pos = R.plain_stats(L, 0)
        ref = R.plain_grad(L, 0, lse[z], lse[rev[z]], W_ROW, W_COL, 1.0 / B)
        cap = fam == "A"
        _within(lse[z], r_lse, R.cap_stat(b_lse) if cap else b_lse, "batched plain lse", what)
        _within(pos[z], r_pos, R.cap_stat(b_pos) if cap else b_pos, "batched plain pos", what)
        _within(dX[z], ref[0], R.cap_dx(ref[2], ref[0]) if cap else ref[2], "batched plain dX", what)
        _within(dsc[z], ref[1], ref[3], "batched plain dscale", what)
    again = ops.simce_lse_pairs(Ed, R.TRI_PAIRS, sc) + ops.simce_grad_pairs(Ed, R.TRI_PAIRS, sc, lse, W_ROW, W_COL, 1.0 / B)
    for u, v in zip(again, (lse, pos, dX, dsc)):
        assert torch.equal(u, v), f"{what}: not reproducible"


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(dev):
    ops = _ops()
    Err = ops._ffi.ClipkError
    sc = torch.tensor([R.SCALE_A], device=dev)
    for P in (6, 1028):
        x, y = torch.zeros(8, P, device=dev), torch.zeros(8, P, device=dev)
        v, c3 = torch.zeros(8, device=dev), torch.zeros(3, 8, device=dev)
        E = torch.zeros(3, 8, P, device=dev)
        for call in (lambda: ops.simce_lse(x, y, sc), lambda: ops.simce_grad(x, y, sc, v, v, 0.5, 0.5, 1.0),
                     lambda: ops.sim_logits(x, y, sc), lambda: ops.simce_lse_cls(x, y, sc),
                     lambda: ops.simce_grad_cls(x, y, sc, v, v, v + 1, v + 1, 0.5, 0.5, 1.0, 8),
                     lambda: ops.simce_lse_hard(x, y, sc, BETA),
                     lambda: ops.simce_grad_hard(x, y, sc, BETA, c3, c3, 0.5, 0.5, 1.0),
                     lambda: ops.simce_lse_pairs(E, R.TRI_PAIRS, sc)):
            with pytest.raises(Err, match=UNSUPPORTED):
                call()
        v6, c6 = torch.zeros(6, 8, device=dev), torch.zeros(6, 3, 8, device=dev)
        with pytest.raises(Err, match=r"\(status -2\)"):
            ops.simce_grad_pairs(E, R.TRI_PAIRS, sc, v6, 0.5, 0.5, 1.0)
        # the batched variants' wrappers check P before the library is asked
        for call in (lambda: ops.simce_lse_pairs_cls(E, R.TRI_PAIRS, sc),
                     lambda: ops.simce_lse_pairs_hard(E, R.TRI_PAIRS, sc, BETA),
                     lambda: ops.simce_grad_pairs_cls(E, R.TRI_PAIRS, sc, v6, v6 + 1, 0.5, 0.5, 1.0),
                     lambda: ops.simce_grad_pairs_hard(E, R.TRI_PAIRS, sc, BETA, c6, 0.5, 0.5, 1.0)):
            with pytest.raises(ValueError, match="P <= 512"):
                call()
    for P in (516, 640):                                        # above 512 a ragged slice has no gradient pass
        x, v = torch.zeros(8, P, device=dev), torch.zeros(8, device=dev)
        ops.simce_lse(x, x, sc)
        with pytest.raises(Err, match=r"\(status -2\)"):
            ops.simce_grad(x, x, sc, v, v, 0.5, 0.5, 1.0)
    x, v, c3 = torch.zeros(8, 516, device=dev), torch.zeros(8, device=dev), torch.zeros(3, 8, device=dev)
    for call in (lambda: ops.simce_lse_cls(x, x, sc),
                 lambda: ops.simce_grad_cls(x, x, sc, v, v, v + 1, v + 1, 0.5, 0.5, 1.0, 8),
                 lambda: ops.simce_lse_hard(x, x, sc, BETA),
                 lambda: ops.simce_grad_hard(x, x, sc, BETA, c3, c3, 0.5, 0.5, 1.0)):
        with pytest.raises(Err, match=UNSUPPORTED):
            call()
    # the widths the first plan cannot hold in LDS (8 waves of 128 columns): refused, not run
    for P in (964, 1020, 1024):
        x = torch.zeros(8, P, device=dev)
        for call in (lambda: ops.simce_lse(x, x, sc), lambda: ops.sim_logits(x, x, sc)):
            with pytest.raises(Err, match=UNSUPPORTED):
                call()
    # label_offset + Mx > Ny
    x, y = torch.zeros(8, 8, device=dev), torch.zeros(10, 8, device=dev)
    v8, v10 = torch.ones(8, device=dev), torch.ones(10, device=dev)
    for call in (lambda: ops.simce_lse_cls(x, y, sc, label_offset=3),
                 lambda: ops.simce_lse_hard(x, y, sc, BETA, label_offset=3),
                 lambda: ops.simce_grad_cls(x, y, sc, v8, v10, v8, v10, 0.5, 0.5, 1.0, 10, label_offset=3),
                 lambda: ops.simce_grad_hard(x, y, sc, BETA, torch.zeros(3, 8, device=dev), torch.zeros(3, 10, device=dev), 0.5,
                                             0.5, 1.0, label_offset=3)):
        with pytest.raises(Err, match=BAD_ARG):
            call()
    ops.simce_lse_cls(x, y, sc, label_offset=2)                 # the last offset that fits


# ---------------------------------------------------------------------------------------------- the tri-modal loss
@pytest.mark.parametrize("P", [36, 48, 160])
def test_plain_tri_modal_gradient_at_ragged_wave_slices(dev, P):
    """The plain batched gradient pass (clipk_simce_grad_pairs: the first-generation kernel) walks each wave's slice of
    P in blocks of 32 columns.  At P = 36, 48, 160 (slices of 40, 48, 80) it read and wrote past its LDS rows and
    returned a wrong dX without an error (simce section).  Now the entry
    refuses such P, and tri_modal_loss takes the batched class-aware gradient pass without ids for them: its gradients agree
    with f64 autograd.  Either the entry matches the reference or it refuses; never a silent wrong answer."""
    from clip_dplm_amd.loss import tri_modal_loss
    ops = _ops()
    B = 100
    E = torch.stack([R.unit_rows(B, P, 400 + m) for m in range(3)])
    Ed, sc = E.to(dev), torch.tensor([R.SCALE_A], device=dev)
    rev = [R.TRI_PAIRS.index((b, a)) for a, b in R.TRI_PAIRS]
    lse, pos = ops.simce_lse_pairs(Ed, R.TRI_PAIRS, sc)
    try:
        dX, dsc = ops.simce_grad_pairs(Ed, R.TRI_PAIRS, sc, lse, W_ROW, W_COL, 1.0 / B)
    except ops._ffi.ClipkError as e:
        assert "(status -2)" in str(e)
        assert R.first_gen_plan(B, B, P)[5] % 32 != 0
    else:
        for z, (a, b) in enumerate(R.TRI_PAIRS):
            L = R.Logits(E[a], E[b], None, R.SCALE_A)
            ref = R.plain_grad(L, 0, lse[z], lse[rev[z]], W_ROW, W_COL, 1.0 / B)
            _within(dX[z], ref[0], R.cap_dx(ref[2], ref[0]), "batched plain dX", f"ragged slice P={P}")
            _within(dsc[z], ref[1], ref[3], "batched plain dscale", f"ragged slice P={P}")
    # the public loss, backward with unequal weights on the three pair losses, against f64 autograd
    w = (1.0, -0.5, 2.25)
    leaves = [E[m].clone().to(dev).requires_grad_(True) for m in range(3)]
    s = torch.tensor(R.SCALE_A, device=dev, requires_grad=True)
    out = tri_modal_loss(*leaves, s)
    (w[0] * out["cell_pert_loss"] + w[1] * out["cell_protein_loss"] + w[2] * out["pert_protein_loss"]).backward()
    ref_leaves = [E[m].double().requires_grad_(True) for m in range(3)]
    rs = torch.tensor(R.SCALE_A, dtype=R.F64, requires_grad=True)
    lab = torch.arange(B)
    ce = torch.nn.functional.cross_entropy
    pair = lambda u, v: 0.5 * (ce(rs * u @ v.t(), lab) + ce(rs * v @ u.t(), lab))
    r = (pair(ref_leaves[0], ref_leaves[1]), pair(ref_leaves[0], ref_leaves[2]), pair(ref_leaves[1], ref_leaves[2]))
    (w[0] * r[0] + w[1] * r[1] + w[2] * r[2]).backward()
    for k, v in zip(("cell_pert_loss", "cell_protein_loss", "pert_protein_loss"), r):
        assert abs(out[k].item() - v.item()) <= 2e-5, (k, out[k].item(), v.item())
    for m in range(3):
        g, rg = leaves[m].grad.double().cpu(), ref_leaves[m].grad
        err = (g - rg).abs().max().item()
        assert torch.allclose(g, rg, rtol=1e-4, atol=1e-7), f"tri_modal_loss P={P} modality {m}: max |err| {err:.3e}"
    assert abs(s.grad.item() - rs.grad.item()) <= 1e-5 * max(1.0, abs(rs.grad.item()))


def test_plain_tri_modal_loss_refuses_a_ragged_slice_above_512(dev):
    from clip_dplm_amd.loss import tri_modal_loss
    ops = _ops()
    e = [R.unit_rows(40, 640, 500 + m).to(dev).requires_grad_(True) for m in range(3)]
    with pytest.raises(ops._ffi.ClipkError, match=UNSUPPORTED):
        tri_modal_loss(*e, torch.tensor(R.SCALE_A, device=dev))
    E, sc = torch.stack([t.detach() for t in e]), torch.tensor([R.SCALE_A], device=dev)
    lse, _ = ops.simce_lse_pairs(E, R.TRI_PAIRS, sc)
    with pytest.raises(ops._ffi.ClipkError, match=r"\(status -2\)"):
        ops.simce_grad_pairs(E, R.TRI_PAIRS, sc, lse, W_ROW, W_COL, 1.0 / 40)
    e = [R.unit_rows(40, 768, 510 + m).to(dev).requires_grad_(True) for m in range(3)]        # four waves of 96: runs
    tri_modal_loss(*e, torch.tensor(R.SCALE_A, device=dev))["loss"].backward()
    assert all(bool(torch.isfinite(t.grad).all()) for t in e)
