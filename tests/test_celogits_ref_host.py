"""tests/celogits_ref.py on the CPU: the f64 reference is pinned against torch's own F.cross_entropy + autograd at every
offset and rectangular case of the table, the f32 restatement stays inside `check`, every mutant of the restatement falls
outside it wherever it applies - so a kernel with the same mistake would fail tests/test_gpu_celogits.py - and the CPU
emulator of the two ops (tests/ops_emulator.py) follows the same contract."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import celogits_ref as R  # noqa: E402
import ops_emulator as E  # noqa: E402

F64 = torch.float64
KINDS = ("row", "col", "bwd")


def _cases(kind=None, family=None):
    return [c for c in R.CASES if (kind is None or c.kind == kind) and (family is None or c.family == family)]


# ------------------------------------------------------------------------------------------------ reference vs torch
@pytest.mark.parametrize("family", ["generic", "peaked"])
def test_reference_equals_torch_cross_entropy_and_autograd(family):
    """lse - pos is F.cross_entropy per row (column) at the label i + off, the rows without a label dropped on the torch
    side; bwd is autograd of  g (wr sum_rows CE + wc sum_cols CE)  with the lse of the reference itself."""
    n = 0
    for case in _cases(family=family):
        S, S2 = R.inputs(case)
        Sd = S.double().requires_grad_(True)
        S2d = S2.double().requires_grad_(True) if S2 is not None else None
        full = Sd if S2d is None else torch.cat([Sd, S2d], 1)
        if case.kind != "bwd":
            lse, pos = R.lse_cols(S, case.off) if case.kind == "col" else R.lse_rows(S, S2, case.off)
            logits = Sd.t() if case.kind == "col" else full
            # a label past N in [S | S2] would be a cache column: the kernels' pos is 0 there, torch's is not - cut to S
            lab = torch.arange(logits.shape[0]) + case.off
            ok = (lab >= 0) & (lab < (case.M if case.kind == "col" else case.N))
            assert torch.allclose(lse, torch.logsumexp(logits.detach(), 1), rtol=0, atol=1e-12), case.name
            assert (pos[~ok] == 0).all()
            if ok.any():
                ce = F.cross_entropy(logits[ok], lab[ok], reduction="none").detach()
                assert torch.allclose((lse - pos)[ok], ce, rtol=0, atol=1e-12), case.name
            n += 1
            continue
        wr, wc = R.WEIGHTS[case.weights]
        lr = R.lse_rows(S, S2, 0)[0] if case.weights != "col" else None
        lc = R.lse_cols(S, 0)[0] if case.weights != "row" else None
        dS, dS2 = R.bwd(S, S2, lr, lc, wr, wc, case.off, case.off_c, R.G)
        labr = torch.arange(case.M) + case.off
        okr = (labr >= 0) & (labr < case.N)
        labc = torch.arange(case.N) + case.off_c
        okc = (labc >= 0) & (labc < case.M)
        # rows / columns without a label still pull their softmax: their term is the lse alone
        loss = full.sum() * 0.0
        if lr is not None:
            loss = loss + wr * (torch.logsumexp(full, 1).sum() - Sd[torch.arange(case.M)[okr], labr[okr]].sum())
        if lc is not None:
            loss = loss + wc * (torch.logsumexp(Sd, 0).sum() - Sd[labc[okc], torch.arange(case.N)[okc]].sum())
        grads = torch.autograd.grad(R.G * loss, [Sd] + ([S2d] if S2d is not None else []), allow_unused=True)
        assert torch.allclose(dS, grads[0], rtol=0, atol=1e-12), case.name
        if S2d is not None:
            want = grads[1] if grads[1] is not None else torch.zeros_like(S2d)
            assert torch.allclose(dS2, want, rtol=0, atol=1e-12), case.name
        n += 1
    assert n > 300


def test_reference_with_label_rows_equals_cross_entropy_mean():
    """The module API's own calls: F.cross_entropy(cat([S, S2], 1), arange) and F.cross_entropy(S.t(), arange), mean
    reduction, and their autograd - what KF.cross_entropy_diag computes."""
    g = torch.Generator().manual_seed(3)
    B, Nc = 37, 21
    S, S2 = torch.randn(B, B, generator=g) * 4, torch.randn(B, Nc, generator=g) * 4
    Sd, S2d = S.double().requires_grad_(True), S2.double().requires_grad_(True)
    lab = torch.arange(B)
    loss = 0.5 * (F.cross_entropy(torch.cat([Sd, S2d], 1), lab) + F.cross_entropy(Sd.t(), lab))
    gS, gS2 = torch.autograd.grad(1.7 * loss, [Sd, S2d])
    lr, pr = R.lse_rows(S, S2, 0)
    lc, pc = R.lse_cols(S, 0)
    assert abs(float(0.5 * ((lr - pr).mean() + (lc - pc).mean()) - loss.detach())) < 1e-12
    dS, dS2 = R.bwd(S, S2, lr, lc, 0.5 / B, 0.5 / B, 0, 0, 1.7)
    assert torch.allclose(dS, gS, rtol=0, atol=1e-13) and torch.allclose(dS2, gS2, rtol=0, atol=1e-13)


def test_reference_on_minus_infinity():
    """-inf logits are zero terms (torch.logsumexp agrees), a row / column without a finite one has lse = -inf, and its
    gradient is NaN in the reference - the marker for "not compared"."""
    for case in _cases(family="holes") + _cases(family="onehot"):
        S, S2 = R.inputs(case)
        ref = R.reference(case, S, S2)
        if case.kind == "bwd":
            lr, lc, _, _ = R.lse_inputs(case, S, S2)
            dead = torch.zeros(case.M, case.N, dtype=torch.bool)
            if lr is not None:
                dead |= (lr == -R.INF)[:, None]
            if lc is not None:
                dead |= (lc == -R.INF)[None, :]
            assert torch.equal(torch.isnan(ref["dS"]), dead), case.name
            continue
        full = S if S2 is None else torch.cat([S, S2], 1)
        want = torch.logsumexp(S.double(), 0) if case.kind == "col" else torch.logsumexp(full.double(), 1)
        assert not torch.isnan(ref["lse"]).any()
        assert torch.equal(ref["lse"] == -R.INF, want == -R.INF), case.name
        fin = torch.isfinite(want)
        assert torch.allclose(ref["lse"][fin], want[fin], rtol=0, atol=1e-12)
        if case.family == "onehot":                         # one live term: the lse IS that logit
            live = torch.isfinite(S.double() if case.kind == "col" else full.double())
            assert (live.sum(0 if case.kind == "col" else 1) <= 1).all()
            assert torch.equal(ref["lse"], (S.double() if case.kind == "col" else full.double()).max(0 if case.kind == "col" else 1).values)


# ------------------------------------------------------------------------------------------------ restatement and mutants
def test_case_table_covers_the_geometry():
    rows = {(c.M, c.N, c.N2) for c in _cases("row")}
    assert set(R.ROW_SHAPES) <= rows and len(R.ROW_SHAPES) == 5 * 7 * 5
    assert set(R.COL_SHAPES) <= {(c.M, c.N) for c in _cases("col")} and len(R.COL_SHAPES) == 35
    for fam in R.FAMILIES:
        b = _cases("bwd", fam)
        assert {(c.N, c.N2) for c in b} >= set(R.BWD_SHAPES)
        assert {c.weights for c in b} == ({"row", "col"} if fam == "onehot" else {"row", "both", "col"})
        for kind in KINDS:
            cs = _cases(kind, fam)
            assert {c.off for c in cs} >= {0, 3, -3} and any(c.off == c.N for c in cs)
            assert 0.3 < sum(c.pad for c in cs) / len(cs) < 0.7
        assert any(c.joint for c in _cases("row", fam)) and any(c.joint for c in b)
        assert any(c.M != c.N for c in b)
        assert any(c.N < 64 and c.N2 > 0 for c in _cases("row", fam)) and any(c.N2 > c.N for c in _cases("row", fam))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_restatement_is_inside_the_bound(family, kind):
    """By construction at most 1 / 8 of the bound; pos is a copy and the onehot family is exact, bit for bit."""
    for case in _cases(kind, family):
        S, S2 = R.inputs(case)
        ref, st = R.reference(case, S, S2), R.restate(case, S, S2)
        for nm, r in ref.items():
            if r is None:
                assert st[nm] is None
                continue
            assert R.check(st[nm], r, st[nm], f"{case.name} {nm}") <= 1 / R.MARGIN + 1e-12
            exact = nm == "pos" or (family == "onehot" and nm == "lse")
            if exact:
                assert torch.equal(st[nm].double(), r), (case.name, nm)
        if family == "onehot" and kind == "bwd":
            # exp(0) = 1: dS is 0 on the label and g w beside it, dS2 is g w or 0 - one f32 product
            lr, lc, wr, wc = R.lse_inputs(case, S, S2)
            w = torch.tensor(wr if lr is not None else wc, dtype=torch.float32)
            gw = torch.tensor(R.G, dtype=torch.float32) * w
            cmp = ~torch.isnan(ref["dS"])
            assert set(st["dS"][cmp].tolist()) <= {0.0, -0.0, float(gw), float(-gw)}, case.name


@pytest.mark.parametrize("mutant", list(R.MUTANTS), ids=list(R.MUTANTS))
def test_every_mutant_is_rejected_wherever_it_applies(mutant):
    """`check` rejects the f32 mutant at every case it applies to, and it applies somewhere in every family and kernel it
    is about (the counts are printed: structural cases / cases where its exact effect is above twice the bound)."""
    seen = {}
    for case in R.CASES:
        if not R.structural(mutant, case):
            continue
        S, S2 = R.inputs(case)
        ref, st = R.reference(case, S, S2), R.restate(case, S, S2)
        key = (case.family, case.kind)
        seen.setdefault(key, [0, 0])[0] += 1
        if not R.applies(mutant, case, S, S2, ref, st):
            continue
        seen[key][1] += 1
        bad = R.rejected(R.restate(case, S, S2, mutant=mutant), ref, st, f"{case.name} [{mutant}]")
        assert bad, (case.name, mutant, R.MUTANTS[mutant])
    for key, (n_struct, n_app) in sorted(seen.items()):
        print(f"{mutant}: {key[0]:8s} {key[1]:4s} structural {n_struct:4d}  applies {n_app:4d}")
    kinds = {"merge_unscaled": ("row", "col"), "no_cache": ("row",), "pos_no_offset": ("row", "col"),
             "col_pos_transposed": ("col",), "onehot_minus": ("bwd",), "ds2_col_term": ("bwd",), "g_dropped": ("bwd",),
             "stride_n": KINDS, "ragged_cols": KINDS, "ragged_rows": KINDS, "three_slices": ("col",), "d1": ("row", "col")}[mutant]
    # merging unscaled cannot show on onehot: one live pair per row, l = 1 and nothing to rescale
    # ... nor can a column term on onehot's dS2: where the columns carry the one logit, S2 holds none
    fams = {"merge_unscaled": R.FAMILIES[:3], "ds2_col_term": R.FAMILIES[:3], "d1": ("holes", "onehot")}.get(mutant, R.FAMILIES)
    for fam in fams:
        for kind in kinds:
            assert seen.get((fam, kind), [0, 0])[1] > 0, (mutant, fam, kind, "applies nowhere")


def test_d1_is_rejected_exactly_where_a_finite_logit_follows_a_masked_one():
    """Mutant 12 is the code before the fix.  It applies - and `check` rejects it, with a NaN lse - at exactly the holes and
    onehot cases where some lane (row slice) meets -inf before a finite logit (celogits_ref.d1_trigger): more than half of
    the row cases, and the column cases with M > 4."""
    n = {}
    for case in _cases(family="holes") + _cases(family="onehot"):
        if case.kind == "bwd":
            continue
        S, S2 = R.inputs(case)
        ref, st = R.reference(case, S, S2), R.restate(case, S, S2)
        trig = R.d1_trigger(case, S, S2)
        assert R.applies("d1", case, S, S2, ref, st) == trig, case.name
        mu = R.restate(case, S, S2, mutant="d1")
        assert torch.isnan(mu["lse"]).any() == trig, case.name
        assert bool(R.rejected(mu, ref, st, case.name)) == trig, case.name
        n.setdefault((case.family, case.kind), []).append(trig)
    for key, v in sorted(n.items()):
        print(f"d1 {key}: {sum(v)} of {len(v)} cases")
        assert sum(v) >= (0.5 * len(v) if key[1] == "row" else 10), key


# ------------------------------------------------------------------------------------------------ the emulator (D3)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_emulator_follows_the_kernel_contract(family):
    """ops_emulator.ce_logits_lse / ce_logits_bwd in f64 equal the reference on the whole table: offsets in both
    directions, rectangular S, pos = 0 and no one-hot for a label outside S, -inf logits."""
    for case in _cases(family=family):
        S, S2 = R.inputs(case)
        ref = R.reference(case, S, S2)
        Sd, S2d = S.double(), (S2.double() if S2 is not None else None)
        if case.kind != "bwd":
            lse, pos = E.ce_logits_lse(Sd, S2d, columns=case.kind == "col", label_offset=case.off)
            assert lse.shape == pos.shape == ref["lse"].shape, case.name
            assert torch.equal(pos, ref["pos"]), case.name
            fin = torch.isfinite(ref["lse"])
            assert torch.equal(lse[~fin], ref["lse"][~fin]) and torch.allclose(lse[fin], ref["lse"][fin], rtol=0, atol=1e-12)
            continue
        lr, lc, wr, wc = R.lse_inputs(case, S, S2)
        dS, dS2 = E.ce_logits_bwd(Sd, S2d, None if lr is None else lr.double(), None if lc is None else lc.double(), wr, wc,
                                  R.G, off_row=case.off, off_col=case.off_c)
        for got, want in ((dS, ref["dS"]), (dS2, ref["dS2"])):
            if want is None:
                assert got is None
                continue
            cmp = ~torch.isnan(want)
            assert torch.allclose(got[cmp], want[cmp], rtol=0, atol=1e-13), case.name


def test_emulator_refuses_cache_columns_in_the_column_direction():
    with pytest.raises(ValueError):
        E.ce_logits_lse(torch.zeros(3, 3), torch.zeros(3, 2), columns=True)
