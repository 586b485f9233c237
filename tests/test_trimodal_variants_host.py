"""CPU: the host logic of the class-aware / hard-negative tri-modal loss (loss.tri_modal_loss with class_ids,
label_smoothing, hard_negative_beta): argument validation, the calls the default makes, loss and autograd gradients of
the three returned losses against the f64 definition, and the world-2 (gloo) path.  The HIP kernels cannot run here:
tests/trimodal_variants_ref.py's stand-ins (and host_harness's) replace clip_dplm_amd.ops.*."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import trimodal_variants_ref as T  # noqa: E402
from host_harness import run_ranks, trap_calls  # noqa: E402

B, P = 48, 32
PAIRS_OPS = ("simce_lse_pairs", "simce_grad_pairs") + T.STAND_INS


@pytest.fixture
def stand_ins(monkeypatch):
    T.install(monkeypatch.setattr)
    return monkeypatch


def _inputs(B=B, P=P, seed=0):
    cell, pert, prot, ids = T.make_inputs(B, P, seed)
    return cell.float(), pert.float(), prot.float(), ids


def test_argument_validation(stand_ins):
    from clip_dplm_amd.loss import tri_modal_loss
    cell, pert, prot, ids = _inputs()
    s = torch.tensor(T.SCALE)
    call = lambda **kw: tri_modal_loss(cell, pert, prot, s, **kw)
    with pytest.raises(ValueError, match="cell_rna"):
        call(class_ids={"cell_rna": ids})
    with pytest.raises(ValueError):
        call(class_ids=[ids, ids, ids])
    with pytest.raises(ValueError, match="shape"):
        call(class_ids=ids[:-1])
    with pytest.raises(ValueError, match="shape"):
        call(class_ids={"pert_protein": ids.reshape(-1, 1)})
    with pytest.raises(ValueError, match="integer"):
        call(class_ids=ids.float())
    with pytest.raises(ValueError, match="integer"):
        call(class_ids={"cell_protein": ids.double()})
    with pytest.raises(ValueError, match="are on"):
        call(class_ids=ids.to("meta"))
    with pytest.raises(ValueError, match="same_class"):
        call(class_ids=ids, same_class="drop")
    with pytest.raises(ValueError, match="label_smoothing"):
        call(label_smoothing=1.0)
    with pytest.raises(ValueError, match="positive"):
        call(class_ids=ids, same_class="positive", hard_negative_beta=0.5)
    with pytest.raises(ValueError, match="label_smoothing"):
        call(hard_negative_beta=0.5, label_smoothing=0.1)
    with pytest.raises(ValueError, match="hard_negative_beta"):
        call(hard_negative_beta=-1.0)


def test_batched_ops_validate_their_operands():
    """ops.simce_*_pairs_{cls,hard} raise ValueError (not assert) before anything reaches the library."""
    from clip_dplm_amd import ops
    E = torch.zeros(3, 8, 16)
    s = torch.ones(1)
    ids = torch.zeros(8, dtype=torch.int64)
    six = [ids] * 6
    with pytest.raises(ValueError, match="E must be"):
        ops.simce_lse_pairs_cls(E.double(), T.TRI_PAIRS, s)
    with pytest.raises(ValueError, match="1 to 6"):
        ops.simce_lse_pairs_cls(E, T.TRI_PAIRS + ((0, 1),), s)
    with pytest.raises(ValueError, match="modalities"):
        ops.simce_lse_pairs_hard(E, ((0, 3), (3, 0)), s, 0.5)
    with pytest.raises(ValueError, match="P <= 512"):
        ops.simce_lse_pairs_cls(torch.zeros(3, 8, 18), T.TRI_PAIRS, s)
    with pytest.raises(ValueError, match="ids"):
        ops.simce_lse_pairs_cls(E, T.TRI_PAIRS, s, ids=six[:5])
    with pytest.raises(ValueError, match="int64"):
        ops.simce_lse_pairs_cls(E, T.TRI_PAIRS, s, ids=[ids.int()] * 6)
    with pytest.raises(ValueError, match="same ids"):
        ops.simce_lse_pairs_hard(E, T.TRI_PAIRS, s, 0.5, ids=[ids, ids.clone()] + six[2:])
    with pytest.raises(ValueError, match="same_class"):
        ops.simce_lse_pairs_cls(E, T.TRI_PAIRS, s, ids=six, same_class="drop")
    with pytest.raises(ValueError, match="beta"):
        ops.simce_lse_pairs_hard(E, T.TRI_PAIRS, s, float("inf"))
    with pytest.raises(ValueError, match="lse"):
        ops.simce_grad_pairs_cls(E, T.TRI_PAIRS, s, torch.zeros(6, 7), torch.zeros(6, 8), 0.5, 0.5, 0.125)
    with pytest.raises(ValueError, match="coef"):
        ops.simce_grad_pairs_hard(E, T.TRI_PAIRS, s, 0.5, torch.zeros(6, 8, 3), 0.5, 0.5, 0.125)
    with pytest.raises(ValueError, match="upstream"):
        ops.simce_grad_pairs_hard(E, T.TRI_PAIRS, s, 0.5, torch.zeros(6, 3, 8), 0.5, 0.5, 0.125, upstream=torch.ones(3))


def test_default_call_makes_only_the_plain_pairs_calls(stand_ins):
    from clip_dplm_amd.loss import tri_modal_loss
    calls = trap_calls(stand_ins.setattr, PAIRS_OPS + ("simce_lse", "simce_grad", "simce_lse_cls", "simce_lse_hard"))
    cell, pert, prot, ids = _inputs()
    leaves = [t.clone().requires_grad_(True) for t in (cell, pert, prot)]
    s = torch.tensor(T.SCALE, requires_grad=True)
    for kw in ({}, dict(class_ids=None, same_class="mask", label_smoothing=0.0, hard_negative_beta=0.0),
               dict(class_ids={}), dict(class_ids={"cell_pert": None})):
        del calls[:]
        tri_modal_loss(*leaves, s, **kw)["loss"].backward()
        assert calls == ["simce_lse_pairs", "simce_grad_pairs"], (kw, calls)
    del calls[:]
    tri_modal_loss(*leaves, s, class_ids=ids)["loss"].backward()
    assert calls == ["simce_lse_pairs_cls", "simce_grad_pairs_cls"], calls
    del calls[:]
    tri_modal_loss(*leaves, s, class_ids=ids, hard_negative_beta=0.5)["loss"].backward()
    assert calls == ["simce_lse_pairs_hard", "simce_grad_pairs_hard"], calls


CASES = {
    "mask": (dict(same_class="mask"), "all"),
    "positive_eps": (dict(same_class="positive", label_smoothing=0.1), "all"),
    "smoothing_only": (dict(label_smoothing=0.1), "none"),
    "beta_ids": (dict(hard_negative_beta=0.5), "all"),
    "one_pair": (dict(same_class="mask"), "pert_protein"),
    "one_pair_beta": (dict(hard_negative_beta=2.0), "cell_pert"),
}


@pytest.mark.parametrize("upstream", [(1.0, 1.0, 1.0), (1.0, 0.0, 2.0)], ids=["sum", "up102"])
@pytest.mark.parametrize("case", list(CASES))
def test_loss_and_gradients_match_the_f64_definition(stand_ins, case, upstream):
    from clip_dplm_amd.loss import tri_modal_loss
    kw, which = CASES[case]
    cell, pert, prot, ids = _inputs()
    if which == "all":
        class_ids, ids3 = ids, (ids,) * 3
    elif which == "none":
        class_ids, ids3 = None, (None,) * 3
    else:
        class_ids = {which: ids}
        ids3 = tuple(ids if k == which else None for k in T.PAIR_KEYS)
    T.assert_not_vacuous(cell, pert, prot, ids3)
    leaves = [t.clone().requires_grad_(True) for t in (cell, pert, prot)]
    s = torch.tensor(T.SCALE, requires_grad=True)
    out = tri_modal_loss(*leaves, s, class_ids=class_ids, **kw)
    got = (out["cell_pert_loss"], out["cell_protein_loss"], out["pert_protein_loss"])
    assert torch.equal(out["loss"], got[0] + got[1] + got[2])
    sum(u * l for u, l in zip(upstream, got)).backward()
    ref_leaves = [t.double().requires_grad_(True) for t in (cell, pert, prot)]
    s64 = torch.tensor(T.SCALE, dtype=torch.float64, requires_grad=True)
    ref = T.tri_losses(*ref_leaves, s64, ids3, kw.get("same_class", "mask"), kw.get("label_smoothing", 0.0),
                       kw.get("hard_negative_beta", 0.0))
    sum(u * l for u, l in zip(upstream, ref)).backward()
    beta = kw.get("hard_negative_beta", 0.0)
    for g, r in zip(got, ref):
        assert abs(g.item() - r.item()) < 1e-5, (case, g.item(), r.item())
    for t, r in zip(leaves, ref_leaves):
        assert torch.allclose(t.grad.double(), r.grad, rtol=1e-4, atol=1e-6 * (1 + beta)), (t.grad.double() - r.grad).abs().max()
    assert abs(s.grad.item() - s64.grad.item()) < 1e-5 * max(1.0, abs(s64.grad.item())) * (1 + beta)


def test_model_forwards_the_keywords(stand_ins):
    """ContrastiveModel.forward hands class_ids / same_class / label_smoothing / hard_negative_beta to tri_modal_loss."""
    import clip_dplm_amd.modeling_trimodal as M
    seen = {}

    def spy(cell, pert, prot, scale, group=None, **kw):
        seen.update(kw, group=group)
        return {"loss": scale.sum()}
    stand_ins.setattr(M, "tri_modal_loss", spy)
    m = M.ContrastiveModel.__new__(M.ContrastiveModel)
    torch.nn.Module.__init__(m)
    m.slice_first_position, m.multi_stream = False, False
    m.logit_scale = torch.nn.Parameter(torch.zeros(()))
    emb = torch.nn.functional.normalize(torch.ones(4, 8), dim=-1)
    for name in ("cell", "pert", "protein"):
        setattr(m, f"{name}_encoder", lambda *a: emb)
        setattr(m, f"{name}_projection", lambda x: x)
    stand_ins.setattr(M.KF, "l2_normalize", lambda x: x)
    ids = torch.arange(4)
    out = m.forward(emb, emb, emb, emb, emb, class_ids=ids, same_class="positive", label_smoothing=0.1)
    assert set(out) == {"cell_embed", "pert_embed", "protein_embed", "loss"}
    assert seen["class_ids"] is ids and seen["same_class"] == "positive" and seen["label_smoothing"] == 0.1
    assert seen["hard_negative_beta"] == 0.0 and seen["group"] is None


GLOO_CASES = [dict(same_class="mask"), dict(same_class="positive", label_smoothing=0.1), dict(hard_negative_beta=0.5)]


def _tri_case(kw, rows, group):
    from clip_dplm_amd.loss import tri_modal_loss
    cell, pert, prot, ids = _inputs(B=24, P=16, seed=3)
    leaves = [t[rows].clone().requires_grad_(True) for t in (cell, pert, prot)]
    s = torch.tensor(T.SCALE, requires_grad=True)
    out = tri_modal_loss(*leaves, s, group=group, class_ids={"cell_pert": ids[rows].clone(), "pert_protein": ids[rows].clone()},
                         **kw)
    (out["cell_pert_loss"] + 2.0 * out["pert_protein_loss"] + 0.5 * out["cell_protein_loss"]).backward()
    return ([out[k + "_loss"].item() for k in T.PAIR_KEYS], [t.grad.clone() for t in leaves], s.grad.clone())


def _rank_body(rank, world):
    import torch.distributed as dist
    n = 24 // world
    return [_tri_case(kw, slice(rank * n, (rank + 1) * n), dist.group.WORLD) for kw in GLOO_CASES]


@pytest.mark.timeout(300)
def test_world2_matches_single_process(stand_ins):
    """With a process group of two ranks tri_modal_loss is three global-batch clip_loss calls with the pair's ids: the
    same losses on every rank and the same gradients as the single-process (batched) path on the concatenated batch."""
    world = 2
    res = run_ranks(_rank_body, world)
    n = 24 // world
    for k, kw in enumerate(GLOO_CASES):
        losses, grads, ds = _tri_case(kw, slice(0, 24), None)
        for r in range(world):
            l_r, g_r, ds_r = res[r][k]
            assert all(abs(a - b) < 1e-6 for a, b in zip(l_r, losses)), (kw, l_r, losses)
            for a, b in zip(g_r, grads):
                assert torch.allclose(a, b[r * n:(r + 1) * n], rtol=1e-5, atol=1e-7), kw
        assert abs(sum(res[r][k][2].item() for r in range(world)) - ds.item()) < 1e-5 * max(1.0, abs(ds.item())), kw
