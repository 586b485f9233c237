"""GPU: class-aware and hard-negative InfoNCE in the batched tri-modal form (include/clipk.h:
clipk_simce_{lse,grad}_pairs_{cls,hard}; loss.tri_modal_loss with class_ids / label_smoothing / hard_negative_beta),
and its use through ContrastiveModel and GraphedTrainStep.  The reference is the f64 restatement of the definitions
on materialised logits (tests/trimodal_variants_ref.py over class_aware_ref.py / hard_negative_ref.py).

Tolerances are those of test_gpu_class_aware_loss.py / test_gpu_hard_negative_loss.py: statistics 2e-5 (x (1 + 2 beta)
for the hard ones, as that file's header derives), loss 1e-5, dX rtol 1e-4 / atol 1e-6 (1 + beta), d scale
1e-5 max(1, |ref|) (1 + beta), counts exact.

Shapes (B, P): (32, 128) the notebook's batch, half-empty 64-tiles; (100, 128) ragged query and key edges, two query
blocks; (300, 64) five key tiles in more than one key split; (64, 512) the P limit."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trimodal_variants_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(32, 128), (100, 128), (300, 64), (64, 512)]
SHAPE_IDS = lambda s: "x".join(map(str, s))
UP6 = (1.0, 1.0, 0.5, 0.5, 2.0, 2.0)          # per-problem upstream gradients (both directions of a pair: one loss)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def _inputs(B, P):
    """Seeded inputs (f64, CPU) and the condition on them, once per shape."""
    cell, pert, prot, ids = T.make_inputs(B, P, seed=B + P)
    T.assert_not_vacuous(cell, pert, prot, (ids,) * 3)
    return cell, pert, prot, ids


@functools.lru_cache(maxsize=None)
def _directed(B, P, same_class, eps, beta, with_ids=(True, False, True)):
    """f64 reference of the six problems; the (cell, protein) pair carries no ids by default."""
    cell, pert, prot, ids = _inputs(B, P)
    E = torch.stack([cell, pert, prot]).float()                     # what the kernels are given
    ids6 = tuple(ids if w else None for w in with_ids for _ in range(2))
    return T.directed_reference(E, T.SCALE, ids6, same_class, eps, beta, upstream=UP6)


def _device_inputs(B, P, dev, with_ids=(True, False, True)):
    cell, pert, prot, ids = _inputs(B, P)
    E = torch.stack([cell, pert, prot]).float().to(dev)
    ids_d = ids.to(dev)
    ids6 = [ids_d if w else None for w in with_ids for _ in range(2)]
    return E, ids6, torch.tensor([T.SCALE], device=dev), torch.tensor(UP6, device=dev)


def _check_grads(dX, dsc, ref, beta, what):
    for z, r in enumerate(ref):
        err = (dX[z].double().cpu() - r["dX"]).abs().max().item()
        ds = dsc[z].sum().item()
        print(f"{what} problem {z}: max |dX - ref| {err:.2e}, dscale {ds:.6f} ref {r['dscale']:.6f}")
        assert torch.allclose(dX[z].double().cpu(), r["dX"], rtol=1e-4, atol=1e-6 * (1 + beta)), (what, z, err)
        assert abs(ds - r["dscale"]) < 1e-5 * max(1.0, abs(r["dscale"])) * (1 + beta), (what, z, ds, r["dscale"])


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("same_class", ["mask", "positive"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_batched_cls_ops_match_definition(dev, shape, same_class, eps):
    from clip_dplm_amd import ops
    B, P = shape
    ref = _directed(B, P, same_class, eps, 0.0)
    E, ids6, sc, up = _device_inputs(B, P, dev)
    lse, tgt, cnt = ops.simce_lse_pairs_cls(E, T.TRI_PAIRS, sc, ids6, same_class, eps)
    what = f"cls {shape} {same_class} eps={eps}"
    for z, r in enumerate(ref):
        e_l = (lse[z].double().cpu() - r["lse"]).abs().max().item()
        e_t = (tgt[z].double().cpu() - r["tgt"]).abs().max().item()
        ce = (lse[z] - tgt[z]).mean().item()
        print(f"{what} problem {z}: |dlse| {e_l:.2e} |dtgt| {e_t:.2e} ce {ce:.7f} ref {r['ce']:.7f}")
        assert e_l <= 2e-5 and e_t <= 2e-5, (what, z, e_l, e_t)
        assert torch.equal(cnt[z].double().cpu(), r["cnt"]), (what, z)
        assert abs(ce - r["ce"]) < 1e-5, (what, z, ce, r["ce"])
    dX, dsc = ops.simce_grad_pairs_cls(E, T.TRI_PAIRS, sc, lse, cnt, 0.5, 0.5, 1.0 / B, ids=ids6, same_class=same_class,
                                       eps=eps, upstream=up)
    _check_grads(dX, dsc, ref, 0.0, what)


@pytest.mark.parametrize("beta", [0.5, 2.0])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_batched_hard_ops_match_definition(dev, shape, beta):
    from clip_dplm_amd import ops
    B, P = shape
    ref = _directed(B, P, "mask", 0.0, beta)
    E, ids6, sc, up = _device_inputs(B, P, dev)
    lse_h, pos, coef = ops.simce_lse_pairs_hard(E, T.TRI_PAIRS, sc, beta, ids6)
    what = f"hard {shape} beta={beta}"
    tol = 2e-5 * (1 + 2 * beta)
    for z, r in enumerate(ref):
        e_l = (lse_h[z].double().cpu() - r["lse"]).abs().max().item()
        e_p = (pos[z].double().cpu() - r["tgt"]).abs().max().item()
        ce = (lse_h[z] - pos[z]).mean().item()
        print(f"{what} problem {z}: |dlse_h| {e_l:.2e} |dpos| {e_p:.2e} ce {ce:.7f} ref {r['ce']:.7f}")
        assert e_l <= tol and e_p <= tol, (what, z, e_l, e_p)
        assert torch.allclose(coef[z, 0].double().cpu(), r["coef"][0], rtol=0, atol=tol), (what, z)      # q in [0, 1]
        assert abs(ce - r["ce"]) < 1e-5, (what, z, ce, r["ce"])
    dX, dsc = ops.simce_grad_pairs_hard(E, T.TRI_PAIRS, sc, beta, coef, 0.5, 0.5, 1.0 / B, ids=ids6, upstream=up)
    _check_grads(dX, dsc, ref, beta, what)


@pytest.mark.parametrize("shape", [(100, 128), (300, 64)], ids=SHAPE_IDS)
def test_degenerate_classes(dev, shape):
    """All ids of one pair equal, "mask": every row's only key is its own partner - that pair's loss and dX are exactly
    0, for the class-aware and for the hard-negative entries; the other pairs' results keep their bits."""
    from clip_dplm_amd import ops
    B, P = shape
    E, ids6, sc, _ = _device_inputs(B, P, dev, (True, True, True))
    one = torch.full((B,), 7 + T.ID_BASE, dtype=torch.int64, device=dev)
    deg = [ids6[0], ids6[1], one, one, ids6[4], ids6[5]]
    lse, tgt, cnt = ops.simce_lse_pairs_cls(E, T.TRI_PAIRS, sc, deg)
    dX, dsc = ops.simce_grad_pairs_cls(E, T.TRI_PAIRS, sc, lse, cnt, 0.5, 0.5, 1.0 / B, ids=deg)
    lse0, tgt0, cnt0 = ops.simce_lse_pairs_cls(E, T.TRI_PAIRS, sc, ids6)
    dX0, dsc0 = ops.simce_grad_pairs_cls(E, T.TRI_PAIRS, sc, lse0, cnt0, 0.5, 0.5, 1.0 / B, ids=ids6)
    for z in (2, 3):
        assert torch.equal(lse[z], tgt[z]) and bool((cnt[z] == B).all())
        assert bool((dX[z] == 0).all()) and bool((dsc[z] == 0).all())
    for z in (0, 1, 4, 5):
        assert torch.equal(lse[z], lse0[z]) and torch.equal(tgt[z], tgt0[z]) and torch.equal(cnt[z], cnt0[z])
        assert torch.equal(dX[z], dX0[z]) and torch.equal(dsc[z], dsc0[z])
    lse_h, pos, coef = ops.simce_lse_pairs_hard(E, T.TRI_PAIRS, sc, 0.5, deg)
    dXh, dsh = ops.simce_grad_pairs_hard(E, T.TRI_PAIRS, sc, 0.5, coef, 0.5, 0.5, 1.0 / B, ids=deg)
    lse_h0, pos0, coef0 = ops.simce_lse_pairs_hard(E, T.TRI_PAIRS, sc, 0.5, ids6)
    dXh0, dsh0 = ops.simce_grad_pairs_hard(E, T.TRI_PAIRS, sc, 0.5, coef0, 0.5, 0.5, 1.0 / B, ids=ids6)
    for z in (2, 3):
        assert torch.equal(lse_h[z], pos[z])
        assert bool((dXh[z] == 0).all()) and bool((dsh[z] == 0).all())
    for z in (0, 1, 4, 5):
        assert torch.equal(lse_h[z], lse_h0[z]) and torch.equal(coef[z], coef0[z])
        assert torch.equal(dXh[z], dXh0[z]) and torch.equal(dsh[z], dsh0[z])


def _tri(dev, B, P, ups=(1.0, 1.0, 1.0), **kw):
    """tri_modal_loss + backward on the device -> (three losses, three embedding gradients, d scale)."""
    from clip_dplm_amd.loss import tri_modal_loss
    cell, pert, prot, _ = _inputs(B, P)
    leaves = [t.float().to(dev).requires_grad_(True) for t in (cell, pert, prot)]
    s = torch.tensor(T.SCALE, device=dev, requires_grad=True)
    out = tri_modal_loss(*leaves, s, **kw)
    losses = [out[k + "_loss"] for k in T.PAIR_KEYS]
    assert torch.equal(out["loss"], losses[0] + losses[1] + losses[2])
    sum(u * l for u, l in zip(ups, losses)).backward()
    return [l.detach() for l in losses], [t.grad for t in leaves], s.grad


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_plain_equivalence(dev, shape):
    """All-distinct ids and eps = 0: the plain tri-modal loss within the plain tolerances (beta = 0 through the
    hard-negative entries likewise); class_ids=None with the defaults: the plain path's bits."""
    from clip_dplm_amd import ops
    B, P = shape
    distinct = (torch.randperm(B, generator=torch.Generator().manual_seed(1)) * 5 + T.ID_BASE).to(dev)
    l0, g0, s0 = _tri(dev, B, P, (1.0, 0.5, 2.0))
    l1, g1, s1 = _tri(dev, B, P, (1.0, 0.5, 2.0), class_ids=distinct)
    for a, b in zip(l1, l0):
        assert abs(a.item() - b.item()) < 1e-5
    for a, b in zip(g1, g0):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-6), (a - b).abs().max()
    assert abs(s1.item() - s0.item()) < 1e-5 * max(1.0, abs(s0.item()))
    l2, g2, s2 = _tri(dev, B, P, (1.0, 0.5, 2.0), class_ids=None, same_class="mask", label_smoothing=0.0,
                      hard_negative_beta=0.0)
    assert all(torch.equal(a, b) for a, b in zip(l2 + g2 + [s2], l0 + g0 + [s0]))
    # beta = 0 is the plain loss (the entries take it; tri_modal_loss itself routes beta = 0 to the plain kernels)
    E, ids6, sc, _ = _device_inputs(B, P, dev, (False, False, False))
    lse_h, pos, coef = ops.simce_lse_pairs_hard(E, T.TRI_PAIRS, sc, 0.0, ids6)
    lse, pos0 = ops.simce_lse_pairs(E, T.TRI_PAIRS, sc)
    assert torch.allclose(lse_h, lse, rtol=0, atol=2e-5) and torch.allclose(pos, pos0, rtol=0, atol=2e-5)


@pytest.mark.parametrize("shape", [(100, 128), (300, 64)], ids=SHAPE_IDS)
def test_determinism(dev, shape):
    from clip_dplm_amd import ops
    B, P = shape
    E, ids6, sc, up = _device_inputs(B, P, dev)

    def run():
        lse, tgt, cnt = ops.simce_lse_pairs_cls(E, T.TRI_PAIRS, sc, ids6, "positive", 0.1)
        dX, dsc = ops.simce_grad_pairs_cls(E, T.TRI_PAIRS, sc, lse, cnt, 0.5, 0.5, 1.0 / B, ids=ids6,
                                           same_class="positive", eps=0.1, upstream=up)
        lse_h, pos, coef = ops.simce_lse_pairs_hard(E, T.TRI_PAIRS, sc, 0.5, ids6)
        dXh, dsh = ops.simce_grad_pairs_hard(E, T.TRI_PAIRS, sc, 0.5, coef, 0.5, 0.5, 1.0 / B, ids=ids6, upstream=up)
        return [t.clone() for t in (lse, tgt, cnt, dX, dsc, lse_h, pos, coef, dXh, dsh)]
    first, second = run(), run()
    assert all(torch.equal(a, b) for a, b in zip(first, second))


AUTOGRAD_CASES = {
    "mask": dict(same_class="mask"),
    "positive_eps": dict(same_class="positive", label_smoothing=0.1),
    "beta": dict(hard_negative_beta=0.5),
}


@pytest.mark.parametrize("case", list(AUTOGRAD_CASES))
@pytest.mark.parametrize("shape", [(32, 128), (300, 64)], ids=SHAPE_IDS)
def test_tri_modal_loss_autograd_vs_f64(dev, shape, case):
    """tri_modal_loss and its backward under unequal upstream gradients (1, 0, 2), ids on two of the three pairs."""
    B, P = shape
    kw = AUTOGRAD_CASES[case]
    beta = kw.get("hard_negative_beta", 0.0)
    cell, pert, prot, ids = _inputs(B, P)
    ups = (1.0, 0.0, 2.0)
    ids_d = ids.to(dev)
    got_l, got_g, got_s = _tri(dev, B, P, ups, class_ids={"cell_pert": ids_d, "pert_protein": ids_d}, **kw)
    leaves = [t.float().double().requires_grad_(True) for t in (cell, pert, prot)]
    s64 = torch.tensor(T.SCALE, dtype=torch.float64, requires_grad=True)
    ref = T.tri_losses(*leaves, s64, (ids, None, ids), kw.get("same_class", "mask"), kw.get("label_smoothing", 0.0), beta)
    sum(u * l for u, l in zip(ups, ref)).backward()
    for k, a, b in zip(T.PAIR_KEYS, got_l, ref):
        print(f"{case} {shape} {k}: {a.item():.7f} ref {b.item():.7f}")
        assert abs(a.item() - b.item()) < 1e-5, (k, a.item(), b.item())
    for a, b in zip(got_g, leaves):
        assert torch.allclose(a.double().cpu(), b.grad, rtol=1e-4, atol=1e-6 * (1 + beta)), (a.double().cpu() - b.grad).abs().max()
    assert abs(got_s.item() - s64.grad.item()) < 1e-5 * max(1.0, abs(s64.grad.item())) * (1 + beta)


def _model_inputs(dev):
    z = np.load(os.path.join(GOLDEN, "trimodal_model.npz"))
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}
    keys = ("cell_state", "connectivity", "gene_esm", "gene_values", "protein_emb")
    return tuple(torch.from_numpy(z[k]).to(dev) for k in keys), sd


def test_model_with_class_ids(dev):
    """ContrastiveModel(..., class_ids=ids) at B = 32: the embeddings are those of the call without ids, and each pair's
    loss is clip_loss(class_ids=ids) on those embeddings."""
    import clip_dplm_amd as K
    from clip_dplm_amd.loss import clip_loss
    inputs, sd = _model_inputs(dev)
    m = K.ContrastiveModel(21, 64, projection_dim=64, esm_dim=40)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    B = inputs[0].shape[0]
    ids = (torch.arange(B) // 4 + T.ID_BASE).to(dev)
    plain = m(*inputs)
    for kw in (dict(), dict(same_class="positive", label_smoothing=0.1), dict(hard_negative_beta=0.5)):
        out = m(*inputs, class_ids=ids, **kw)
        assert set(out) == set(plain)
        emb = [out[k] for k in ("cell_embed", "pert_embed", "protein_embed")]
        for k, e in zip(("cell_embed", "pert_embed", "protein_embed"), emb):
            assert torch.equal(e, plain[k]), k
        scale = m.logit_scale.exp()
        for key, (a, b) in zip(T.PAIR_KEYS, T.PAIR_MODS):
            want = clip_loss(emb[a].detach(), emb[b].detach(), scale.detach(), class_ids=ids, **kw)
            assert abs(out[key + "_loss"].item() - want.item()) < 1e-5, (kw, key, out[key + "_loss"].item(), want.item())
        assert out["loss"].item() != plain["loss"].item()


def test_graphed_train_step_with_class_ids_equals_eager(dev):
    """GraphedTrainStep over ContrastiveModel with the ids as one more input: different ids on every replay, the same
    losses and weights as the steps issued eagerly (the pattern of test_gpu_class_aware_loss.py's test of this name)."""
    import clip_dplm_amd as K
    from clip_dplm_amd.training import GraphedTrainStep
    inputs, _ = _model_inputs(dev)
    B = inputs[0].shape[0]

    def build():
        torch.manual_seed(2)
        m = K.ContrastiveModel(21, 64, projection_dim=64, esm_dim=40, dropout=0.0)
        for mod in m.modules():
            if isinstance(mod, torch.nn.Dropout):
                mod.p = 0.0
        return m.to(dev).train()
    g = torch.Generator().manual_seed(3)
    batches = []
    for k in range(4):
        noisy = tuple(x + 0.01 * k * torch.ones_like(x) if x.is_floating_point() and i in (0, 2, 4) else x
                      for i, x in enumerate(inputs))
        cls = torch.randint(0, 4 + 6 * k, (B,), generator=g) + T.ID_BASE
        batches.append(noisy + (cls.to(dev),))
    loss_of = lambda m: (lambda *x: m(*x[:-1], class_ids=x[-1], label_smoothing=0.1)["loss"])
    me = build()
    oe = K.FusedAdamW(me, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    eager = []
    for i, batch in enumerate(batches):
        oe.zero_grad()
        loss = loss_of(me)(*batch)
        loss.backward()
        oe.step(lr=1e-3 * (1 + i))
        eager.append(loss.item())
    mg = build()
    og = K.FusedAdamW(mg, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    step = GraphedTrainStep(mg, og, loss_of(mg), batches[0])
    graphed = [step(*batch, lr=1e-3 * (1 + i)).item() for i, batch in enumerate(batches)]
    assert graphed == eager, (graphed, eager)
    for (n, p), (_, q) in zip(me.named_parameters(), mg.named_parameters()):
        assert torch.equal(p, q), n
    assert build()(*batches[0][:-1])["loss"].item() != eager[0]          # the ids change the loss


def test_bad_arguments(dev):
    """CLIPK_ERR_UNSUPPORTED (-2) for P = 516 (> 512) and P = 130 (P % 4); CLIPK_ERR_BAD_ARG (-1) for npairs = 7, a
    modality index out of range and a reverse that is not the pair's other direction."""
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    bad_arg, unsupported = -1, -2
    B = 32
    f = lambda *s: torch.zeros(*s, device=dev)
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device=dev)
    sc = torch.ones(1, device=dev)
    ids = torch.zeros(B, dtype=torch.int64, device=dev)
    flat = [v for pr in T.TRI_PAIRS for v in pr]
    rev = [1, 0, 3, 2, 5, 4]
    ints = lambda v: (C.c_int * len(v))(*v)
    ptrs = lambda n: (C.c_void_p * n)(*([ids.data_ptr()] * n))

    def lse_cls(P, pairs=flat, n=6):
        E = f(3, B, P)
        return lib.clipk_simce_lse_pairs_cls(E.data_ptr(), 3, B, P, ints(pairs), n, sc.data_ptr(), ptrs(max(n, 6)), 0, 0.0,
                                             f(8, B).data_ptr(), f(8, B).data_ptr(), f(8, B).data_ptr(), ws.data_ptr(),
                                             ws.numel(), None)

    def grad_cls(P, pairs=flat, reverse=rev, n=6):
        E = f(3, B, P)
        return lib.clipk_simce_grad_pairs_cls(E.data_ptr(), 3, B, P, ints(pairs), ints(reverse), n, sc.data_ptr(),
                                              ptrs(max(n, 6)), 0, 0.0, f(8, B).data_ptr(), f(8, B).data_ptr(), 0.5, 0.5,
                                              1.0 / B, None, f(8, B, P).data_ptr(), f(8, B).data_ptr(), ws.data_ptr(),
                                              ws.numel(), None)

    def lse_hard(P, pairs=flat, n=6):
        E = f(3, B, P)
        return lib.clipk_simce_lse_pairs_hard(E.data_ptr(), 3, B, P, ints(pairs), n, sc.data_ptr(), 0.5, ptrs(max(n, 6)),
                                              f(8, B).data_ptr(), f(8, B).data_ptr(), f(8, 3, B).data_ptr(), ws.data_ptr(),
                                              ws.numel(), None)

    def grad_hard(P, pairs=flat, reverse=rev, n=6):
        E = f(3, B, P)
        return lib.clipk_simce_grad_pairs_hard(E.data_ptr(), 3, B, P, ints(pairs), ints(reverse), n, sc.data_ptr(), 0.5,
                                               ptrs(max(n, 6)), f(8, 3, B).data_ptr(), 0.5, 0.5, 1.0 / B, None,
                                               f(8, B, P).data_ptr(), f(8, B).data_ptr(), ws.data_ptr(), ws.numel(), None)
    seven = flat + [0, 1]
    for fn in (lse_cls, grad_cls, lse_hard, grad_hard):
        assert fn(516) == unsupported and fn(130) == unsupported, fn.__name__
        assert fn(128, pairs=[0, 3] + flat[2:]) == bad_arg, fn.__name__
    for fn in (lse_cls, lse_hard):
        assert fn(128, pairs=seven, n=7) == bad_arg and fn(128, n=0) == bad_arg, fn.__name__
    for fn in (grad_cls, grad_hard):
        assert fn(128, pairs=seven, reverse=rev + [6], n=7) == bad_arg, fn.__name__
        assert fn(128, reverse=[6] + rev[1:]) == bad_arg, fn.__name__
    for kind in ("cls", "hard"):
        size = getattr(lib, f"clipk_simce_pairs_{kind}_workspace")
        assert size(6, B, 516) == 0 and size(6, B, 130) == 0 and size(7, B, 128) == 0 and size(6, B, 128) > 0
    torch.cuda.synchronize()
