"""f64 reference and CPU stand-ins for the class-aware / hard-negative tri-modal loss (loss.tri_modal_loss with
class_ids / label_smoothing / hard_negative_beta; include/clipk.h: clipk_simce_{lse,grad}_pairs_{cls,hard}).

Nothing is defined here: per pair the loss is tests/class_aware_ref.py's resp. tests/hard_negative_ref.py's
`loss_from_logits` on the materialised f64 logits with w_row = w_col = 0.5, and the stand-ins (the signatures of
clip_dplm_amd.ops.simce_{lse,grad}_pairs_{cls,hard}) loop those files' unbatched stand-ins over the problems.

Inputs are built the way a PerturbAtlas batch is: four cells per perturbation, so the perturbation and protein rows of
a batch are near-duplicates in runs of four, and the ids sit above 2^40 to keep the int64 comparison honest.
"""
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import class_aware_ref as CR  # noqa: E402
import hard_negative_ref as HR  # noqa: E402

SCALE = 14.3
ID_BASE = 1 << 40
TRI_PAIRS = ((0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1))
PAIR_KEYS = ("cell_pert", "cell_protein", "pert_protein")
PAIR_MODS = ((0, 1), (0, 2), (1, 2))


def make_inputs(B, P, seed=0):
    """(cell, pert, prot) f64 [B, P] unit rows and ids int64 [B] = arange(B) // 4 + 2^40."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.arange(B) // 4 + ID_BASE
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ncls = (B + 3) // 4
    cell = F.normalize(r(B, P), dim=-1)
    pert = F.normalize(r(ncls, P)[ids - ID_BASE] + 0.05 * r(B, P), dim=-1)
    prot = F.normalize(r(ncls, P)[ids - ID_BASE] + 0.05 * r(B, P), dim=-1)
    return cell, pert, prot, ids


def pair_loss(a, b, scale, ids, same_class="mask", eps=0.0, beta=0.0):
    """One pair's symmetric loss from the definitions, in the dtype of a / b (f64 for the reference)."""
    S = scale * (a @ b.t())
    if beta > 0.0:
        return HR.loss_from_logits(S, b.shape[0], ids, beta, 0.5, 0.5)
    return CR.loss_from_logits(S, b.shape[0], ids, same_class, eps, 0.5, 0.5)


def tri_losses(cell, pert, prot, scale, ids3, same_class="mask", eps=0.0, beta=0.0):
    """(cell_pert, cell_protein, pert_protein) losses; ids3: the three pairs' ids (None: all distinct)."""
    E = (cell, pert, prot)
    return tuple(pair_loss(E[a], E[b], scale, t, same_class, eps, beta) for (a, b), t in zip(PAIR_MODS, ids3))


def assert_not_vacuous(cell, pert, prot, ids3, scale=SCALE):
    """The condition on the inputs: for every pair that is given ids, the f64 masked loss differs from the f64 plain
    loss by more than 5e-3 (500 x the loss tolerance) - else a kernel that ignored the ids would pass."""
    masked = tri_losses(cell.double(), pert.double(), prot.double(), scale, ids3)
    plain = tri_losses(cell.double(), pert.double(), prot.double(), scale, (None,) * 3)
    for key, t, m, p in zip(PAIR_KEYS, ids3, masked, plain):
        if t is not None:
            assert abs(m.item() - p.item()) > 5e-3, (key, m.item(), p.item())


def directed_reference(E, scale, ids6, same_class="mask", eps=0.0, beta=0.0, upstream=None):
    """f64, per directed problem of TRI_PAIRS over E [3, B, P]: the row statistics of the definition, the problem's
    one-directional CE, and - of the pair's symmetric loss L_ab (w_row = w_col = 0.5, both directions) times
    upstream[z] - dX = dL_ab / dE_a and dscale = dL_ab / dscale.  Returns a list of dicts."""
    E = E.double()
    out = []
    for z, ((a, b), ids) in enumerate(zip(TRI_PAIRS, ids6)):
        X = E[a].clone().requires_grad_(True)
        sc = torch.tensor(float(scale), dtype=torch.float64, requires_grad=True)
        S = sc * (X @ E[b].t())
        B = X.shape[0]
        if beta > 0.0:
            st = HR.stats(S, B, 0, ids, ids, beta)
            d = dict(lse=st["lse_h"].detach(), tgt=st["pos"].detach(), coef=HR.coefficients(st, beta).detach())
            L = HR.loss_from_logits(S, B, ids, beta, 0.5, 0.5)
        else:
            lse, tgt, cnt = CR.stats(S, B, 0, ids, ids, same_class, eps)[:3]
            d = dict(lse=lse.detach(), tgt=tgt.detach(), cnt=cnt)
            L = CR.loss_from_logits(S, B, ids, same_class, eps, 0.5, 0.5)
        d["ce"] = (d["lse"] - d["tgt"]).mean().item()
        g = 1.0 if upstream is None else float(upstream[z])
        d["dX"], d["dscale"] = torch.autograd.grad(g * L, (X, sc))
        d["dscale"] = d["dscale"].item()
        out.append(d)
    return out


# ---- stand-ins for clip_dplm_amd.ops (same signatures and return values), the unbatched stand-ins per problem
def simce_lse_pairs_cls(E, pairs, scale, ids=None, same_class="mask", eps=0.0):
    ids = [None] * len(pairs) if ids is None else ids
    res = [CR.simce_lse_cls(E[a], E[b], scale, t, t, same_class, eps) for (a, b), t in zip(pairs, ids)]
    return tuple(torch.stack(v) for v in zip(*res))


def _rev(pairs):
    pairs = list(pairs)
    return [pairs.index((b, a)) for a, b in pairs]


def simce_grad_pairs_cls(E, pairs, scale, lse, cnt, w_row, w_col, inv_bg, ids=None, same_class="mask", eps=0.0,
                         upstream=None):
    ids = [None] * len(pairs) if ids is None else ids
    B = E.shape[1]
    res = [CR.simce_grad_cls(E[a], E[b], scale, lse[z], lse[r], cnt[z], cnt[r], w_row, w_col, inv_bg, B, cls_x=ids[z],
                             cls_y=ids[z], same_class=same_class, eps=eps,
                             upstream=None if upstream is None else upstream[z])
           for z, ((a, b), r) in enumerate(zip(pairs, _rev(pairs)))]
    return tuple(torch.stack(v) for v in zip(*res))


def simce_lse_pairs_hard(E, pairs, scale, beta, ids=None):
    ids = [None] * len(pairs) if ids is None else ids
    res = [HR.simce_lse_hard(E[a], E[b], scale, beta, t, t) for (a, b), t in zip(pairs, ids)]
    return tuple(torch.stack(v) for v in zip(*res))


def simce_grad_pairs_hard(E, pairs, scale, beta, coef, w_row, w_col, inv_bg, ids=None, upstream=None):
    ids = [None] * len(pairs) if ids is None else ids
    res = [HR.simce_grad_hard(E[a], E[b], scale, beta, coef[z], coef[r], w_row, w_col, inv_bg, cls_x=ids[z],
                              cls_y=ids[z], upstream=None if upstream is None else upstream[z])
           for z, ((a, b), r) in enumerate(zip(pairs, _rev(pairs)))]
    return tuple(torch.stack(v) for v in zip(*res))


STAND_INS = ("simce_lse_pairs_cls", "simce_grad_pairs_cls", "simce_lse_pairs_hard", "simce_grad_pairs_hard")


def install(set_attr):
    """host_harness.install plus the four batched stand-ins of this file (set_attr: monkeypatch.setattr)."""
    import host_harness
    host_harness.install(set_attr)
    from clip_dplm_amd import ops
    me = sys.modules[__name__]
    for n in STAND_INS:
        set_attr(ops, n, getattr(me, n))
