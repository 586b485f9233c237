"""CPU: the sequence of kernel-namespace calls and collectives behind loss.clip_loss, variant by variant.

Recorded through the loss._kernels seam (the stand-ins of tests/host_harness.py, each wrapped) and thin wrappers around
dist.all_gather_into_tensor and dist.all_reduce: per call the name, the tensor shapes and the scalar arguments, forward
and backward, at world size 1 (no group) and 2 (gloo).  The expected lists are written out below from the shapes alone:
plain, class-aware and hard-negative loss must keep their launches, operands and collectives whatever the autograd
plumbing around them looks like.
"""
import inspect
import os
import sys

import pytest
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import host_harness as H  # noqa: E402

BL, P, NC = 12, 16, 5
OPS = ("simce_lse", "simce_grad", "ce_combine", "simce_lse_cls", "simce_grad_cls", "simce_lse_hard", "simce_grad_hard")
INF, NULL_COEF = "+inf", "(0, -inf, -inf)"

# (clip_loss keywords but class_ids, with class ids)
VARIANTS = {
    "plain": (dict(), False),
    "mask_smoothed": (dict(same_class="mask", label_smoothing=0.1), True),
    "positive": (dict(same_class="positive", label_smoothing=0.0), True),
    "smoothed_no_ids": (dict(label_smoothing=0.1), False),
    "hard": (dict(hard_negative_beta=0.5), False),
    "hard_ids": (dict(hard_negative_beta=2.0), True),
}
CASES = [(v, sym, cache) for v in VARIANTS for sym in (True, False) for cache in (False, True)]


def _describe(v):
    """A tensor as its shape (a sentinel of the one-sided loss as its name and shape), anything else as it is."""
    if not torch.is_tensor(v):
        return v
    shape = tuple(v.shape)
    if v.is_floating_point() and v.numel():
        if bool((v == float("inf")).all()):
            return (INF, shape)
        if v.dim() == 2 and v.shape[0] == 3 and bool((v[0] == 0).all()) and bool((v[1:] == float("-inf")).all()):
            return (NULL_COEF, shape)
    return shape


def _record_calls(set_attr, log):
    """Wrap the installed stand-ins and the two collectives; every call appends (name, {argument: description})."""
    from clip_dplm_amd import ops

    def wrap(name, fn):
        sig = inspect.signature(fn)

        def f(*args, **kw):
            bound = sig.bind(*args, **kw)
            bound.apply_defaults()
            log.append((name, {k: _describe(v) for k, v in bound.arguments.items()}))
            return fn(*args, **kw)
        return f
    for n in OPS:
        set_attr(ops, n, wrap(n, getattr(ops, n)))
    gather, reduce = dist.all_gather_into_tensor, dist.all_reduce

    def all_gather_into_tensor(out, t, group=None):
        log.append(("all_gather_into_tensor", dict(out=tuple(out.shape), inp=tuple(t.shape))))
        return gather(out, t, group=group)

    def all_reduce(t, group=None):
        log.append(("all_reduce", dict(t=tuple(t.shape))))
        return reduce(t, group=group)
    set_attr(dist, "all_gather_into_tensor", all_gather_into_tensor)
    set_attr(dist, "all_reduce", all_reduce)


def _rank_body(rank, world, set_attr=setattr):
    log = []
    _record_calls(set_attr, log)
    cases = [(VARIANTS[v][1], cache, dict(VARIANTS[v][0], symmetric=sym)) for v, sym, cache in CASES]
    return [calls for *_, calls in H.clip_loss_cases(cases, log, rank, world, BL, P, NC)]


def _expected(variant, symmetric, with_cache, world, rank):
    kw, with_ids = VARIANTS[variant]
    off, bg, nc = rank * BL, world * BL, NC if with_cache else 0
    X, G, C, S1, V, VG = (BL, P), (bg, P), (NC, P) if with_cache else None, (1,), (BL,), (bg,)
    ids = dict(cls_x=V, cls_y=VG) if with_ids else dict(cls_x=None, cls_y=None)
    w_row, w_col = (0.5, 0.5) if symmetric else (1.0, 0.0)
    real = lambda shape: shape
    # per variant: the kernels' suffix, the rows of the statistics gather, its own scalars and operands, the per-row
    # statistics of a gradient call (mine: the rows' own, keys: the gathered ones of the other direction)
    if "hard_negative_beta" in kw:
        op, rows, own, nkeys = "_hard", 6, dict(ids, beta=kw["hard_negative_beta"]), lambda n: {}
        null = real if symmetric else lambda shape: (NULL_COEF, shape)
        stats = lambda mine, keys: dict(coef_x=mine((3, BL)), coef_y=keys((3, bg)))
    elif variant == "plain":
        op, rows, own, nkeys = "", 2, {}, lambda n: {}
        null = real if symmetric else lambda shape: (INF, shape)
        stats = lambda mine, keys: dict(lse_x=mine(V), lse_y=keys(VG))
    else:       # nkeys_y: a's rows meet the Bg rows of a as the keys of b's direction, b's rows the Bg + Nc keys of a's
        op, rows, nkeys = "_cls", 4, lambda n: dict(nkeys_y=n)
        own = dict(ids, same_class=kw.get("same_class", "mask"), eps=kw["label_smoothing"])
        null = real if symmetric else lambda shape: (INF, shape)
        stats = lambda mine, keys: dict(lse_x=mine(V), lse_y=keys(VG), cnt_x=V, cnt_y=VG)
    common = dict(x=X, y=G, scale=S1, label_offset=off, **own)
    seq = [("simce_lse" + op, dict(cache=C, **common))] + [("simce_lse" + op, dict(cache=None, **common))] * symmetric
    if world == 1:
        c = V if symmetric else None
        seq.append(("ce_combine", dict(lse_r=V, pos_r=V, lse_c=c, pos_c=c, w_row=w_row, w_col=w_col, bg=bg)))
    else:
        gathers = [((2, BL, P), (world * 2, BL, P))] + [(V, VG)] * with_ids + [((rows, BL), (world * rows, BL))]
        seq[:0] = [("all_gather_into_tensor", dict(out=o, inp=i)) for i, o in gathers[:-1]]
        seq += [("all_gather_into_tensor", dict(out=gathers[-1][1], inp=gathers[-1][0])), ("all_reduce", dict(t=()))]
    common.update(inv_bg=1.0 / bg, upstream=S1)
    seq.append(("simce_grad" + op, dict(w_row=w_row, w_col=w_col, cache=C, **stats(real, null), **nkeys(bg), **common)))
    seq.append(("simce_grad" + op, dict(w_row=w_col, w_col=w_row, cache=None, **stats(null, real), **nkeys(bg + nc),
                                        **common)))
    return seq


def _compare(got, world, rank):
    assert len(got) == len(CASES)
    for case, calls in zip(CASES, got):
        assert calls == _expected(*case, world, rank), (case, world, rank)


def test_world1_call_sequence(monkeypatch):
    H.install(monkeypatch.setattr)
    _compare(_rank_body(0, 1, monkeypatch.setattr), 1, 0)


@pytest.mark.timeout(300)
def test_world2_call_sequence():
    for rank, got in enumerate(H.run_ranks(_rank_body, world=2)):
        _compare(got, 2, rank)
