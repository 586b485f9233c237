"""Class-aware / hard-negative tri-modal loss: the batched path against three clip_loss calls.

What is timed: the loss forward + backward on the embeddings only (leaves [B, P] x 3 and the scale), device events
around `iters` back-to-back eager iterations, warm.  Yardstick: three `clip_loss(..., class_ids=ids)` calls on the same
tensors, summed.  The two paths alternate, `rounds` times; a figure is the median over the rounds and its spread is
max - min over the rounds.

    python tools/bench_trimodal_variants.py [--rounds 7] [--iters 200] [--out FILE.json] [--yardstick-only]

--yardstick-only times the three-call path alone: it needs nothing this tool's own commit added, so a copy of this file
under tools/ of a checkout of an older commit times that commit's kernels.  Inputs are built the way a PerturbAtlas
batch is: four cells per perturbation.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(32, 128), (32, 512), (256, 128), (256, 512), (1024, 128), (1024, 512)]
VARIANTS = {"mask": dict(same_class="mask"), "beta0.5": dict(hard_negative_beta=0.5)}


def inputs(B, P, dev):
    g = torch.Generator().manual_seed(B * 1000 + P)
    ids = torch.arange(B) // 4 + (1 << 40)
    ncls = (B + 3) // 4
    r = lambda *s: torch.randn(*s, generator=g)
    cell = F.normalize(r(B, P), dim=-1)
    pert = F.normalize(r(ncls, P)[ids - (1 << 40)] + 0.05 * r(B, P), dim=-1)
    prot = F.normalize(r(ncls, P)[ids - (1 << 40)] + 0.05 * r(B, P), dim=-1)
    leaves = [t.to(dev).requires_grad_(True) for t in (cell, pert, prot)]
    return leaves, torch.tensor(14.3, device=dev, requires_grad=True), ids.to(dev)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return 1e3 * s.elapsed_time(e) / iters                   # us per iteration


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--yardstick-only", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    from clip_dplm_amd.loss import clip_loss
    if not a.yardstick_only:
        from clip_dplm_amd.loss import tri_modal_loss
    dev = torch.device("cuda:0")
    rows = []
    for name, kw in VARIANTS.items():
        for B, P in SHAPES:
            (cell, pert, prot), s, ids = inputs(B, P, dev)
            leaves = (cell, pert, prot, s)

            def three():
                for t in leaves:
                    t.grad = None
                loss = (clip_loss(cell, pert, s, class_ids=ids, **kw) + clip_loss(cell, prot, s, class_ids=ids, **kw)
                        + clip_loss(pert, prot, s, class_ids=ids, **kw))
                loss.backward()
                return loss

            def batched():
                for t in leaves:
                    t.grad = None
                loss = tri_modal_loss(cell, pert, prot, s, class_ids=ids, **kw)["loss"]
                loss.backward()
                return loss
            paths = {"three_calls": three} if a.yardstick_only else {"three_calls": three, "batched": batched}
            vals = {}
            for k, fn in paths.items():
                for _ in range(20):
                    out = fn()
                vals[k] = out.item()
            us = {k: [] for k in paths}
            for _ in range(a.rounds):
                for k, fn in paths.items():                  # alternating
                    us[k].append(timed(fn, a.iters))
            row = {"variant": name, "B": B, "P": P}
            for k in paths:
                row[k + "_us"] = round(statistics.median(us[k]), 2)
                row[k + "_spread_us"] = round(max(us[k]) - min(us[k]), 2)
                row[k + "_loss"] = vals[k]
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
