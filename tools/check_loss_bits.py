"""Outputs of the loss entries that exist on both sides of a change, for a bitwise old-against-new comparison.

Run the same file in a checkout (built) of each commit, on the same GPU:
    (old checkout)  python tools/check_loss_bits.py old.pt
    (new checkout)  python tools/check_loss_bits.py new.pt old.pt      # exit status 1 if any case differs

Cases, at (B, P) = (100, 128), (300, 64), (1024, 512) and, for partial tiles, (63, 4), (65, 60), (200, 512):
  * clip_loss plain / class ids "mask" / "positive" + label smoothing / one class / hard-negative beta 0.5;
  * tri_modal_loss under unequal upstream gradients: plain, with class ids, with hard_negative_beta (the batched
    class-aware and hard-negative launches);
  * cache keys: contrastive_loss with a queue of 50 rows, plain and with hard_negative_beta; clip_loss with class ids and a
    cache of 50 rows;
  * key splits: at B = 200 a queue / cache of 19034 rows gives 301 key tiles, 101 splits of 3 tiles, the last of 1.
Loss, every embedding gradient and d scale of each are compared as bit patterns (torch.equal on the int32 views, so that
NaNs and signed zeros count too).
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import clip_dplm_amd  # noqa: E402
from clip_dplm_amd.loss import clip_loss, contrastive_loss, tri_modal_loss  # noqa: E402

print("package from", os.path.dirname(clip_dplm_amd.__file__))
dev = torch.device("cuda:0")
out = {}


def unit(g, *shape):
    return F.normalize(torch.randn(*shape, generator=g), dim=-1).to(dev)


def keep(key, loss, *leaves):
    out[key] = [t.detach().cpu() for t in (loss, *(x.grad for x in leaves))]


for B, P in ((100, 128), (300, 64), (1024, 512), (63, 4), (65, 60), (200, 512)):
    g = torch.Generator().manual_seed(B + P)
    ids = (torch.arange(B) // 4 + (1 << 40)).to(dev)
    for name, kw in (("plain", {}), ("mask", dict(class_ids=ids)), ("pos", dict(class_ids=ids, same_class="positive", label_smoothing=0.1)),
                     ("one", dict(class_ids=torch.zeros_like(ids))), ("beta", dict(class_ids=ids, hard_negative_beta=0.5))):
        a = unit(g, B, P).requires_grad_(True)
        b = unit(g, B, P).requires_grad_(True)
        s = torch.tensor(14.3, device=dev, requires_grad=True)
        l = clip_loss(a, b, s, **kw); l.backward()
        keep(f"{name}-{B}x{P}", l, a, b, s)
        if name == "one":      # every row's denominator is its own key: the exact gradient is 0
            print(f"one class {B}x{P}: loss {l.item():.3e}, max |da| {a.grad.abs().max().item():.3e}, max |db| "
                  f"{b.grad.abs().max().item():.3e}")
    for name, kw in (("tri", {}), ("tri-ids", dict(class_ids=ids)), ("tri-beta", dict(class_ids=ids, hard_negative_beta=0.5))):
        a, b, c = (unit(g, B, P).requires_grad_(True) for _ in range(3))
        s = torch.tensor(14.3, device=dev, requires_grad=True)
        o = tri_modal_loss(a, b, c, s, **kw)
        (o["cell_pert_loss"] + 2 * o["pert_protein_loss"] + 0.5 * o["cell_protein_loss"]).backward()
        keep(f"{name}-{B}x{P}", o["loss"], a, b, c, s)
    for Q in (50, 19034) if B == 200 else (50,):
        queue = unit(g, Q, P)
        for name, kw in (("queue", {}), ("queue-beta", dict(hard_negative_beta=0.5))):
            a, b = (unit(g, B, P).requires_grad_(True) for _ in range(2))
            l = contrastive_loss(a, b, 0.07, queue=queue, **kw); l.backward()
            keep(f"{name}{Q}-{B}x{P}", l, a, b)
        a, b = (unit(g, B, P).requires_grad_(True) for _ in range(2))
        s = torch.tensor(14.3, device=dev, requires_grad=True)
        l = clip_loss(a, b, s, cache=queue, class_ids=ids, label_smoothing=0.1); l.backward()
        keep(f"cache-mask{Q}-{B}x{P}", l, a, b, s)
torch.save(out, sys.argv[1])


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


if len(sys.argv) > 2:
    ref = torch.load(sys.argv[2])
    bad = [k for k in ref if k not in out or len(ref[k]) != len(out[k])
           or not all(torch.equal(bits(x), bits(y)) for x, y in zip(ref[k], out[k]))]
    print("compared", len(ref), "cases,", sum(len(v) for v in ref.values()), "tensors,",
          sum(t.numel() for v in ref.values() for t in v), "elements bitwise against", sys.argv[2], "-> differing:", bad)
    sys.exit(1 if bad else 0)
