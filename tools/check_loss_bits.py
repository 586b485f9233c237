"""Outputs of the loss entries that exist on both sides of a change, for a bitwise old-against-new comparison.

Run the same file in a checkout (built) of each commit, on the same GPU:
    (old checkout)  python tools/check_loss_bits.py old.pt
    (new checkout)  python tools/check_loss_bits.py new.pt old.pt      # exit status 1 if any case differs

Cases: clip_loss plain / class ids "mask" / "positive" + label smoothing / one class / hard-negative beta 0.5, and the
plain tri_modal_loss under unequal upstream gradients, at (B, P) = (100, 128), (300, 64), (1024, 512): loss, every
embedding gradient and d scale of each are compared with torch.equal.
"""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import clip_dplm_amd  # noqa: E402
from clip_dplm_amd.loss import clip_loss, tri_modal_loss  # noqa: E402

print("package from", os.path.dirname(clip_dplm_amd.__file__))
dev = torch.device("cuda:0")
out = {}
for B, P in ((100, 128), (300, 64), (1024, 512)):
    g = torch.Generator().manual_seed(B + P)
    ids = (torch.arange(B) // 4 + (1 << 40)).to(dev)
    for name, kw in (("plain", {}), ("mask", dict(class_ids=ids)), ("pos", dict(class_ids=ids, same_class="positive", label_smoothing=0.1)),
                     ("one", dict(class_ids=torch.zeros_like(ids))), ("beta", dict(class_ids=ids, hard_negative_beta=0.5))):
        a = F.normalize(torch.randn(B, P, generator=g), dim=-1).to(dev).requires_grad_(True)
        b = F.normalize(torch.randn(B, P, generator=g), dim=-1).to(dev).requires_grad_(True)
        s = torch.tensor(14.3, device=dev, requires_grad=True)
        l = clip_loss(a, b, s, **kw); l.backward()
        out[f"{name}-{B}x{P}"] = [t.detach().cpu() for t in (l, a.grad, b.grad, s.grad)]
        if name == "one":      # every row's denominator is its own key: the exact gradient is 0
            print(f"one class {B}x{P}: loss {l.item():.3e}, max |da| {a.grad.abs().max().item():.3e}, max |db| "
                  f"{b.grad.abs().max().item():.3e}")
    a, b, c = (F.normalize(torch.randn(B, P, generator=g), dim=-1).to(dev).requires_grad_(True) for _ in range(3))
    s = torch.tensor(14.3, device=dev, requires_grad=True)
    o = tri_modal_loss(a, b, c, s); (o["cell_pert_loss"] + 2 * o["pert_protein_loss"] + 0.5 * o["cell_protein_loss"]).backward()
    out[f"tri-{B}x{P}"] = [t.detach().cpu() for t in (o["loss"], a.grad, b.grad, c.grad, s.grad)]
torch.save(out, sys.argv[1])
if len(sys.argv) > 2:
    ref = torch.load(sys.argv[2])
    bad = [k for k in ref if not all(torch.equal(x, y) for x, y in zip(ref[k], out[k]))]
    print("compared", len(ref), "cases bitwise against", sys.argv[2], "-> differing:", bad)
    sys.exit(1 if bad else 0)
