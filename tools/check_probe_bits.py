"""Outputs of the four Linear + cross-entropy entries (clipk_linear_ce_* and clipk_linear_ce_tiled_*, through ops), for
a bitwise old-against-new comparison.

Run the same file in a checkout (built) of each commit, on the same GPU:
    (old checkout)  python tools/check_probe_bits.py old.pt
    (new checkout)  python tools/check_probe_bits.py new.pt old.pt      # exit status 1 if any tensor differs

Cases: every (M, K1, K2, C) of the SHAPES lists of tests/test_gpu_classifier.py and tests/test_gpu_classifier_wide.py
(the 64-class entries where C <= 64, the tiled entries at every shape), with the two sources as listed and in the other
form (one source of K1 + K2 columns, or K1 cut in two), fresh and accumulating onto seeded dW / dbias; one case per
family with labels outside [0, C); one tiled case of two backward slabs (C = 65536).  Every output of each case - lse,
tgt, pred, the logits where the entry has them, dW, dbias, dX1, dX2 - is compared with torch.equal (NaN tgt rows of the
out-of-range labels: as bit patterns).
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import clip_dplm_amd  # noqa: E402
from clip_dplm_amd import ops  # noqa: E402
from test_gpu_classifier import SHAPES as NARROW, make  # noqa: E402
from test_gpu_classifier_wide import SHAPES as WIDE  # noqa: E402

print("package from", os.path.dirname(clip_dplm_amd.__file__))
dev = torch.device("cuda:0")
out = {}


def case(tag, tiled, M, K1, K2, C, labels=None):
    x1, x2, w, b, lab = make(M, K1, K2, C, seed=4)
    lab = lab if labels is None else labels
    x1, x2, w, b, lab = (None if t is None else t.to(dev) for t in (x1, x2, w, b, lab))
    g = torch.tensor([0.75], device=dev)
    if tiled:
        fw = ops.linear_ce_tiled_fwd(x1, w, b, lab, x2)
        bwd = ops.linear_ce_tiled_bwd
    else:
        fw = ops.linear_ce_fwd(x1, w, b, lab, x2, want_logits=True)
        bwd = ops.linear_ce_bwd
    fresh = bwd(x1, w, b, lab, fw[0], g, x2=x2, want_dx=True, want_dx2=True)
    g0 = torch.Generator().manual_seed(5)
    dw0, db0 = torch.randn(C, K1 + K2, generator=g0).to(dev), torch.randn(C, generator=g0).to(dev)
    acc = bwd(x1, w, b, lab, fw[0], g, x2=x2, dw=dw0, dbias=db0, accumulate=True, want_dx=True, want_dx2=True)
    torch.cuda.synchronize()
    out[f"{tag}-{'tiled' if tiled else 'narrow'}-{M}x{K1}+{K2}x{C}"] = [
        None if t is None else t.cpu() for t in (*fw, *fresh, *acc)]


for M, K1, K2, C in dict.fromkeys(NARROW + WIDE):
    forms = [(K1, K2), (K1 + K2, 0) if K2 else ((K1 // 8) * 4, K1 - (K1 // 8) * 4)]
    for k1, k2 in forms:
        if k1 == 0:
            continue                                       # (K1 = 4 has no second form)
        for tiled in (False, True):
            if tiled or C <= 64:
                case("shape", tiled, M, k1, k2, C)
bad_labels = make(150, 64, 36, 11, seed=4)[4]
bad_labels[17], bad_labels[101], bad_labels[149] = 11, -1, 2 ** 40
case("badlabel", False, 150, 64, 36, 11, bad_labels)
bad_labels = make(150, 64, 36, 70, seed=4)[4]
bad_labels[17], bad_labels[101], bad_labels[149] = 70, -1, 2 ** 40
case("badlabel", True, 150, 64, 36, 70, bad_labels)
case("twoslabs", True, 577, 4, 0, 65536)


def same(x, y):
    if x is None or y is None:
        return x is None and y is None
    if x.dtype.is_floating_point:
        return torch.equal(x.view(torch.int32), y.view(torch.int32))
    return torch.equal(x, y)


torch.save(out, sys.argv[1])
print("wrote", len(out), "cases,", sum(t is not None for v in out.values() for t in v), "tensors")
if len(sys.argv) > 2:
    ref = torch.load(sys.argv[2])
    assert ref.keys() == out.keys(), "the two runs have different cases"
    bad = [k for k in ref if len(ref[k]) != len(out[k]) or not all(same(x, y) for x, y in zip(ref[k], out[k]))]
    for k in bad:                                          # which outputs, in the order (forward, fresh, accumulated)
        names = (["lse", "tgt", "pred"] + ["logits"] * (len(out[k]) == 12) + ["dW", "dbias", "dX1", "dX2"] * 2)
        print(k, [(i, nm, int((x != y).sum())) for i, (nm, x, y) in enumerate(zip(names, ref[k], out[k])) if not same(x, y)])
    n = sum(t is not None for v in ref.values() for t in v)
    print("compared", n, "tensors of", len(ref), "cases bitwise against", sys.argv[2], "-> differing:", bad)
    sys.exit(1 if bad else 0)
