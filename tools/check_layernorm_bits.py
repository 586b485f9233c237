"""Outputs of the LayerNorm family of csrc/rowwise.hip (and the two L2-normalise entries), through ops, for a bitwise
old-against-new comparison.

Run the same file in a checkout (built) of each commit, on the same GPU:
    (old checkout)  python tools/check_layernorm_bits.py old.pt
    (new checkout)  python tools/check_layernorm_bits.py new.pt old.pt      # exit status 1 if any tensor differs

Cases, from the lists of tests/test_gpu_layernorm.py: forward at WIDTHS x ROWS, f32 x with every activation and bf16 x
with None / gelu; backward at WIDTHS x ROWS for every entry of TRIPLES, without and with dropout, fresh and accumulating
onto seeded dgamma / dbeta; part_out + colreduce_entries; the second-order widths x activations; the mean-pool cases
(no mask, ragged, one empty sample) forward and backward; l2norm at 512 and 516 columns; the model widths 480, 640, 768,
1280 and 2560 at 1000 rows (forward both types, backward every triple with dropout).  Every output is compared as bit
patterns.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import clip_dplm_amd  # noqa: E402
from clip_dplm_amd import ops  # noqa: E402
import layernorm_ref as R  # noqa: E402
from test_gpu_layernorm import DT, ROWS, TRIPLES, WIDTHS, _mask  # noqa: E402

print("package from", os.path.dirname(clip_dplm_amd.__file__))
dev = torch.device("cuda:0")
out = {}
DROP = (0.1, 99)


def put(tag, tensors):
    torch.cuda.synchronize()
    out[tag] = [None if t is None else t.cpu() for t in tensors]


def cast(t, kind):
    return None if (t is None or kind is None) else t.to(DT[kind]).to(dev)


def fwd_case(rows, cols, xk, act, seed=50):
    x = R.randn((rows, cols), seed, 2.0, 0.5)
    gamma, beta = R.params(cols, seed + 1)
    xd, g, b = cast(x, xk), gamma.to(dev), beta.to(dev)
    put(f"fwd-{rows}x{cols}-{xk}-{act}", ops.layernorm_fwd(xd, g, b, 1e-5, act=act, want_f32=True, want_bf16=True))
    return xd, g, b


def bwd_case(rows, cols, triple, act, drops, seed=80):
    dyk, xk, addk = triple
    gamma, beta = R.params(cols, seed + 1)
    xd, g, b = cast(R.randn((rows, cols), seed, 2.0, 0.5), xk), gamma.to(dev), beta.to(dev)
    dy, add = cast(R.randn((rows, cols), seed + 2), dyk), cast(R.randn((rows, cols), seed + 3), addk)
    _, _, mean, rstd = ops.layernorm_fwd(xd, g, b, 1e-5, act=act)
    for drop in drops:
        kw = dict(act=act, dx_add=add, want_f32=True, want_bf16=True, dropout_bf16=drop)
        fresh = ops.layernorm_bwd(dy, xd, g, b, mean, rstd, **kw)
        dg0, db0 = R.randn((cols,), seed + 5).to(dev), R.randn((cols,), seed + 6).to(dev)
        acc = ops.layernorm_bwd(dy, xd, g, b, mean, rstd, dgamma=dg0, dbeta=db0, accumulate=True, **kw)
        put(f"bwd-{rows}x{cols}-{'-'.join(map(str, triple))}-{act}-drop{drop is not None}", (*fresh, *acc[:2], dg0, db0))
    return dy, xd, g, b, mean, rstd, add


for cols in WIDTHS:
    for rows in ROWS:
        for act in (None, "gelu", "celu", "softplus"):
            fwd_case(rows, cols, "f32", act)
        for act in (None, "gelu"):
            fwd_case(rows, cols, "bf16", act)
        for triple in TRIPLES:
            bwd_case(rows, cols, triple, "gelu" if rows % 2 else None, (None, DROP))

entries, keep = [], []
for i, (rows, cols) in enumerate([(9, 4), (5, 516), (9, 2048), (9, 2052)]):
    dy, xd, g, b, mean, rstd, add = bwd_case(rows, cols, TRIPLES[1], None, (), seed=150 + 10 * i)
    blocks, nfloat = ops.layernorm_bwd_partial_shape(rows, cols)
    part = torch.zeros(nfloat, device=dev)
    dx = ops.layernorm_bwd(dy, xd, g, b, mean, rstd, dx_add=add, part_out=part)[0]
    dgd, dbd = R.randn((cols,), 155 + 10 * i).to(dev), R.randn((cols,), 156 + 10 * i).to(dev)
    entries.append((part, blocks, cols, dgd, dbd))
    keep.append((rows, cols, dx, part, dgd, dbd))
ops.colreduce_entries(entries)
for rows, cols, dx, part, dgd, dbd in keep:
    put(f"deferred-{rows}x{cols}", (dx, part[:ops.layernorm_bwd_partial_shape(rows, cols)[0] * 2 * cols], dgd, dbd))

for cols in (4, 516, 1028, 2048):
    for act in (None, "celu", "softplus"):
        for rows in (1, 5):
            a, dy, g = R.randn((rows, cols), 160, 1.5, 0.3), R.randn((rows, cols), 161), R.randn((rows, cols), 162)
            gamma, beta = R.params(cols, 163)
            ad, dyd, gd, gmd, btd = (t.to(dev) for t in (a, dy, g, gamma, beta))
            _, _, mean, rstd = ops.layernorm_fwd(ad, gmd, btd, 1e-5, act=act)
            fresh = ops.layernorm_bwd2(gd, dyd, ad, gmd, btd, mean, rstd, act=act)
            dg0, db0 = R.randn((cols,), 164).to(dev), R.randn((cols,), 165).to(dev)
            ops.layernorm_bwd2(gd, dyd, ad, gmd, btd, mean, rstd, act=act, dgamma=dg0, dbeta=db0, accumulate=True)
            put(f"bwd2-{rows}x{cols}-{act}", (*fresh, dg0, db0))

for cols in (4, 516, 1028, 4092):
    for B, L in ((1, 1), (3, 5), (2, 9)):
        for xk in ("f32", "bf16"):
            x = R.randn((B * L, cols), 170, 2.0, 0.5)
            gamma, beta = R.params(cols, 171)
            xd, g, b, dpd = cast(x, xk), gamma.to(dev), beta.to(dev), R.randn((B, cols), 172).to(dev)
            for kind in ("none", "ragged", "empty"):
                mask = _mask(kind, B, L)
                pooled, mean, rstd, wrow = ops.layernorm_meanpool_fwd(xd, g, b, 1e-5, B, L, None if mask is None else mask.to(dev))
                bw = ops.layernorm_meanpool_bwd(dpd, wrow, xd, g, mean, rstd, B, L, want_f32=True, want_bf16=True)
                put(f"pool-{B}x{L}x{cols}-{xk}-{kind}", (pooled, mean, rstd, wrow, *bw))

for cols in (512, 516):
    x, dy = R.randn((37, cols), 180).to(dev), R.randn((37, cols), 181).to(dev)
    y, n = ops.l2norm_fwd(x)
    put(f"l2norm-{cols}", (y, n, ops.l2norm_bwd(dy, y, n)))

for cols in (480, 640, 768, 1280, 2560):
    for xk in ("f32", "bf16"):
        fwd_case(1000, cols, xk, "gelu", seed=190)
    for triple in TRIPLES:
        bwd_case(1000, cols, triple, None, (DROP,), seed=200)


def same(x, y):
    if x is None or y is None:
        return x is None and y is None
    if x.dtype != y.dtype or x.shape != y.shape:
        return False
    view = {torch.float32: torch.int32, torch.bfloat16: torch.int16}.get(x.dtype)
    return torch.equal(x.view(view), y.view(view)) if view else torch.equal(x, y)


torch.save(out, sys.argv[1])
print("wrote", len(out), "cases,", sum(t is not None for v in out.values() for t in v), "tensors")
if len(sys.argv) > 2:
    ref = torch.load(sys.argv[2])
    assert ref.keys() == out.keys(), "the two runs have different cases"
    bad = [k for k in ref if len(ref[k]) != len(out[k]) or not all(same(x, y) for x, y in zip(ref[k], out[k]))]
    for k in bad:                                          # which outputs of the case, by position
        print(k, [i for i, (x, y) in enumerate(zip(ref[k], out[k])) if not same(x, y)])
    n = sum(t is not None for v in ref.values() for t in v)
    print("compared", n, "tensors of", len(ref), "cases bitwise against", sys.argv[2], "-> differing:", bad)
    sys.exit(1 if bad else 0)
