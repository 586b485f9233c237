"""Outputs of the bf16 Linear kernels (clipk_gemm_nt: csrc/gemm_nt.hip "v1", gemm_nt_v2.hip, gemm_nt_v3.hip, gemm_nt_v4.hip),
through ops, for a bitwise old-against-new comparison.

Run the same file in a checkout (built) of each commit, on the same GPU:
    (old checkout)  python tools/check_gemm_bits.py old.pt
    (new checkout)  python tools/check_gemm_bits.py new.pt old.pt      # exit status 1 if any tensor differs

Cases, from the lists of tests/test_gpu_gemm.py: V1_SHAPES x families x NO_U8 under gemm_kernel = 1; V2_SHAPES x families x
REQUESTS x gemm_epi_generic 0 / 1 under gemm_kernel = 2; V34_CASES x REQUESTS x 0 / 1 for gemm_kernel = 3 and 4 with
gemm_nwg = 8; the three v2 option instantiations (gemm_bm, gemm_stages); one call per kernel with every operand a column
slice of a wider buffer.  The dropout requests are seeded and in the lists.  The v1 outputs are kept whole (a difference
is reported in ulps); of the others the file keeps each tensor's dtype, shape and SHA-256 over its bytes.
"""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import clip_dplm_amd  # noqa: E402
from clip_dplm_amd import ops  # noqa: E402
import gemm_ref as R  # noqa: E402
import test_gpu_gemm as G  # noqa: E402

print("package from", os.path.dirname(clip_dplm_amd.__file__))
dev = torch.device("cuda:0")
out = {}


def digest(t):
    t = t.contiguous()
    return (str(t.dtype), tuple(t.shape), hashlib.sha256(t.view(torch.uint8).numpy().tobytes()).hexdigest())


def put(tag, tensors, whole=False):
    torch.cuda.synchronize()
    out[tag] = [None if t is None else (t.cpu() if whole else digest(t.cpu())) for t in tensors]


def options(**kw):
    ops.reset_options()
    for k, v in kw.items():
        ops.set_option(k, v)


for M, N, K in G.V1_SHAPES:
    for fam in R.FAMILIES:
        options(gemm_kernel=1)
        for name in G.NO_U8:
            put(f"v1-{M}x{N}x{K}-{fam}-{name}", G._run(G._case(fam, M, N, K), name, ops, dev), whole=True)
for M, N, K in G.V2_SHAPES:
    for fam in R.FAMILIES:
        for generic in (0, 1):
            options(gemm_kernel=2, gemm_epi_generic=generic)
            for name in G.REQUESTS:
                put(f"v2-{M}x{N}x{K}-{fam}-{name}-g{generic}", G._run(G._case(fam, M, N, K), name, ops, dev))
for shape, fam in G.V34_CASES:
    for kernel in ("v3", "v4"):
        for generic in (0, 1):
            options(gemm_kernel=G.KERNEL[kernel], gemm_nwg=8, gemm_epi_generic=generic)
            for name in G.REQUESTS:
                put(f"{kernel}-{'x'.join(map(str, shape))}-{fam}-{name}-g{generic}", G._run(G._case(fam, *shape), name, ops, dev))
for bm, stages in ((256, 1), (256, 2), (0, 2)):
    for M in (1, 255, 257, 600):
        for K in (64, 96, 480):
            options(gemm_kernel=2, gemm_bm=bm, gemm_stages=stages)
            put(f"v2opt-{bm}-{stages}-{M}x136x{K}", G._run(G._case("a", M, 136, K), "relu_res32_pre", ops, dev))
# leading dimensions: lda = K + 8, ldb = K + 16, ldc = N + 8, ldp = N + 16, ldd = N + 24, ldr = N + 32, the run-time
# epilogue with every operand at once and the plain mode
for kernel, (M, N, K) in (("v1", (77, 136, 120)), ("v2", (129, 136, 96)), ("v3", (2072, 264, 160)), ("v4", (2072, 264, 160))):
    options(gemm_kernel=G.KERNEL[kernel], **({"gemm_nwg": 8} if kernel in ("v3", "v4") else {}))
    c = G._case("a", M, N, K)
    a_w, b_w = G._wide(c.a.to(G.BF), 8, dev, float("nan"))[1], G._wide(c.b.to(G.BF), 16, dev, float("nan"))[1]
    bias = c.bias.to(dev)
    for name, act, odt, res, pdt, aux, dact in (("generic_all", "relu", torch.float32, c.res, G.BF, c.aux.to(G.BF), "relu"),
                                                ("plain", None, G.BF, None, None, None, None)):
        cv = G._out(M, N, 8, odt, dev)[1]
        pv = None if pdt is None else G._out(M, N, 16, pdt, dev)[1]
        av = None if aux is None else G._wide(aux, 24, dev, float("nan"))[1]
        rv = None if res is None else G._wide(res, 32, dev, float("nan"))[1]
        rc = G._gemm_raw(ops, a_w, b_w, cv, bias=bias, act=act, pre=pv, aux=av, dact=dact, res=rv)
        assert rc == 0, (kernel, name, rc)
        put(f"ld-{kernel}-{name}", (cv, pv), whole=kernel == "v1")
ops.reset_options()


def same(x, y):
    if x is None or y is None or not torch.is_tensor(x):
        return x == y
    if x.dtype != y.dtype or x.shape != y.shape:
        return False
    view = {torch.float32: torch.int32, torch.bfloat16: torch.int16}.get(x.dtype)
    return torch.equal(x.view(view), y.view(view)) if view else torch.equal(x, y)


def ulps(x, y):
    """Largest distance in units of the last place between two same-typed float tensors (bit patterns as ordered integers)."""
    view = {torch.float32: torch.int32, torch.bfloat16: torch.int16}.get(x.dtype)
    if view is None or x.shape != y.shape:
        return "n/a"
    key = lambda t: (lambda i: torch.where(i < 0, -(i & (2 ** 31 - 1 if view == torch.int32 else 2 ** 15 - 1)), i))(t.view(view).to(torch.int64))
    return int((key(x) - key(y)).abs().max())


torch.save(out, sys.argv[1])
print("wrote", len(out), "cases,", sum(t is not None for v in out.values() for t in v), "tensors")
if len(sys.argv) > 2:
    ref = torch.load(sys.argv[2], weights_only=False)
    assert ref.keys() == out.keys(), "the two runs have different cases"
    bad = [k for k in ref if len(ref[k]) != len(out[k]) or not all(same(x, y) for x, y in zip(ref[k], out[k]))]
    for k in bad:                                          # which outputs of the case, by position (v1: and by how many ulps)
        print(k, [(i, ulps(x, y) if torch.is_tensor(x) and torch.is_tensor(y) else "digest")
                  for i, (x, y) in enumerate(zip(ref[k], out[k])) if not same(x, y)])
    n = sum(t is not None for v in ref.values() for t in v)
    print("compared", n, "tensors of", len(ref), "cases bitwise against", sys.argv[2], "-> differing:", bad)
    sys.exit(1 if bad else 0)
