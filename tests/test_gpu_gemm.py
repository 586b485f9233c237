"""GPU: the bf16 Linear kernels (clipk_gemm_nt: csrc/gemm_nt.hip "v1", gemm_nt_v2.hip, gemm_nt_v3.hip, gemm_nt_v4.hip and the
shared csrc/gemm_epilogue.h) and the two weight-gradient kernels (clipk_gemm_wgrad: csrc/gemm_wgrad.hip 128 x 128,
gemm_wgrad_v3.hip 256 x 256 in both schedules) against the plain f64 references and the DERIVED bounds of tests/gemm_ref.py
(pinned on the CPU by tests/test_gemm_ref_host.py), branch by branch.  Inputs come from seeded CPU generators and go to the
device; references are f64 on the CPU; nothing is masked out or skipped.  Families (a) N(0,1) x N(0,0.05^2), (b) rows
scaled by 2^+-6, (d) residual offset 1000 are compared with the bound; family (c), small integers, EXACTLY (bf16 outputs:
the one rounding of the integer reference) wherever no GELU is involved.  Shapes are the smallest that reach a branch; the
persistent kernels walk several tiles per workgroup through option gemm_nwg = 8, not through workload-sized M.

What the code promises exactly is compared bit for bit - each test's docstring names the lines it rests on:
  bf16 output = RNE of the f32 output of the same request; specialised epilogue mode = run-time epilogue (all modes
  but the two GELU forward ones, whose specialised body evaluates x Phi(x) and the run-time one fma(|x| / 2, erf, x / 2):
  those two are held to the f64 bound instead, their bf16 pre-activation output still bit for bit); rows independent of
  the batch; epi_nt = 1 = epi_nt = 0; results independent of gemm_nwg, of the v2 instantiation (gemm_bm, gemm_stages: one
  K order), of leading dimensions; weight gradients independent of want_bias, reproducible, and on family (c)
  independent of wgrad_splits (on the others the split changes the summation order: the f64 bound).

Worst |error| / bound over this file, measured on an MI355X against the f64 reference (a ratio above 1 fails; the file
prints them at the end of a run with -s):
                    v1       v2       v3       v4                             128 x 128   256 x 256
  product         0.0120   0.0070   0.0055   0.0055        dW, db              0.1114      0.0008
  f32 outputs     0.9255   0.9218   0.8498   0.8498        accumulated         0.9992      0.0600
  bf16 outputs    1.0000   1.0000   1.0000   1.0000
  8-bit codes       -      0.9996   0.9996   0.9996
"product" is the bare f32 product against K u |A| |B|^T alone: the main loops use about a hundredth of it.  The other rows sit
near 1 by construction, not for want of headroom: where one final rounding dominates (a bf16 store, the nearest code level,
an f32 add of a bias or a preloaded dW far larger than the product) the bound IS that rounding's half ulp, and a correctly
rounded result reaches it (1.0000: an exact tie).
"""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import elementwise_ref as E
import gemm_ref as R

pytestmark = pytest.mark.gpu

F64 = torch.float64
BF = torch.bfloat16
BAD_ARG, UNSUPPORTED = -1, -2           # include/clipk.h
GUARD = 8
KERNEL = {"v1": 1, "v2": 2, "v3": 3, "v4": 4}
RATIOS = {}                             # kernel family and output type -> worst |error| / bound seen in this run


def _ops():
    from clip_dplm_amd import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    print("\nworst |error| / bound per kernel family: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(RATIOS.items())))


def _within(got, ref, bound, key, what=""):
    """|got - ref| <= bound per element (a bound of 0 where the reference is an exact 0); records the worst ratio."""
    got = got.detach().cpu().to(F64)
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max())
    print(f"{what}: worst |err| / bound = {ratio:.4f}")
    RATIOS[key] = max(RATIOS.get(key, 0.0), ratio if bool((err <= bound).all()) else max(ratio, 1.0001))
    assert (err <= bound).all(), f"{what}: worst |err| / bound = {ratio:.3f}"


def _bits(t):
    t = t.detach().cpu()
    if t.dtype == BF:
        return E.bf16_bits(t)
    if t.dtype == torch.float32:
        return E.f32_bits(t)
    return t.contiguous().numpy()


def _same(a, b):
    """Bitwise equality (NaN-safe, -0 != +0)."""
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _is_rne(x16, x32):
    return np.array_equal(E.bf16_bits(x16.cpu()), E.bf16_rne_bits(E.f32_bits(x32.cpu())))


def _exact(got, ref, what):
    """Family (c): the f32 result IS the integer reference; a bf16 result is its one rounding."""
    got = got.detach().cpu()
    want = E.round_f64_to_bf16(ref) if got.dtype == BF else ref
    assert torch.equal(got.to(F64), want), f"{what}: {int((got.to(F64) != want).sum())} elements differ from the exact reference"


# ------------------------------------------------------------------------------------------------ forward: requests
# Every epilogue request the models make (encoders.py, functional.py) and every row of gemm_epilogue.h epi_mode_for but the
# rotations.  Fields: bias, act, out (f32: f32 output), res (residual type), pre (pre-activation output), u8 (8-bit aux),
# dact (act' of aux), alpha, drop.  `mode`: what epi_mode_for answers (documentation; "generic" = EPI_GENERIC).
def _req(mode, bias=False, act=None, out="bf16", res=None, pre=False, u8=False, dact=None, alpha=1.0, drop=False):
    return SimpleNamespace(mode=mode, bias=bias, act=act, out=out, res=res, pre=pre, u8=u8, dact=dact, alpha=alpha, drop=drop)


REQUESTS = {
    "plain": _req("PLAIN", bias=True),
    "plain_nb": _req("PLAIN_NB"),
    "res32": _req("RES32", bias=True, res="f32", out="f32"),
    "res16": _req("RES16", bias=True, res="bf16", out="f32"),
    "pres16": _req("PRES16", res="bf16"),
    "gelu_pre": _req("GELU_PRE", bias=True, act="gelu", pre=True),
    "gelu_nopre": _req("GELU_PRE", bias=True, act="gelu"),           # the zero-length descriptor for u
    "dgelu": _req("DGELU", dact="gelu"),
    "gelu_d8": _req("GELU_D8", bias=True, act="gelu", pre=True, u8=True),
    "dgelu8": _req("DGELU8", dact="gelu8", u8=True),
    "relu": _req("generic", bias=True, act="relu"),
    "f32": _req("generic", bias=True, out="f32"),
    "f32_nb": _req("generic", out="f32"),                              # the bare product: |error| against K u |A| |B|^T alone
    "f32_pre": _req("generic", bias=True, out="f32", pre=True),
    "bias_pres16": _req("generic", bias=True, res="bf16"),
    "drelu": _req("generic", dact="relu"),
    "alpha": _req("generic", bias=True, alpha=0.5),
    "dropout": _req("generic", bias=True, act="relu", drop=True),
    # the models' remaining combinations (encoders.py _rna_layer_fwd / _rna_layer_bwd, functional.py linear)
    "res32_nb": _req("RES32", res="f32", out="f32"),                   # input gradient + f32 residual-path gradient
    "drop_res32": _req("generic", bias=True, res="f32", out="f32", drop=True),        # dropout(Linear) + residual
    "gelu_pre_drop": _req("generic", bias=True, act="gelu", pre=True, drop=True),     # FFN with dropout
    "dgelu_drop": _req("generic", dact="gelu", drop=True),                             # x mask x GELU'(u)
    "relu_pre": _req("generic", bias=True, act="relu", pre=True),
    "relu_res32_pre": _req("generic", bias=True, act="relu", res="f32", out="f32", pre=True),
}
NO_U8 = [n for n, q in REQUESTS.items() if not q.u8]                 # what the generic-K kernel accepts
BITWISE_MODES = ["plain", "plain_nb", "res32", "res16", "pres16", "dgelu", "dgelu8"]
DROP_SEED = 77


@functools.lru_cache(maxsize=4)
def _case(fam, M, N, K):
    """CPU inputs of one (family, shape), the f64 product and |A| |B|^T, computed once and shared."""
    a, b = R.operands(fam, M, N, K, 100)
    bias, res, aux = R.epilogue_operands(fam, M, N, 200)
    codes = torch.randint(0, 256, (M, N), generator=torch.Generator().manual_seed(300), dtype=torch.int64).to(torch.uint8)
    a64, b64 = a.to(F64), b.to(F64)
    return SimpleNamespace(fam=fam, M=M, N=N, K=K, a=a, b=b, bias=bias, res=res, res16=R.bf16(res), aux=aux, codes=codes,
                           product=(a64 @ b64.t(), a64.abs() @ b64.abs().t()), dev={}, keep=None,
                           drop_p=0.5 if fam == "c" else 0.1)      # p = 1/2: the survivors' scale 2 is exact on (c)


def _dev(c, name, dev):
    """Device copy of a case's operand (bf16 where the kernel takes bf16), made once."""
    if name not in c.dev:
        t = getattr(c, name)
        c.dev[name] = (t.to(BF) if name in ("a", "b", "aux", "res16") else t).to(dev)
    return c.dev[name]


def _keep(c, ops, dev):
    """The epilogue's keep mask, from ops.dropout_f32 with the same (p, seed) over the same element index m N + n
    (test_gpu_kernels.py test_dropout_f32_kernel_matches_the_epilogue_mask), and the f32 survivors' scale."""
    if c.keep is None:
        y = ops.dropout_f32(torch.ones(c.M, c.N, device=dev), (c.drop_p, DROP_SEED))
        c.keep = ((y != 0).to(torch.float32).cpu(), np.float32(1.0) / (np.float32(1.0) - np.float32(c.drop_p)))
    return c.keep


def _kwargs(c, q, dev, rows=None):
    """ops.gemm_nt keyword arguments of request q on case c (the first `rows` rows of it)."""
    m = c.M if rows is None else rows
    kw = dict(out_dtype=torch.float32 if q.out == "f32" else BF, act=q.act, alpha=q.alpha, out_preact=q.pre,
              aux_u8=q.u8 and q.pre)
    if q.bias:
        kw["bias"] = _dev(c, "bias", dev)
    if q.res:
        kw["residual"] = _dev(c, "res" if q.res == "f32" else "res16", dev)[:m]
    if q.dact:
        kw["dact_aux"] = _dev(c, "codes" if q.dact == "gelu8" else "aux", dev)[:m]
        kw["dact"] = "gelu" if q.dact == "gelu8" else q.dact
    if q.drop:
        kw["dropout"] = (c.drop_p, DROP_SEED)
    return kw


def _run(c, name, ops, dev, rows=None):
    """(out, pre or None) of request `name` on the device."""
    q = REQUESTS[name]
    m = c.M if rows is None else rows
    r = ops.gemm_nt(_dev(c, "a", dev)[:m], _dev(c, "b", dev), **_kwargs(c, q, dev, rows))
    return r if q.pre else (r, None)


def _reference(c, q, ops, dev):
    return R.linear(c.a, c.b, bias=c.bias if q.bias else None, act=q.act, alpha=q.alpha,
                    residual=None if not q.res else (c.res if q.res == "f32" else c.res16),
                    dact_aux=None if not q.dact else (c.codes if q.dact == "gelu8" else c.aux), dact=q.dact,
                    keep=_keep(c, ops, dev) if q.drop else None, want_bounds=True, product=c.product)


def _verify(c, name, out, pre, ops, dev, key):
    """One request's outputs against gemm_ref: the bound on families (a), (b), (d), exactly on (c) where no GELU is in it."""
    q = REQUESTS[name]
    ref, rpre, e, e_pre = _reference(c, q, ops, dev)
    what = f"{key} {name} ({c.fam}) {c.M}x{c.N}x{c.K}"
    assert out.dtype == (torch.float32 if q.out == "f32" else BF) and out.shape == (c.M, c.N)
    exact = c.fam == "c" and "gelu" not in (q.act, q.dact) and q.dact != "gelu8"
    if exact:
        _exact(out, ref, what)
    else:
        _within(out, ref, e if q.out == "f32" else R.bf16_bound(ref, e), f"{key} {'product' if name == 'f32_nb' else q.out}", what)
    if pre is None:
        return
    if q.u8:                                                           # 8-bit GELU' codes of the pre-activation
        assert pre.dtype == torch.uint8 and pre.shape == (c.M, c.N)
        _within(R.gelu8_decode(pre.cpu()), E.act_grad(rpre, "gelu"), R.gelu_code_bound(rpre, e_pre), key + " codes", what + " codes")
    elif c.fam == "c":
        _exact(pre, rpre, what + " pre")
    else:
        _within(pre, rpre, R.bf16_bound(rpre, e_pre), key + " bf16", what + " pre")


def _forward_all(c, names, ops, dev, key):
    for name in names:
        out, pre = _run(c, name, ops, dev)
        _verify(c, name, out, pre, ops, dev, key)


# ------------------------------------------------------------------------------------------------ forward: v1
# gemm_nt.hip: M = 1 (every staging row clamped to row 0), 77 (one ragged tile), 129 (a second tile with one row);
# N = 8 (one 8-column piece), 136 (a second n-tile with one piece); K = 8, 40 (one K-step, ksub = 1 / 2), 72 (two steps,
# ksub = 1 on the last), 120 (two steps, the zero-selected chunk of the tail); K = 64 reaches it through gemm_kernel = 1 only
V1_SHAPES = [(1, 8, 8), (77, 136, 40), (129, 8, 72), (129, 136, 120), (77, 136, 64)]


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("M,N,K", V1_SHAPES)
def test_v1_generic_k_kernel_private_epilogue(dev, kopt, M, N, K, fam):
    """gemm_nt.hip gemm_nt_kernel: the generic-K kernel's PRIVATE epilogue (lines 132-219) - bias, activation, pre-activation
    out, act'(aux), f32 and bf16 residual, dropout, alpha, f32 out - which the first-generation tests reach with the plain
    product only; natural K % 32 != 0 and (K = 64) option gemm_kernel = 1."""
    ops = _ops()
    kopt("gemm_kernel", 1)
    _forward_all(_case(fam, M, N, K), NO_U8, ops, dev, "v1")


# ------------------------------------------------------------------------------------------------ forward: v2
# gemm_nt_v2.hip <128, 1>: K = 32 (one step, ksub = 1 on the only step), 64 (one full step), 96 (two steps, ksub = 1 on the
# last), 160; M = 1 and 15 (every staging row clamped to row M - 1), 128, 129, 300; N = 8, 128, 136, 264
V2_SHAPES = [(1, 8, 32), (15, 136, 64), (128, 128, 96), (129, 264, 160), (300, 136, 96)]


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("M,N,K", V2_SHAPES)
def test_v2_every_epilogue_request(dev, kopt, M, N, K, fam, generic):
    """gemm_nt_v2_kernel<128, 1, MODE>: every specialised mode of gemm_epilogue.h (generic = 0) and the run-time epilogue
    for the same requests (option gemm_epi_generic = 1), plus the requests epi_mode_for sends to EPI_GENERIC (relu, f32 out
    + pre-activation, bias + bf16 residual + bf16 out, act' = relu, alpha = 0.5, dropout), at small M and one / two K-steps."""
    ops = _ops()
    kopt("gemm_kernel", 2)
    kopt("gemm_epi_generic", generic)
    _forward_all(_case(fam, M, N, K), list(REQUESTS), ops, dev, "v2")


# ------------------------------------------------------------------------------------------------ forward: v3 / v4
# K = 160 (nk = 3 with the K % 64 = 32 tail), 192 (nk = 3), 224 (nk = 4 with the tail: the first steady-state K-tile of v3),
# 256, 480; 8 workgroups over 16 .. 27 (v3) / 32 .. 51 (v4) tiles: each walks 2 - 7 tiles (next-tile prefetch, the
# `first` / VMCNT_PLUS waits, the generic-mode drain)
V34_SHAPES = [(2048, 264, 160), (2072, 520, 192), (2048, 256, 224), (2072, 264, 256), (2072, 520, 480)]
V34_CASES = [(s, f) for s in V34_SHAPES for f in ("a", "c")] + [(s, f) for s in (V34_SHAPES[1], V34_SHAPES[4]) for f in ("b", "d")]


@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("kernel", ["v3", "v4"])
@pytest.mark.parametrize("shape,fam", V34_CASES)
def test_v3_v4_persistent_kernels_walk_several_tiles(dev, kopt, shape, fam, kernel, generic):
    """gemm_nt_v3.hip / gemm_nt_v4.hip with gemm_nwg = 8 (gemm_nt_persistent.h:98-99): every workgroup walks several
    tiles at M = 2048 / 2072 - the prefetch of the next tile under the epilogue, vmcnt(8 + NS) / vmcnt(6 + NS) after a
    specialised epilogue's stores, the drain after the run-time one - for every epilogue request, with K = 160 (the
    smallest the dispatcher admits: nk = 3 with the half K-tile) upwards."""
    ops = _ops()
    kopt("gemm_kernel", KERNEL[kernel])
    kopt("gemm_nwg", 8)
    kopt("gemm_epi_generic", generic)
    _forward_all(_case(fam, *shape), list(REQUESTS), ops, dev, kernel)


@pytest.mark.parametrize("kernel", ["v3", "v4"])
def test_v3_v4_one_tile_per_workgroup_and_independence_of_nwg(dev, kopt, kernel):
    """gemm_nwg = 0 (the default: one workgroup per CU, here exactly one tile each - the loop of gemm_nt_v3.hip:181-220 leaves at
    its first `if (!more) break`) against the bound, and BITWISE equal to gemm_nwg = 8 and 16: a tile's arithmetic does not
    depend on which workgroup computes it or on what it computed before (acc is zeroed per tile, gemm_nt_v3.hip:188-191)."""
    ops = _ops()
    kopt("gemm_kernel", KERNEL[kernel])
    c = _case("a", 2072, 520, 480)
    names = ["plain", "res32", "gelu_pre", "gelu_d8", "dgelu", "relu_res32_pre"]
    base = {}
    for name in names:
        base[name] = _run(c, name, ops, dev)
        _verify(c, name, *base[name], ops, dev, kernel)
    for nwg in (8, 16):
        kopt("gemm_nwg", nwg)
        for name in names:
            out, pre = _run(c, name, ops, dev)
            assert _same(out, base[name][0]) and (pre is None or _same(pre, base[name][1])), (name, nwg)


# ------------------------------------------------------------------------------------------------ exact properties
PROP_CASES = [("v1", (129, 136, 120)), ("v2", (300, 136, 96)), ("v3", (2072, 264, 160)), ("v4", (2072, 264, 160))]


def _select(kopt, kernel):
    kopt("gemm_kernel", KERNEL[kernel])
    if kernel in ("v3", "v4"):
        kopt("gemm_nwg", 8)


@pytest.mark.parametrize("kernel,shape", PROP_CASES)
def test_bf16_output_is_rne_of_the_f32_output(dev, kopt, kernel, shape):
    """The bf16 output equals RNE of the f32 output of the same request, bit for bit.  plain vs f32: the specialised body
    packs acc + bias (gemm_epilogue.h:292, 333), the run-time body stores acc * 1.0f + bias (410, 420, 477) - the same f32
    value; res16 vs bias + bf16 residual + bf16 out: acc + bias + residual in both (347 / 470), stored (352) or packed (482).
    v1: one kernel, `p.c_f32` decides at the store (gemm_nt.hip:209-217)."""
    ops = _ops()
    _select(kopt, kernel)
    for fam in ("a", "d"):
        c = _case(fam, *shape)
        for n16, n32 in (("plain", "f32"), ("bias_pres16", "res16")):
            assert _is_rne(_run(c, n16, ops, dev)[0], _run(c, n32, ops, dev)[0]), (fam, n16)


@pytest.mark.parametrize("kernel,shape", PROP_CASES[1:])
def test_specialised_mode_equals_the_run_time_epilogue(dev, kopt, kernel, shape):
    """Per mode, specialised == gemm_epi_generic = 1, bit for bit: PLAIN, PLAIN_NB, RES32, RES16, PRES16 add the same
    operands in the same order (gemm_epilogue.h:292 + 338 / 347 against 420 + 464 / 470, alpha = 1 an exact multiply), DGELU
    multiplies by the same gelu_erf_grad (398 / 454 through act_grad, common.h:96), DGELU8 by the same gelu_grad_decode
    (388 / 449).  GELU_PRE / GELU_D8: the pre-activation bits are equal (367 / 432); GELU itself is x Phi(x) in
    gelu_erf8 (common.h:177) but fma(|x| / 2, erf, x / 2) in gelu_erf (common.h:76), and the code is rounded by
    v_cvt_pk_u8_f32 there but by + 0.5 and truncation here (common.h:111, 194): not equal by construction - both are held
    to the f64 bound by the tests above, and here the codes to at most one level apart."""
    ops = _ops()
    _select(kopt, kernel)
    c = _case("a", *shape)
    names = BITWISE_MODES + ["gelu_pre", "gelu_d8"]
    spec = {n: _run(c, n, ops, dev) for n in names}
    kopt("gemm_epi_generic", 1)
    for n in names:
        out, pre = _run(c, n, ops, dev)
        if n in BITWISE_MODES:
            assert _same(out, spec[n][0]), n
        elif n == "gelu_pre":
            assert _same(pre, spec[n][1]), n
        else:
            assert int((pre.cpu().to(torch.int32) - spec[n][1].cpu().to(torch.int32)).abs().max()) <= 1


@pytest.mark.parametrize("kernel,shape,rows", [("v1", (129, 136, 120), 77), ("v2", (300, 136, 96), 129), ("v2", (300, 136, 96), 15),
                                               ("v3", (2072, 264, 160), 2050), ("v4", (2072, 264, 160), 2050)])
def test_rows_do_not_depend_on_the_batch(dev, kopt, kernel, shape, rows):
    """Rows 0 .. m - 1 of the M-row call == the call on the first m rows, bit for bit, with m inside another tile than M: an
    output element is one dot product over k of its own row and column in a fixed K order (MFMA lanes do not mix rows),
    tails are clamped (v1 / v2: gemm_nt.hip:64, gemm_nt_v2.hip:73) or zero-filled by the descriptor's range check
    (gemm_nt_persistent.h:60-64), and only stores are predicated."""
    ops = _ops()
    _select(kopt, kernel)
    c = _case("a", *shape)
    for n in ("plain", "res32", "gelu_pre", "dgelu", "relu_res32_pre"):
        full, part = _run(c, n, ops, dev), _run(c, n, ops, dev, rows=rows)
        assert _same(full[0][:rows], part[0]), n
        assert full[1] is None or _same(full[1][:rows], part[1]), n


@pytest.mark.parametrize("kernel,shape", PROP_CASES[1:])
def test_streaming_stores_change_nothing(dev, kopt, kernel, shape):
    """epi_nt = 1 == epi_nt = 0: the option only selects the aux bits of the buffer stores (gemm_epilogue.h:172-175, 380),
    every specialised mode."""
    ops = _ops()
    _select(kopt, kernel)
    c = _case("a", *shape)
    names = [n for n, q in REQUESTS.items() if q.mode != "generic"]
    base = {n: _run(c, n, ops, dev) for n in names}
    kopt("epi_nt", 1)
    for n in names:
        out, pre = _run(c, n, ops, dev)
        _verify(c, n, out, pre, ops, dev, kernel)
        assert _same(out, base[n][0]) and (pre is None or _same(pre, base[n][1])), n


# ------------------------------------------------------------------------------------------------ v2 instantiations
@pytest.mark.parametrize("bm,stages", [(256, 1), (256, 2), (0, 2)])
@pytest.mark.parametrize("K", [64, 96, 480])
@pytest.mark.parametrize("M", [1, 255, 257, 600])
def test_v2_option_instantiations(dev, kopt, M, K, bm, stages):
    """gemm_nt_v2_kernel<256, 1>, <256, 2>, <128, 2> (options gemm_bm = 256, gemm_stages = 2; gemm_nt_v2.hip:181-193): the
    8-wave tile and the two-stage pipeline with its counted vmcnt(8) / vmcnt(6) waits (143-144), one K-step (K = 64), a
    last step with ksub = 1 (96), many (480); run-time epilogue with bias + relu + f32 residual + pre-activation.  Within the
    f64 bound, exact on family (c), and bitwise equal to the default <128, 1> instantiation: all four walk K in the same
    64-deep steps and 32-deep halves (`compute`, 111-127)."""
    ops = _ops()
    kopt("gemm_kernel", 2)
    cases = [_case(fam, M, 136, K) for fam in ("a", "c")]
    base = [_run(c, "relu_res32_pre", ops, dev) for c in cases]       # gemm_bm = 0, gemm_stages = 1: the defaults
    kopt("gemm_bm", bm)
    kopt("gemm_stages", stages)
    for c, (out0, pre0) in zip(cases, base):
        out, pre = _run(c, "relu_res32_pre", ops, dev)
        _verify(c, "relu_res32_pre", out, pre, ops, dev, "v2")
        assert _same(out, out0) and _same(pre, pre0)


# ------------------------------------------------------------------------------------------------ raw calls
def _gemm_raw(ops, a, b, c, bias=None, act=None, pre=None, aux=None, dact=None, res=None, alpha=1.0, drop_p=0.0, rope=None,
              M=None, N=None, K=None):
    """clipk_gemm_nt on 2-D device tensors (views welcome: leading dimensions are their row strides); returns the status."""
    args = ops.GemmArgs()
    args.A, args.lda = a.data_ptr(), a.stride(0)
    args.B, args.ldb = b.data_ptr(), b.stride(0)
    args.C, args.ldc, args.c_dtype = c.data_ptr(), c.stride(0), ops.F32 if c.dtype == torch.float32 else ops.BF16
    args.M, args.N, args.K = (a.shape[0] if M is None else M), (b.shape[0] if N is None else N), (a.shape[1] if K is None else K)
    args.bias = ops.ptr(bias)
    args.act, args.dact = ops.ACT[act], ops.ACT[dact]
    args.out_preact, args.ldp = ops.ptr(pre), (pre.stride(0) if pre is not None else 0)
    args.dact_aux, args.ldd = ops.ptr(aux), (aux.stride(0) if aux is not None else 0)
    args.residual, args.ldr = ops.ptr(res), (res.stride(0) if res is not None else 0)
    args.r_dtype = ops.F32 if (res is not None and res.dtype == torch.float32) else ops.BF16
    args.alpha, args.drop_p, args.drop_seed = alpha, drop_p, DROP_SEED
    u8 = (pre is not None and pre.dtype == torch.uint8) or (aux is not None and aux.dtype == torch.uint8)
    args.aux_dtype = ops.U8 if u8 else ops.BF16
    args.rope_cos = args.rope_sin = None
    args.rope_L = args.rope_hd = args.rope_cols = args.rope_row0 = args.rope_interleaved = 0
    if rope is not None:
        args.rope_cos, args.rope_sin, args.rope_L, args.rope_hd, args.rope_cols = rope[0].data_ptr(), rope[1].data_ptr(), *rope[2:]
    return ops._lib().clipk_gemm_nt(C.byref(args), ops._stream())


def _wide(t, extra, dev, fill, rows_extra=0):
    """(buffer, view): t [r, c] as the leading columns of a [r + rows_extra, c + extra] device buffer filled with `fill`."""
    r, c = t.shape
    buf = torch.full((r + rows_extra, c + extra), fill, dtype=t.dtype, device=dev)
    buf[:r, :c] = t.to(dev)
    return buf, buf[:r, :c]


def _out(M, N, extra, dtype, dev):
    """(buffer, view) of an output with `extra` padding columns and GUARD rows below M, all sentinel."""
    fill = 201 if dtype == torch.uint8 else -12288.0
    buf = torch.full((M + GUARD, N + extra), fill, dtype=dtype, device=dev)
    return buf, buf[:M, :N]


def _untouched(buf, M, N):
    """Everything outside [:M, :N] still holds the sentinel."""
    fill = buf[-1, -1]
    return bool((buf[M:] == fill).all()) and bool((buf[:M, N:] == fill).all())


# requests of the leading-dimension test: (name, act, out type, residual type, pre type, aux type, dact) - the run-time
# epilogue with every operand at once, then each specialised mode that reads or writes a strided operand
LD_REQUESTS = [("generic_all", "relu", torch.float32, torch.float32, BF, BF, "relu"),
               ("plain", None, BF, None, None, None, None), ("res32", None, torch.float32, torch.float32, None, None, None),
               ("res16", None, torch.float32, BF, None, None, None), ("pres16", None, BF, BF, None, None, None),
               ("gelu_pre", "gelu", BF, None, BF, None, None), ("gelu_d8", "gelu", BF, None, torch.uint8, None, None),
               ("dgelu", None, BF, None, None, BF, "gelu"), ("dgelu8", None, BF, None, None, torch.uint8, "gelu")]


@pytest.mark.parametrize("kernel,shape", [("v1", (77, 136, 120)), ("v2", (129, 136, 96)), ("v3", (2072, 264, 160)),
                                          ("v4", (2072, 264, 160))])
def test_leading_dimensions(dev, kopt, kernel, shape):
    """Every operand a column slice of a wider buffer: lda = K + 8, ldb = K + 16, ldc / ldp / ldd / ldr = N + 8 / 16 / 24 / 32,
    the inputs' padding NaN, the outputs' padding and GUARD rows below M a sentinel.  v3 / v4 build per-lane buffer offsets
    and descriptor extents from lda / ldb (gemm_nt_v3.hip:63-64, gemm_nt_persistent.h:60-64), the specialised epilogues their store offsets and
    extents from ldc / ldp (gemm_epilogue.h:193-197), the operand fetches from ldr / ldd (243-253).  Bitwise equal to the
    dense call, sentinels untouched, nothing non-finite."""
    ops = _ops()
    _select(kopt, kernel)
    M, N, K = shape
    c = _case("a", M, N, K)
    nan = float("nan")
    a_d, b_d = _dev(c, "a", dev), _dev(c, "b", dev)
    _, a_w = _wide(c.a.to(BF), 8, dev, nan)
    _, b_w = _wide(c.b.to(BF), 16, dev, nan)
    bias = _dev(c, "bias", dev)
    for name, act, odt, rdt, pdt, adt, dact in LD_REQUESTS:
        if kernel == "v1" and torch.uint8 in (pdt, adt):
            continue                                                   # refused there: test_refusals_forward
        res = None if rdt is None else (c.res if rdt == torch.float32 else c.res16.to(BF))
        aux = None if adt is None else (c.codes if adt == torch.uint8 else c.aux.to(BF))
        has_bias = name not in ("pres16", "dgelu", "dgelu8")
        outs = []
        for wide in (False, True):
            cbuf, cv = _out(M, N, 8 if wide else 0, odt, dev)
            pbuf, pv = _out(M, N, 16 if wide else 0, pdt, dev) if pdt is not None else (None, None)
            av = None if aux is None else _wide(aux, 24 if wide else 0, dev, 0 if adt == torch.uint8 else nan)[1]
            rv = None if res is None else _wide(res, 32 if wide else 0, dev, nan)[1]
            rc = _gemm_raw(ops, a_w if wide else a_d, b_w if wide else b_d, cv, bias=bias if has_bias else None, act=act,
                           pre=pv, aux=av, dact=dact, res=rv)
            assert rc == 0, (name, wide, rc)
            assert _untouched(cbuf, M, N) and (pbuf is None or _untouched(pbuf, M, N)), (name, wide)
            outs.append((cv.contiguous(), None if pv is None else pv.contiguous()))
        assert torch.isfinite(outs[1][0].float()).all() and (outs[1][1] is None or torch.isfinite(outs[1][1].float()).all()), name
        assert _same(outs[0][0], outs[1][0]), name
        assert outs[0][1] is None or _same(outs[0][1], outs[1][1]), name
        # ... and right: every operand at once is a request no other test makes
        ref, _, e, _ = R.linear(c.a, c.b, bias=c.bias if has_bias else None, act=act, dact_aux=aux,
                                dact="gelu8" if adt == torch.uint8 else dact,
                                residual=None if res is None else res.to(torch.float32), want_bounds=True, product=c.product)
        _within(outs[1][0], ref, e if odt == torch.float32 else R.bf16_bound(ref, e), f"{kernel} {'f32' if odt == torch.float32 else 'bf16'}",
                f"{kernel} ld {name}")


def _refused(ops, rc, code):
    """The status is `code`, through what ops.check raises for it."""
    with pytest.raises(ops._ffi.ClipkError, match=rf"\(status {code}\)"):
        ops.check(rc, "clipk_gemm_nt")


@pytest.mark.parametrize("kernel", ["v1", "v2", "v3"])
def test_refusals_forward(dev, kopt, kernel):
    """Argument checks of clipk_gemm_nt / gemm_nt_one (gemm_nt.hip:231-234, 262-270, 286-287) and of epi_mode_for
    (gemm_epilogue.h:72-75): each returns before any launch with the status the code names, and leaves the output alone.
    N or K % 8 (UNSUPPORTED), lda / ldb / ldc % 8 (UNSUPPORTED), ldp / ldd / ldr % 8 (BAD_ARG), misaligned A / B / C / bias /
    residual (BAD_ARG), drop_p >= 1 and NaN (BAD_ARG), 8-bit aux with a non-GELU activation (UNSUPPORTED, fast kernels), 8-bit
    aux or rotation on the generic-K kernel (UNSUPPORTED)."""
    ops = _ops()
    kopt("gemm_kernel", KERNEL[kernel])
    M, N, K = (2048, 136, 160) if kernel == "v3" else (16, 136, 96)
    z = lambda r, c_, dt=BF: torch.zeros(r, c_, dtype=dt, device=dev)   # noqa: E731
    a, b = z(M, K), z(N, K)
    bias = torch.zeros(N, device=dev)
    cbuf, cv = _out(M, N, 0, BF, dev)
    before = cbuf.clone()

    def check(code, a_=a, b_=b, c_=cv, **kw):
        _refused(ops, _gemm_raw(ops, a_, b_, c_, **kw), code)
        torch.cuda.synchronize()
        assert _same(cbuf, before)

    check(UNSUPPORTED, N=N - 4)                                        # N % 8
    check(UNSUPPORTED, K=K - 4)                                        # K % 8
    check(UNSUPPORTED, a_=z(M, K + 4)[:, :K])                          # lda % 8
    check(UNSUPPORTED, b_=z(N, K + 4)[:, :K])                          # ldb % 8
    cbuf4 = torch.full((M + GUARD, N + 4), -12288.0, dtype=BF, device=dev)
    _refused(ops, _gemm_raw(ops, a, b, cbuf4[:M, :N]), UNSUPPORTED)    # ldc % 8
    assert bool((cbuf4 == -12288.0).all())
    check(BAD_ARG, res=z(M, N + 4)[:, :N])                             # ldr % 8
    check(BAD_ARG, aux=z(M, N + 4)[:, :N], dact="relu")                # ldd % 8
    check(BAD_ARG, pre=z(M, N + 4)[:, :N], act="relu")                 # ldp % 8
    flat = torch.zeros(M * K + 8, dtype=BF, device=dev)
    check(BAD_ARG, a_=flat[4:4 + M * K].view(M, K))                    # A 8 bytes off a 16-byte boundary
    flatb = torch.zeros(N * K + 8, dtype=BF, device=dev)
    check(BAD_ARG, b_=flatb[4:4 + N * K].view(N, K))
    flatc = torch.full((M * N + 8,), -12288.0, dtype=BF, device=dev)
    _refused(ops, _gemm_raw(ops, a, b, flatc[4:4 + M * N].view(M, N)), BAD_ARG)
    assert bool((flatc == -12288.0).all())
    check(BAD_ARG, bias=torch.zeros(N + 2, device=dev)[2:])
    check(BAD_ARG, res=torch.zeros(M * N + 4, device=dev)[2:2 + M * N].view(M, N))
    check(BAD_ARG, drop_p=1.0)                                         # nn.Dropout(p = 1) zeroes: not a mask
    check(BAD_ARG, drop_p=1.5)
    check(BAD_ARG, drop_p=float("nan"))
    u8 = z(M, N, torch.uint8)
    if kernel == "v1":                                                 # the generic-K kernel has no 8-bit aux and no rotation
        check(UNSUPPORTED, pre=u8, act="gelu")
        check(UNSUPPORTED, aux=u8, dact="gelu")
        cos = torch.ones(8, 8, device=dev)
        check(UNSUPPORTED, bias=bias, rope=(cos, cos, 8, 16, 32))
    else:
        check(UNSUPPORTED, pre=u8, act="relu")                         # 8-bit codes: GELU only
        check(UNSUPPORTED, aux=u8, dact="relu")


# ------------------------------------------------------------------------------------------------ weight gradient
@functools.lru_cache(maxsize=4)
def _wcase(fam, M, N, K):
    dy, x = R.wgrad_operands(fam, M, N, K, 400)
    dw, db, e_dw, e_db = R.wgrad(dy, x, want_bounds=True)
    return SimpleNamespace(fam=fam, M=M, N=N, K=K, dy=dy, x=x, dw=dw, db=db, e_dw=e_dw, e_db=e_db)


def _wgrad_checks(c, ops, dev, key):
    """What every weight-gradient case checks: dW / db within the bound ((a), (b)) or exact ((c)); dW bitwise equal with and
    without the bias; accumulation into preloaded buffers (on (c): reference + preload exactly; else one more rounding); a
    second call bitwise reproducible."""
    what = f"{key} ({c.fam}) {c.M}x{c.N}x{c.K}"
    dy, x = c.dy.to(BF).to(dev), c.x.to(BF).to(dev)
    dw, db = ops.gemm_wgrad(dy, x, want_bias=True)
    dw0, none = ops.gemm_wgrad(dy, x, want_bias=False)
    assert none is None and _same(dw0, dw), what + ": dW depends on want_bias"
    if c.fam == "c":
        _exact(dw, c.dw, what + " dW")
        _exact(db, c.db, what + " db")
    else:
        _within(dw, c.dw, c.e_dw, key, what + " dW")
        _within(db, c.db, c.e_db, key, what + " db")
    pre_w = R.randint((c.N, c.K), 500, -3, 3) if c.fam == "c" else R.randn((c.N, c.K), 500)
    pre_b = R.randint((c.N,), 501, -3, 3) if c.fam == "c" else R.randn((c.N,), 501)
    rw, rb = c.dw + pre_w.to(F64), c.db + pre_b.to(F64)
    acc_w, acc_b = ops.gemm_wgrad(dy, x, dw=pre_w.clone().to(dev), dbias=pre_b.clone().to(dev), accumulate=True, want_bias=True)
    if c.fam == "c":
        _exact(acc_w, rw, what + " dW accumulated")
        _exact(acc_b, rb, what + " db accumulated")
    else:
        _within(acc_w, rw, R.rnd(rw, c.e_dw), key + " accumulated", what + " dW accumulated")
        _within(acc_b, rb, R.rnd(rb, c.e_db), key + " accumulated", what + " db accumulated")
    acc_w0, _ = ops.gemm_wgrad(dy, x, dw=pre_w.clone().to(dev), accumulate=True, want_bias=False)
    assert _same(acc_w0, acc_w), what + ": accumulated dW depends on want_bias"
    dw2, db2 = ops.gemm_wgrad(dy, x, want_bias=True)
    assert _same(dw2, dw) and _same(db2, db), what + ": not reproducible"
    return dw, db


# M = 1, 7, 63 (a single ragged 64-row step through the register-staged branch, gemm_wgrad.hip:134-147), 64 (one whole
# LDS-DMA step), 65, 512 | 513 (the 512-rows-per-split rule, make_plan: 1 | 2 splits), 1100 (3 splits, ragged last step)
WG_M = [1, 7, 63, 64, 65, 512, 513, 1100]
WG_NK = [(8, 8), (120, 136), (128, 128), (136, 264), (264, 120)]


@pytest.mark.parametrize("N,K", WG_NK)
@pytest.mark.parametrize("M", WG_M)
def test_wgrad_128_kernel(dev, kopt, M, N, K):
    """gemm_wgrad.hip wgrad_kernel + wgrad_reduce_kernel (option wgrad_kernel = 2): M < 64 and ragged last steps, both sides of
    the split rule, ragged N / K tiles with the clamped source columns (lines 97-98), `bslab == nullptr`."""
    ops = _ops()
    kopt("wgrad_kernel", 2)
    for fam in ("a", "b", "c"):
        _wgrad_checks(_wcase(fam, M, N, K), ops, dev, "wgrad128")


@pytest.mark.parametrize("N,K", [(8, 264), (256, 256), (264, 8)])
@pytest.mark.parametrize("splits", [1, 2, 3])
@pytest.mark.parametrize("M", [1024, 1030, 1100])
@pytest.mark.parametrize("sched", [3, 4])
def test_wgrad_256_kernel(dev, kopt, sched, M, splits, N, K):
    """gemm_wgrad_v3.hip in both schedules (option wgrad_kernel = 3 / 4) at the smallest M it takes, with wgrad_splits = 1, 2, 3
    (clipk_wgrad_v3_plan: one split of 16 - 18 steps, two, three with a ragged last step; M = 1024 caps the request at 2),
    ragged N / K tiles, and `bslab == nullptr` (want_bias = False, line 100)."""
    ops = _ops()
    kopt("wgrad_kernel", sched)
    kopt("wgrad_splits", splits)
    for fam in ("a", "b", "c"):
        _wgrad_checks(_wcase(fam, M, N, K), ops, dev, "wgrad256")


@pytest.mark.parametrize("sched", [3, 4])
def test_wgrad_256_options_fall_back_below_1024_rows(dev, kopt, sched):
    """use_v3 (gemm_wgrad.hip:259): wgrad_kernel = 3 / 4 at M = 1023 runs the 128 x 128 kernel - still right, and bitwise what
    wgrad_kernel = 2 gives."""
    ops = _ops()
    c = _wcase("a", 1023, 264, 256)
    kopt("wgrad_kernel", sched)
    kopt("wgrad_splits", 2)
    dw, db = _wgrad_checks(c, ops, dev, "wgrad128")
    _wgrad_checks(_wcase("c", 1023, 264, 256), ops, dev, "wgrad128")
    kopt("wgrad_kernel", 2)
    dw2, db2 = ops.gemm_wgrad(c.dy.to(BF).to(dev), c.x.to(BF).to(dev), want_bias=True)
    assert _same(dw, dw2) and _same(db, db2)


@pytest.mark.parametrize("sched", [3, 4])
def test_wgrad_does_not_depend_on_the_split_count_on_integers(dev, kopt, sched):
    """Family (c): every partial sum is an integer, so wgrad_splits = 1, 2, 3 give the same bits (on the other families the split
    changes the order of the f32 additions: they are held to the f64 bound in test_wgrad_256_kernel instead)."""
    ops = _ops()
    kopt("wgrad_kernel", sched)
    c = _wcase("c", 1100, 264, 256)
    dy, x = c.dy.to(BF).to(dev), c.x.to(BF).to(dev)
    got = []
    for splits in (1, 2, 3):
        kopt("wgrad_splits", splits)
        got.append(ops.gemm_wgrad(dy, x, want_bias=True))
    assert all(_same(g[0], got[0][0]) and _same(g[1], got[0][1]) for g in got[1:])
    _exact(got[0][0], c.dw, "dW")


@pytest.mark.parametrize("kernel,M", [(2, 65), (2, 1100), (3, 1030), (4, 1030)])
def test_wgrad_leading_dimensions(dev, kopt, kernel, M):
    """lddy = N + 8, ldx = K + 16, lddw = K + 8 with NaN in the inputs' padding and a sentinel in dW's padding and GUARD rows:
    the 128 x 128 kernel's 32-bit lane offsets (gemm_wgrad.hip:131-132, 140-141), the 256 x 256 kernel's per-lane offsets and
    descriptor extents (gemm_wgrad_v3.hip:112-123), the reduce kernel's row stride (gemm_wgrad.hip:219).  Bitwise equal to the
    dense call."""
    ops = _ops()
    kopt("wgrad_kernel", kernel)
    N, K = 136, 264
    c = _wcase("a", M, N, K)
    nan = float("nan")
    dense = ops.gemm_wgrad(c.dy.to(BF).to(dev), c.x.to(BF).to(dev), want_bias=True)
    _, dyv = _wide(c.dy.to(BF), 8, dev, nan)
    _, xv = _wide(c.x.to(BF), 16, dev, nan)
    wbuf = torch.full((N + GUARD, K + 8), -12288.0, device=dev)
    dw, db = ops.gemm_wgrad(dyv, xv, dw=wbuf[:N, :K], want_bias=True)
    assert _untouched(wbuf, N, K)
    assert torch.isfinite(dw).all() and _same(dw.contiguous(), dense[0]) and _same(db, dense[1])
    _within(dw.contiguous(), c.dw, c.e_dw, "wgrad128" if kernel == 2 else "wgrad256", f"wgrad ld {kernel} {M}")


def test_wgrad_interleaved_rows_at_a_small_shape(dev, kopt):
    """il = (hd, il_cols) at (M, N, K) = (300, 96, 64), hd = 24 (the first-generation test starts at M = 3000): dW rows and db
    entries land in the ORIGINAL order (wgrad_reduce_kernel's il_src, gemm_wgrad.hip:219, 233), within the bound, exact on
    (c), bitwise equal to the plain call on the un-permuted dY, accumulation included."""
    ops = _ops()
    kopt("wgrad_kernel", 2)
    M, N, K, hd = 300, 96, 64, 24
    src = ops.il_source_rows(N, hd, 48)
    for fam in ("a", "c"):
        c = _wcase(fam, M, N, K)
        dy, x = c.dy.to(BF).to(dev), c.x.to(BF).to(dev)
        dyp = c.dy[:, src].contiguous().to(BF).to(dev)
        dw0, db0 = ops.gemm_wgrad(dy, x, want_bias=True)
        dw1, db1 = ops.gemm_wgrad(dyp, x, want_bias=True, il=(hd, 48))
        assert _same(dw0, dw1) and _same(db0, db1)
        rw, rb, e_w, e_b = R.wgrad(c.dy[:, src], c.x, il=(hd, 48), want_bounds=True)
        assert torch.equal(rw, c.dw) and torch.equal(rb, c.db)
        if fam == "c":
            _exact(dw1, rw, "il dW")
            _exact(db1, rb, "il db")
        else:
            _within(dw1, rw, e_w, "wgrad128", "il dW")
            _within(db1, rb, e_b, "wgrad128", "il db")
        acc_w, acc_b = torch.ones_like(dw0), torch.ones_like(db0)
        ops.gemm_wgrad(dyp, x, dw=acc_w, dbias=acc_b, accumulate=True, want_bias=True, il=(hd, 48))
        ref_w, ref_b = ops.gemm_wgrad(dy, x, dw=torch.ones_like(dw0), dbias=torch.ones_like(db0), accumulate=True, want_bias=True)
        assert _same(acc_w, ref_w) and _same(acc_b, ref_b)


def test_refusals_wgrad(dev):
    """clipk_gemm_wgrad's argument checks (gemm_wgrad.hip:278-282) return before any launch and leave dW alone: il_rows %
    il_hd != 0, an odd il_hd, il_rows > N (BAD_ARG); N or K % 8, lddy / ldx % 8, lddw % 4 (UNSUPPORTED); misaligned dY / dW
    (BAD_ARG)."""
    ops = _ops()
    M, N, K = 64, 96, 64
    dy, x = torch.zeros(M, N, dtype=BF, device=dev), torch.zeros(M, K, dtype=BF, device=dev)
    wbuf = torch.full((N, K), -12288.0, device=dev)

    def check(code, dy_=dy, x_=x, dw_=wbuf, il=(0, 0)):
        with pytest.raises(ops._ffi.ClipkError, match=rf"\(status {code}\)"):
            ops.gemm_wgrad(dy_, x_, dw=dw_, want_bias=True, il=il)
        torch.cuda.synchronize()
        assert bool((wbuf == -12288.0).all())

    check(BAD_ARG, il=(24, 50))                                        # il_rows % il_hd
    check(BAD_ARG, il=(3, 48))                                         # odd head
    check(BAD_ARG, il=(24, 120))                                       # il_rows > N
    check(UNSUPPORTED, dy_=torch.zeros(M, N + 4, dtype=BF, device=dev))                       # N % 8
    check(UNSUPPORTED, x_=torch.zeros(M, K + 4, dtype=BF, device=dev), dw_=torch.zeros(N, K + 4, device=dev))   # K % 8
    check(UNSUPPORTED, dy_=torch.zeros(M, N + 4, dtype=BF, device=dev)[:, :N])                # lddy % 8
    check(UNSUPPORTED, x_=torch.zeros(M, K + 4, dtype=BF, device=dev)[:, :K])                 # ldx % 8
    w2 = torch.full((N, K + 2), -12288.0, device=dev)
    check(UNSUPPORTED, dw_=w2[:, :K])                                  # lddw % 4
    assert bool((w2 == -12288.0).all())
    check(BAD_ARG, dy_=torch.zeros(M * N + 8, dtype=BF, device=dev)[4:4 + M * N].view(M, N))
    w3 = torch.full((N * K + 4,), -12288.0, device=dev)
    check(BAD_ARG, dw_=w3[2:2 + N * K].view(N, K))
    assert bool((w3 == -12288.0).all())
