"""Plain f64 references of the bf16 Linear (clipk_gemm_nt: csrc/gemm_nt*.hip, csrc/gemm_epilogue.h) and of the weight
gradient (clipk_gemm_wgrad: csrc/gemm_wgrad*.hip), the seeded input families their tests share and the per-element error
bounds they allow.  Pure torch on the CPU; activations, bf16 helpers and the GELU tolerance come from
tests/elementwise_ref.py; no GPU and no kernel code here (ops.il_source_rows, the host-side index formula of the
pair-interleaved row order, is the one import from the package).  Inputs are the values the kernel sees - bf16-rounded
where it takes bf16 - widened to f64.

tests/test_gemm_ref_host.py pins the references, holds a numpy-f32 stand-in inside the bounds and shows that every seeded
fault falls outside them; tests/test_gpu_gemm.py compares the HIP kernels with them.

Order of operations (ops.gemm_nt):  s = A B^T;  pre = alpha s + bias  (the pre-activation output is taken here);
v = act(pre);  v *= keep / (1 - p);  v *= act'(aux);  out = v + residual.

Bounds (derived, none taken from GPU output).  u = 2^-23, h = 2^-24, S = |A| |B|^T (f64).
  * Main loop.  The products of two bf16 values are exact in f32 (16 significant bits).  An f32 accumulation of n such
    products in ANY order and grouping makes n - 1 additions, each with a relative error of at most u whether the adder
    rounds to nearest (h) or truncates (u) - the matrix pipe's internal adds are not documented to round - so
        |s^ - s| <= n u S                         n = K (forward), M (weight gradient; S = |dY|^T |X|).
  * Every fused f32 add or multiply of the epilogue rounds once: an incoming error e on an exact result r becomes
        rnd(r, e) = e + h (|r| + e).
    alpha s (one multiply), + bias, x dropout scale, x act'(aux), + residual: one rnd each, when the operand is present.
  * Activation: e -> L e + act_tol(pre), L the Lipschitz constant of the activation (1; GELU: 1.13 = max |GELU'|) and
    elementwise_ref.act_tol the evaluation error of the f32 formula (relu and relu' are exact: no term).
  * act'(aux): the factor g carries elementwise_ref.act_tol(grad) = t: e -> rnd(r, e (|g| + t) + |v| t).  8-bit codes
    ("gelu8"): g = fma(code, 0.005f, -0.13f) in f32, t = h |g|.
  * bf16 output: the kernel stores RNE(x) of some f32 x with |x - ref| <= e, so |out - ref| <= e + half a bf16 ulp of the
    largest such x:  e + half_ulp_bf16(|ref| + e).
  * 8-bit GELU' code output: the decoded level is the nearest of the 0.005 grid to GELU'(pre^):
        |decode(code) - GELU'(pre)| <= 0.0025 + 0.8 e_pre + act_tol(GELU') + 2^-15 0.005     (0.8 >= max |GELU''|).
  * Weight gradient: M u S for dW, M u sum_m |dY| for db (the column sum is one more MFMA against ones, same pipe); the
    fixed-order sum of the split slabs is part of the same n - 1 additions.  Accumulating into a preloaded dW: one rnd.

Family (c) - small integers - needs no bound: every product and partial sum is an integer below 2^24 for K, M <= 4096, so
the f32 result equals the integer reference in whatever order it is summed, and a bf16 output equals its one rounding.
"""
import torch

import elementwise_ref as E

F64 = torch.float64
U = 2.0 ** -23
H = 2.0 ** -24
FAMILIES = ("a", "b", "c", "d")
OFFSET = 1000.0                 # family (d): common offset of the residual
LIP = {None: 1.0, "none": 1.0, "relu": 1.0, "gelu": 1.13, "celu": 1.0, "softplus": 1.0}
GD8_MIN, GD8_STEP = -0.13, 0.005       # csrc/common.h: the 8-bit GELU' grid


def _w(t):
    return None if t is None else t.detach().cpu().to(F64)


def bf16(x):
    """The values rounded to bf16, kept as an f32 tensor."""
    return x.to(torch.bfloat16).to(torch.float32)


def randn(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32) * scale + shift


def randint(shape, seed, lo=-2, hi=2):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float32)


def _row_scale(n, period):
    """2^-6, 1, 2^6 by row: a wrong row or column shows up against its neighbours."""
    return (2.0 ** (6.0 * ((torch.arange(n) % period) % 3 - 1))).to(torch.float32).view(n, 1)


# ---------------------------------------------------------------------------------------------- inputs
def operands(fam, M, N, K, seed):
    """(a [M, K], b [N, K]) bf16-representable f32: (a), (d) N(0, 1) x N(0, 0.05^2); (b) the same with the rows of both
    scaled by 2^-6 / 1 / 2^6 (period 3 for a, 5 -> 3 for b); (c) integers in -2 .. 2."""
    if fam == "c":
        return randint((M, K), seed), randint((N, K), seed + 1)
    a, b = randn((M, K), seed), randn((N, K), seed + 1, 0.05)
    if fam == "b":
        a, b = a * _row_scale(M, 3), b * _row_scale(N, 5)
    return bf16(a), bf16(b)


def epilogue_operands(fam, M, N, seed):
    """bias [N] f32, residual [M, N] f32 (round it with bf16() for a bf16 residual), aux [M, N] bf16-representable:
    N(0, 1) each; (c): integers in -2 .. 2; (d): the residual is OFFSET + N(0, 1)."""
    if fam == "c":
        return randint((N,), seed), randint((M, N), seed + 1), randint((M, N), seed + 2)
    res = randn((M, N), seed + 1, 1.0, OFFSET if fam == "d" else 0.0)
    return randn((N,), seed), res, bf16(randn((M, N), seed + 2))


def wgrad_operands(fam, M, N, K, seed):
    """(dy [M, N], x [M, K]) bf16-representable: (a), (d) N(0, 0.1^2) x N(0, 1); (b) rows (the contraction index) of both
    scaled by 2^-6 / 1 / 2^6 - so are the COLUMNS of dy; (c) integers in -2 .. 2."""
    if fam == "c":
        return randint((M, N), seed), randint((M, K), seed + 1)
    dy, x = randn((M, N), seed, 0.1), randn((M, K), seed + 1)
    if fam == "b":
        dy, x = dy * _row_scale(N, 5).view(1, N), x * _row_scale(K, 3).view(1, K)
    return bf16(dy), bf16(x)


# ---------------------------------------------------------------------------------------------- helpers
def half_ulp_bf16(v):
    v = v.to(F64).abs().clamp(min=2.0 ** -126)
    return 2.0 ** (torch.floor(torch.log2(v)) - 8)


def rnd(r, e):
    """Error after one f32 operation whose exact result is r and whose operands carried the (propagated) error e."""
    return e + H * (r.abs() + e)


def bf16_bound(ref, e):
    return e + half_ulp_bf16(ref.abs() + e)


def gelu8_decode(codes):
    """fma(code, 0.005f, -0.13f) as the f32 value the kernels multiply with, in f64."""
    q = codes.to(F64)
    step, lo = float(torch.tensor(GD8_STEP, dtype=torch.float32)), float(torch.tensor(GD8_MIN, dtype=torch.float32))
    return (q * step + lo).to(torch.float32).to(F64)


def _grad(aux, name):
    """(factor g, its tolerance t) of the act'(aux) multiply."""
    if name == "gelu8":
        g = gelu8_decode(aux)
        return g, H * g.abs()
    a = _w(aux)
    g = E.act_grad(a, name)
    return g, (torch.zeros_like(g) if name == "relu" else E.act_tol(a, name, True, g))     # relu' is 0 or 1: exact


# ---------------------------------------------------------------------------------------------- forward
def linear(a, b, bias=None, act=None, alpha=1.0, residual=None, dact_aux=None, dact=None, keep=None, want_bounds=False,
           product=None):
    """(out, pre) in f64; with want_bounds also (e_out, e_pre): the f32 error bounds of the module docstring (apply
    bf16_bound for a bf16 output).  keep: None or (mask [M, N] of 0 / 1, scale) - the dropout multiply, `scale` the f32
    value 1 / (1 - p).  dact = "gelu8": dact_aux holds 8-bit GELU' codes.  product: (A B^T, |A| |B|^T) if the caller has
    them already (f64)."""
    if product is None:
        a, b = _w(a), _w(b)
        product = (a @ b.t(), a.abs() @ b.abs().t())
    s, S = product
    K = a.shape[1]
    e = K * U * S
    r = s
    if alpha != 1.0:
        r = alpha * s
        e = rnd(r, abs(alpha) * e)
    if bias is not None:
        r = r + _w(bias)
        e = rnd(r, e)
    pre, e_pre = r, e
    if act not in (None, "none"):
        r = E.act(pre, act)
        e = LIP[act] * e + (0.0 if act == "relu" else E.act_tol(pre, act, False, r))       # max(x, 0) is exact
    if keep is not None:
        mask, scale = keep
        r = r * (_w(mask) * float(scale))
        e = rnd(r, e * float(scale))
    if dact_aux is not None:
        g, t = _grad(dact_aux, dact)
        v = r
        r = v * g
        e = rnd(r, e * (g.abs() + t) + v.abs() * t)
    if residual is not None:
        r = r + _w(residual)
        e = rnd(r, e)
    return (r, pre, e, e_pre) if want_bounds else (r, pre)


def gelu_code_bound(pre, e_pre):
    """Allowed |decode(code) - GELU'(pre)| of the 8-bit pre-activation output (module docstring)."""
    g = E.act_grad(pre, "gelu")
    return 0.5 * GD8_STEP + 0.8 * e_pre + E.act_tol(pre, "gelu", True, g) + 2.0 ** -15 * GD8_STEP


# ---------------------------------------------------------------------------------------------- weight gradient
def wgrad(dy, x, il=None, want_bounds=False):
    """(dW [N, K], db [N]) = (dY^T X, colsum dY) in f64; il = (hd, il_cols): dY's first il_cols columns are in
    pair-interleaved head order and the results come out in the ORIGINAL order.  want_bounds: also (e_dw, e_db)."""
    dy, x = _w(dy), _w(x)
    M, N = dy.shape
    dw, db = dy.t() @ x, dy.sum(0)
    e_dw, e_db = M * U * (dy.abs().t() @ x.abs()), M * U * dy.abs().sum(0)
    if il is not None and il[1] > 0:
        from clip_dplm_amd.ops import il_source_rows
        src = il_source_rows(N, il[0], il[1])

        def back(t):
            o = torch.empty_like(t)
            o[src] = t                                     # permuted row j holds original row src[j]
            return o
        dw, db, e_dw, e_db = back(dw), back(db), back(e_dw), back(e_db)
    return (dw, db, e_dw, e_db) if want_bounds else (dw, db)
