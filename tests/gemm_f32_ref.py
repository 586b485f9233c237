"""Plain f64 references of the exact-f32 GEMM (clipk_gemm_f32: csrc/gemm_f32.hip, tiled and skinny forms) and of its
weight gradient (clipk_gemm_wgrad_f32), the seeded input families their tests share and the per-element error bounds they
allow.  Pure torch on the CPU; no GPU and no kernel code here.  The families are those of tests/gemm_ref.py with FULL 24-bit
mantissas - nothing is rounded to bf16, so an operand that a kernel rounds on its way shows as an error of 2^-9, far outside.

tests/test_gemm_f32_ref_host.py pins the references, holds torch's own f32 product inside the bounds and shows that every
mutant falls outside them; tests/test_gpu_gemm_f32.py compares the HIP kernels with them.

    out[M, N] = alpha * A[M, K] B[N, K]^T (+ bias[N]) (+ addend_scale * addend[M, N])
    dW[N, K] (+)= dY[M, N]^T X[M, K]        db[N] (+)= sum over rows of dY

Operands are LOGICAL here (a [M, K], b [N, K]); the (trans_a, trans_b) layouts only change how a test stores them.

Families:  (a) N(0, 1) x N(0, 0.05^2);  (b) the same with the rows of a and of b scaled by 2^-6 / 1 / 2^6 with periods 3 and
5 (a wrong row or column shows against its neighbours; the family on which "rows do not depend on the batch" is compared
bit for bit, the smaller batch being the first rows of the larger);  (c) integers in -2 .. 2 for a, b, bias and addend, alpha
and addend_scale powers of two;  (d) as (a) with the addend offset by 1000.

Family (c) needs no bound: |partial sum| <= 4 K << 2^24 for every K here, so every partial sum in every summation order,
split and grouping is an integer that f32 holds exactly, the power-of-two scalings are exact, and the f32 result EQUALS the
reference.  A dropped, doubled or mis-paired contraction index, a mis-indexed bias or addend changes an integer.

Bounds for (a), (b), (d) (derived, none taken from GPU output).  u = 2^-23, h = 2^-24, S = |a| |b|^T in f64.
  * Product.  Every term enters through one fused multiply-add (the product itself is not rounded), whose addition has a
    relative error of at most u whether the matrix pipe's adder rounds to nearest (h) or truncates (u).  A term that goes
    through n such roundings on its way to the result carries a factor (1 + d_1) .. (1 + d_n), |d_i| <= u, so
        |s^ - s| <= gamma(n) S,      gamma(n) = n u / (1 - n u),
    in ANY order and grouping.  Tiled form: one chain over the K terms, n <= K.  Skinny form: the K terms are dealt to at
    most 16 waves x 8 splits; a wave's chain is shorter than K, its partial tile then goes through at most 16 additions in
    the workgroup's fixed-order sum (the first onto a zero) and at most 8 in the reduce over the splits: n <= K + 16 + 8.
    One bound serves both forms: gamma(K + 24).
  * Epilogue.  Every f32 operation rounds once: an incoming error e on an exact result r becomes rnd(r, e) = e + h (|r| + e)
    (gemm_ref.rnd).  alpha s: one;  + bias: one;  addend_scale * addend: one (h |product|, no incoming error);  + that:
    one.  Where the compiler contracts a multiply and the add after it into one fma, one of these roundings does not
    happen: the bound stays an upper bound.
  * Weight gradient: gamma(M) |dY|^T |X| for dW (a chain over the M rows), gamma(M) sum_m |dY| for db (M additions in the
    one-pass kernel, fewer in the column reduce); accumulating into a preloaded dW / db: one rnd.
On (a), (b), (d) the kernels use a small part of gamma(K + 24) S (the bf16 GEMMs measured about a hundredth): these families
hold the arithmetic to f32, family (c) is what notices a wrong index.
"""
import torch

from gemm_ref import F64, H, OFFSET, U, randint, randn, rnd, _row_scale  # noqa: F401  (one set of generators and helpers)

FAMILIES = ("a", "b", "c", "d")
SKINNY_ADDS = 16 + 8            # additions of the skinny form's partial tiles: 16 waves, then at most 8 splits


def gamma(n):
    """Relative error of a value that went through n f32 additions, each rounded or truncated."""
    return n * U / (1.0 - n * U)


def _w(t):
    return None if t is None else t.detach().cpu().to(F64)


# ---------------------------------------------------------------------------------------------- inputs
def operands(fam, M, N, K, seed):
    """(a [M, K], b [N, K]) f32 with full mantissas.  (The batch-independence tests slice the first rows of ONE draw: the
    row scale of (b) depends on the row index alone.)"""
    if fam == "c":
        return randint((M, K), seed), randint((N, K), seed + 1)
    a, b = randn((M, K), seed), randn((N, K), seed + 1, 0.05)
    if fam == "b":
        a, b = a * _row_scale(M, 3), b * _row_scale(N, 5)
    return a, b


def epilogue_operands(fam, M, N, seed):
    """(bias [N], addend [M, N], alpha, addend_scale): N(0, 1) and 0.37 / -1.7; (c) integers in -2 .. 2 and the powers of
    two 0.5 / 4; (d) the addend is OFFSET + N(0, 1).  alpha and addend_scale are Python floats that f32 holds exactly."""
    if fam == "c":
        return randint((N,), seed), randint((M, N), seed + 1), 0.5, 4.0
    f = lambda v: float(torch.tensor(v, dtype=torch.float32))       # noqa: E731
    return randn((N,), seed), randn((M, N), seed + 1, 1.0, OFFSET if fam == "d" else 0.0), f(0.37), f(-1.7)


def wgrad_operands(fam, M, N, K, seed):
    """(dy [M, N], x [M, K]): (a), (d) N(0, 0.1^2) x N(0, 1); (b) the columns of both scaled by 2^-6 / 1 / 2^6 (periods 5,
    3: the rows of dW and the entries of db); (c) integers in -2 .. 2."""
    if fam == "c":
        return randint((M, N), seed), randint((M, K), seed + 1)
    dy, x = randn((M, N), seed, 0.1), randn((M, K), seed + 1)
    if fam == "b":
        dy, x = dy * _row_scale(N, 5).view(1, N), x * _row_scale(K, 3).view(1, K)
    return dy, x


# ---------------------------------------------------------------------------------------------- forward
def product(a, b):
    """(a b^T, |a| |b|^T) in f64: what gemm() takes as `product` when several requests share the operands."""
    a, b = _w(a), _w(b)
    return a @ b.t(), a.abs() @ b.abs().t()


def gemm(a, b, alpha=None, bias=None, addend=None, addend_scale=None, want_bound=False, product_=None):
    """out in f64; with want_bound also the f32 error bound of the module docstring.  alpha / addend_scale: None or a float."""
    s, S = product(a, b) if product_ is None else product_
    K = a.shape[1]
    e = gamma(K + SKINNY_ADDS) * S
    r = s
    if alpha is not None:
        r = float(alpha) * s
        e = rnd(r, abs(float(alpha)) * e)
    if bias is not None:
        r = r + _w(bias)
        e = rnd(r, e)
    if addend is not None:
        t = _w(addend)
        et = torch.zeros_like(t)
        if addend_scale is not None:
            t = float(addend_scale) * t
            et = H * t.abs()
        r = r + t
        e = rnd(r, e + et)
    return (r, e) if want_bound else r


# ---------------------------------------------------------------------------------------------- weight gradient
def wgrad(dy, x, pre_w=None, pre_b=None, want_bound=False):
    """(dW [N, K], db [N]) = (dY^T X (+ pre_w), colsum dY (+ pre_b)) in f64; want_bound: also (e_dw, e_db)."""
    dy, x = _w(dy), _w(x)
    M = dy.shape[0]
    dw, db = dy.t() @ x, dy.sum(0)
    e_dw, e_db = gamma(M) * (dy.abs().t() @ x.abs()), gamma(M) * dy.abs().sum(0)
    if pre_w is not None:
        dw = dw + _w(pre_w)
        e_dw = rnd(dw, e_dw)
    if pre_b is not None:
        db = db + _w(pre_b)
        e_db = rnd(db, e_db)
    return (dw, db, e_dw, e_db) if want_bound else (dw, db)


def outside(got, ref, bound):
    """Number of elements outside the bound (NaN counts)."""
    return int((~((got.detach().cpu().to(F64) - ref).abs() <= bound)).sum())
