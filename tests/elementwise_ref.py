"""Plain f64 references of the small kernels in csrc/elementwise.hip and of the column-sum / L2-norm kernels in
csrc/rowwise.hip: pure torch / numpy on the CPU, one short function per op, written from the semantics those files cite
(F.relu / nn.GELU / F.celu / F.softplus, EsmEmbeddings, position-0 and mean pooling, F.normalize, torch.optim.AdamW after
clip_grad_norm_, round-to-nearest-even f32 -> bf16).  Nothing is imported from clip_dplm_amd.

tests/test_elementwise_ref_host.py pins every function here against torch's own f64 op; tests/test_gpu_elementwise.py
compares the HIP kernels with them.  The second half of the file is what the GELU tolerance of the GPU test is measured
with: the kernels' Abramowitz-Stegun 7.1.26 erf (csrc/common.h gelu_parts) evaluated in numpy float32.
"""
import math

import numpy as np
import torch

ACTS = ("relu", "gelu", "celu", "softplus")
F64 = torch.float64


# ---------------------------------------------------------------------------------------------- activations
def act(x, name):
    """F.relu / nn.GELU() (erf form) / F.celu(alpha=1) / F.softplus(beta=1, threshold=20) in f64.  1 + erf(z) is written
    erfc(-z): the same function, without the cancellation that leaves 1 + erf(z) no correct digit below z = -5.8."""
    x = x.to(F64)
    if name == "relu":
        return torch.where(x > 0, x, torch.zeros_like(x))
    if name == "gelu":
        return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))
    if name == "celu":
        return torch.where(x > 0, x, torch.expm1(torch.clamp(x, max=0.0)))
    if name == "softplus":
        return torch.where(x > 20, x, torch.log1p(torch.exp(torch.clamp(x, max=20.0))))
    raise ValueError(name)


def act_grad(x, name):
    """d act / dx in f64 (the branch points as torch has them: relu'(0) = 0, celu'(0) = 1, softplus' = 1 above 20)."""
    x = x.to(F64)
    if name == "relu":
        return (x > 0).to(F64)
    if name == "gelu":
        return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    if name == "celu":
        return torch.where(x > 0, torch.ones_like(x), torch.exp(torch.clamp(x, max=0.0)))
    if name == "softplus":
        return torch.where(x > 20, torch.ones_like(x), torch.sigmoid(x))
    raise ValueError(name)


# ---------------------------------------------------------------------------------------------- bf16 rounding
# the bit patterns the cast tests place in the vector body and in the scalar tail
CAST_TABLE = np.array([0x3f808000, 0x3f818000,            # ties: down to the even 0x3f80, up to the even 0x3f82
                       0xbf808000, 0xbf818000,
                       0x3f7fffff,                        # carry into the exponent -> 1.0
                       0x7f7fffff, 0xff7fffff,            # largest finite -> inf
                       0x7f800000, 0xff800000,            # inf
                       0x7fc00000, 0xffc00001, 0x7f800001, 0x7fa00000, 0xff80ffff,     # quiet / signalling NaN
                       0x00000000, 0x80000000,            # +-0
                       0x00800000, 0x80800000,            # smallest normal
                       0x00000001, 0x00008000, 0x007fffff, 0x807f8000], dtype=np.uint32)  # subnormals (the last: a tie)


def bf16_rne_bits(bits):
    """f32 bit patterns (any integer array / tensor) -> bf16 bit patterns, round to nearest even in integer arithmetic.
    NaN stays NaN (quiet bit set, payload truncated), as torch's and the hardware's conversions keep it."""
    b = np.asarray(bits).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    nan = (b & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    r = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    return np.where(nan, (b >> np.uint64(16)) | np.uint64(0x40), r).astype(np.uint16)


def f32_bits(x):
    """f32 tensor -> its bit patterns as a numpy uint32 array."""
    return x.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


def bf16_bits(x):
    """bf16 tensor -> its bit patterns as a numpy uint16 array."""
    return x.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def bf16_from_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(bits, dtype=np.uint16)).view(np.int16)).view(torch.bfloat16)


def f32_from_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(bits, dtype=np.uint32)).view(np.int32)).view(torch.float32)


def round_f64_to_bf16(p):
    """f64 tensor -> the nearest bf16 value (ties to even), returned as f64.  ONE rounding: going through f32 first would
    round twice.  Normal range: the 52-bit mantissa is cut to 7 bits on the f64 bit pattern; below 2^-126 the grid is
    the fixed subnormal step 2^-133; beyond the largest finite bf16 the result is inf."""
    p = p.to(F64).contiguous()
    b = p.view(torch.int64).numpy().view(np.uint64)
    r = (b + np.uint64((1 << 44) - 1) + ((b >> np.uint64(45)) & np.uint64(1))) >> np.uint64(45) << np.uint64(45)
    out = torch.from_numpy(r.view(np.int64).copy()).view(F64)
    out = torch.where(out.abs() > 3.3895313892515355e38, torch.copysign(torch.full_like(p, math.inf), p), out)
    sub = torch.round(p * 2.0 ** 133) * 2.0 ** -133               # torch.round: half to even
    out = torch.where(p.abs() < 2.0 ** -126, sub, out)
    return torch.where(torch.isnan(p), p, out)


def dact(dy, aux, name, dy_bf16):
    """bf16( dy * act'(aux) ) as f64 values plus the exact f64 product: aux is rounded to bf16 first, dy too when the
    kernel reads it as bf16 (the f32 form multiplies the f32 value); product in f64, ONE rounding to bf16."""
    a = aux.to(torch.bfloat16).to(F64)
    d = dy.to(torch.bfloat16).to(F64) if dy_bf16 else dy.to(torch.float32).to(F64)
    p = d * act_grad(a, name)
    return round_f64_to_bf16(p), p


# ---------------------------------------------------------------------------------------------- axpby / colsum
def axpby(a, b, s):
    """a + s * b (a = None: s * b), f64."""
    y = float(s) * b.to(F64)
    return y if a is None else a.to(F64) + y


def colsum(x):
    """(sum over rows, sum over rows of |x|), f64: the value and the scale of its rounding bound."""
    x = x.to(F64)
    return x.sum(0), x.abs().sum(0)


# ---------------------------------------------------------------------------------------------- embedding
def embed_weight(ids, row_scale, mask, mask_token_id, V):
    """Per-token factor [B, L] f64: row_scale[b] * mask[b, l] * (id != mask_token_id); valid [B, L]: 0 <= id < V."""
    B, L = ids.shape
    w = torch.ones(B, L, dtype=F64)
    if row_scale is not None:
        w = w * row_scale.to(F64).view(B, 1)
    if mask is not None:
        w = w * (mask.view(B, L) != 0).to(F64)
    w = w * (ids != mask_token_id).to(F64)
    return w, (ids >= 0) & (ids < V)


def embed_fwd(ids, table, row_scale=None, mask=None, mask_token_id=-1):
    """x[b, l] = table[ids[b, l]] * factor, [B, L, d] in the table's dtype (the kernel's one f32 product when the table
    is f32: exact comparison); a token outside the table gives a NaN row."""
    V = table.shape[0]
    w, ok = embed_weight(ids, row_scale, mask, mask_token_id, V)
    w = w if row_scale is None else (row_scale.to(table.dtype).view(-1, 1) * (w != 0).to(table.dtype))
    x = table[ids.clamp(0, V - 1)] * w.to(table.dtype).unsqueeze(-1)
    return torch.where(ok.unsqueeze(-1), x, torch.full_like(x, math.nan))


def embed_bwd(ids, dx, V, row_scale=None, mask=None, mask_token_id=-1):
    """(dtable, sum of |terms|), both f64 [V, d]: index_add_ of dx * factor over the tokens whose id is inside the table
    (the others contribute nothing)."""
    B, L = ids.shape
    w, ok = embed_weight(ids, row_scale, mask, mask_token_id, V)
    sel = ok.view(-1)
    terms = (dx.to(F64).view(B * L, -1) * w.view(-1, 1))[sel]
    idx = ids.view(-1)[sel]
    d = dx.shape[-1]
    return (torch.zeros(V, d, dtype=F64).index_add_(0, idx, terms),
            torch.zeros(V, d, dtype=F64).index_add_(0, idx, terms.abs()))


# ---------------------------------------------------------------------------------------------- pooling
def pool_fwd(x, B, L, mask=None, mode=1):
    """mode 0: position 0; mode 1: mean over the valid positions, 0 for a sequence without any."""
    x = x.to(F64).view(B, L, -1)
    if mode == 0:
        return x[:, 0].clone()
    m = torch.ones(B, L, dtype=F64) if mask is None else (mask.view(B, L) != 0).to(F64)
    n = m.sum(1, keepdim=True)
    return torch.where(n > 0, (x * m.unsqueeze(-1)).sum(1) / n.clamp(min=1.0), torch.zeros(B, x.shape[-1], dtype=F64))


def pool_bwd(dy, B, L, mask=None, mode=1):
    dy = dy.to(F64)
    dx = torch.zeros(B, L, dy.shape[-1], dtype=F64)
    if mode == 0:
        dx[:, 0] = dy
        return dx
    m = torch.ones(B, L, dtype=F64) if mask is None else (mask.view(B, L) != 0).to(F64)
    n = m.sum(1, keepdim=True)
    sc = torch.where(n > 0, m / n.clamp(min=1.0), torch.zeros_like(m))
    return dy.unsqueeze(1) * sc.unsqueeze(-1)


# ---------------------------------------------------------------------------------------------- L2 normalise
def l2norm(x, dy=None, eps=1e-12):
    """F.normalize(x, dim=-1, eps): y = x / max(|x|, eps), the norm, and (with dy) dx = (dy - y (y.dy)) / |x| for
    |x| >= eps, dy / eps below it (the clamp is a constant there)."""
    x = x.to(F64)
    n = x.pow(2).sum(-1, keepdim=True).sqrt()
    y = x / n.clamp(min=eps)
    if dy is None:
        return y, n.squeeze(-1)
    dy = dy.to(F64)
    dx = torch.where(n < eps, dy / eps, (dy - y * (y * dy).sum(-1, keepdim=True)) / n.clamp(min=eps))
    return y, n.squeeze(-1), dx


# ---------------------------------------------------------------------------------------------- optimiser
def sumsq(g):
    return float(g.to(F64).pow(2).sum())


def clip_coef(g, max_norm, grad_scale=1.0):
    """torch.nn.utils.clip_grad_norm_ on the SCALED gradient: min(1, max_norm / (norm + 1e-6))."""
    norm = math.sqrt(sumsq(g)) * grad_scale
    return min(1.0, max_norm / (norm + 1e-6))


def adamw_step(w, g, m, v, lr, beta1, beta2, eps, weight_decay, step, max_norm=None, grad_scale=1.0):
    """One torch.optim.AdamW step in f64 on g * grad_scale, clipped to max_norm when given.  Returns new (w, m, v)."""
    w, g, m, v = (t.to(F64) for t in (w, g, m, v))
    coef = clip_coef(g, max_norm, grad_scale) if max_norm is not None else 1.0
    g = g * grad_scale * coef
    w = w * (1.0 - lr * weight_decay)                                   # decoupled decay
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    bc1 = 1.0 - beta1 ** step
    bc2_sqrt = math.sqrt(1.0 - beta2 ** step)
    w = w - (lr / bc1) * m / (v.sqrt() / bc2_sqrt + eps)
    return w, m, v


# ---------------------------------------------------------------------------------------------- GELU tolerance
# The kernels evaluate erf by Abramowitz-Stegun 7.1.26 in f32 with the hardware's approximate reciprocal and exp2
# (csrc/common.h gelu_parts).  The same formula in numpy float32 (correctly rounded ops, fma as one f64 operation rounded
# to f32), measured over act_grid() against the f64 functions above:  E = max |err| / max(1, |x|).
# tests/test_elementwise_ref_host.py asserts the measurement stays within these figures and that they are not stale
# (within 25 % of it); the GPU test allows 4 E max(1, |x|): the factor 4 covers the two 1-ulp hardware approximations.
GELU_E = 1.5e-7          # measured 1.431e-07 at x = 1.205 (GELU)
GELU_GRAD_E = 2.2e-7     # measured 2.154e-07 at x = 0.343 (GELU')
GPU_FACTOR = 4.0


def act_grid():
    """f32 inputs of the activation tests: 60 001 points on [-30, 30] plus the branch points and the far tails."""
    g = torch.linspace(-30.0, 30.0, 60001, dtype=F64).to(torch.float32)
    t20 = np.float32(20.0)
    extra = torch.tensor([0.0, -0.0, 20.0, float(np.nextafter(t20, np.float32(0))), float(np.nextafter(t20, np.float32(40))),
                          88.0, -88.0, -104.0], dtype=torch.float32)
    return torch.cat([g, extra])


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _gelu_parts_f32(x):
    f = np.float32
    x = np.asarray(x, dtype=f)
    ax = np.abs(x)
    one = np.ones_like(x)
    t = one / _fma32(np.full_like(x, f(0.3275911) * f(0.70710678118654752440)), ax, one)
    e = np.exp2(f(-0.72134752044448170368) * x * x).astype(f)
    poly = _fma32(np.full_like(x, f(1.061405429)), t, np.full_like(x, f(-1.453152027)))
    for c in (1.421413741, -0.284496736, 0.254829592):
        poly = _fma32(poly, t, np.full_like(x, f(c)))
    return _fma32(-poly * t, e, one), e


def gelu_as_f32(x):
    """csrc/common.h gelu_erf in numpy float32 (x: f32 tensor) -> f32 tensor."""
    x = x.detach().cpu().numpy().astype(np.float32)
    erf_abs, _ = _gelu_parts_f32(x)
    return torch.from_numpy(_fma32(np.float32(0.5) * np.abs(x), erf_abs, np.float32(0.5) * x))


def gelu_grad_as_f32(x):
    """csrc/common.h gelu_erf_grad in numpy float32."""
    x = x.detach().cpu().numpy().astype(np.float32)
    erf_abs, e = _gelu_parts_f32(x)
    cdf = _fma32(np.copysign(np.float32(0.5), x), erf_abs, np.full_like(x, 0.5))
    return torch.from_numpy(_fma32(x * np.float32(0.39894228040143267794), e, cdf))


def dact_gelu_grad_as_f32(x):
    """GELU' as dact_kernel evaluates it (csrc/elementwise.hip dact_grad) in numpy float32: gelu_erf_grad, and below
    x = -4 the Mills-ratio form phi(x) N(x^2) / (x D(x^2)) with exp2 scaled by 2^64 (gelu_grad_tail)."""
    f = np.float32
    xn = x.detach().cpu().numpy().astype(f)
    xc = np.maximum(xn, f(-20.0))
    s = xc * xc
    num = _fma32(_fma32(s + f(9.0), s, np.full_like(s, 6.0)), s, np.full_like(s, -8.0))
    den = xc * _fma32(s + f(10.0), s, np.full_like(s, 15.0))
    e = np.exp2(_fma32(f(-0.72134752044448170368) * xc, xc, np.full_like(s, 64.0))).astype(f)
    with np.errstate(divide="ignore"):                      # x = 0: not selected below
        tail = (f(0.39894228040143267794) * e) * num * (np.ones_like(s) / den) * f(2.0 ** -64)
    return torch.from_numpy(np.where(xn < f(-4.0), tail, gelu_grad_as_f32(x).numpy()).astype(f))


def gelu_error(x, grad=False):
    """max over x of |numpy-f32 A&S value - f64 reference| / max(1, |x|)."""
    got = (gelu_grad_as_f32(x) if grad else gelu_as_f32(x)).to(F64)
    ref = act_grad(x, "gelu") if grad else act(x, "gelu")
    return float(((got - ref).abs() / x.to(F64).abs().clamp(min=1.0)).max())


def act_tol(x, name, grad, ref):
    """Allowed |kernel - f64| per element.  relu / celu / softplus: rtol 1e-6, atol 1e-7 (ocml expm1f / log1pf / expf
    to a few ulp, exact branch points).  gelu: GPU_FACTOR * E * max(1, |x|)."""
    if name == "gelu":
        return GPU_FACTOR * (GELU_GRAD_E if grad else GELU_E) * x.to(F64).abs().clamp(min=1.0)
    return 1e-6 * ref.abs() + 1e-7


def dact_check(out_bits, dy, aux, name, dy_bf16):
    """The rule for bf16( dy * act'(aux) ): `out_bits` (uint16 array) equal the reference's bits, or differ from them
    only where the exact f64 product p lies within the kernel's tolerance of a bf16 rounding boundary, i.e. the value is
    the bf16 rounding of something in [p - tol, p + tol] with tol = |dy| * act_tol(act') + 2^-24 |p| (the f32 product
    the kernel rounds first).  Returns (number of elements outside that interval, number of elements whose bits differ
    from the reference's, number of those more than one bf16 step away); +0 and -0 count as equal (an underflowed
    GELU' is +0 in the kernel and -1e-200 in f64)."""
    ref, p = dact(dy, aux, name, dy_bf16)
    a = aux.to(torch.bfloat16).to(F64)
    d = dy.to(torch.bfloat16).to(F64) if dy_bf16 else dy.to(torch.float32).to(F64)
    tol = d.abs() * act_tol(a, name, True, act_grad(a, name)) + 2.0 ** -24 * p.abs()
    lo, hi = round_f64_to_bf16(p - tol), round_f64_to_bf16(p + tol)
    out = bf16_from_bits(out_bits).to(F64).view(ref.shape)
    outside = int(((out < lo) | (out > hi) | torch.isnan(out)).sum())
    differ = out != ref
    # one bf16 step: the next representable value on either side of the reference
    step = torch.maximum(2.0 ** (torch.floor(torch.log2(ref.abs().clamp(min=2.0 ** -126))) - 7), torch.tensor(2.0 ** -133, dtype=F64))
    far = differ & ((out - ref).abs() > step * 1.0000001)
    return outside, int(differ.sum()), int(far.sum())
