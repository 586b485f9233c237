"""CPU: tests/elementwise_ref.py - the yardstick tests/test_gpu_elementwise.py compares the small HIP kernels with - pinned
against torch's own f64 ops (F.gelu, F.celu, F.softplus, F.normalize with autograd, torch.optim.AdamW after
clip_grad_norm_, F.embedding with autograd, .to(torch.bfloat16)), and the measured GELU tolerance against its recorded
figure, so that neither can drift on a machine without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import elementwise_ref as R  # noqa: E402

F64 = torch.float64


def _randn(shape, seed, dtype=F64):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


TORCH_ACT = {"relu": F.relu, "gelu": F.gelu, "celu": F.celu, "softplus": F.softplus}

CAST_TABLE = R.CAST_TABLE


@pytest.mark.parametrize("name", R.ACTS)
def test_act_and_its_gradient_equal_torch_f64(name):
    x = R.act_grid().to(F64).requires_grad_(True)
    y = TORCH_ACT[name](x)
    (g,) = torch.autograd.grad(y.sum(), x)
    # absolute terms: 1 + erf cancels to 2^-53 in the negative tail (times |x| <= 104), in torch's GELU as in the
    # reference's, and torch differentiates softplus as 1 - 1 / (1 + e^x) below the threshold
    assert torch.allclose(R.act(x.detach(), name), y.detach(), rtol=1e-14, atol=1e-13)
    assert torch.allclose(R.act_grad(x.detach(), name), g, rtol=1e-13, atol=1e-13)


def test_gelu_measured_error_stays_within_the_recorded_figure():
    """E = max |A&S 7.1.26 in numpy float32 - f64| / max(1, |x|) over the test grid: not above the recorded GELU_E /
    GELU_GRAD_E (the GPU bound is 4 E max(1, |x|)) and the record not more than 25 % above the measurement."""
    x = R.act_grid()
    for grad, rec in ((False, R.GELU_E), (True, R.GELU_GRAD_E)):
        e = R.gelu_error(x, grad)
        print(f"grad={grad}: measured E = {e:.4e}, recorded {rec:.2e}, GPU bound {R.GPU_FACTOR * rec:.2e} * max(1, |x|)")
        assert e <= rec <= 1.25 * e


def test_bf16_rne_bits_equal_torch_on_the_table_and_on_random_bits():
    rnd = torch.randint(0, 2 ** 32, (200000,), generator=torch.Generator().manual_seed(1), dtype=torch.int64).numpy()
    bits = np.concatenate([CAST_TABLE, rnd.astype(np.uint32)])
    got = R.bf16_rne_bits(bits)
    want = R.bf16_bits(R.f32_from_bits(bits).to(torch.bfloat16))
    nan = (bits & 0x7fffffff) > 0x7f800000
    assert np.array_equal(got[~nan], want[~nan])
    for b in (got[nan], want[nan]):                       # NaN stays NaN (torch canonicalises it, the payload is free)
        assert ((b & 0x7fff) > 0x7f80).all()
    assert got[0] == 0x3f80 and got[1] == 0x3f82 and got[4] == 0x3f80 and got[5] == 0x7f80 and got[6] == 0xff80


def test_round_f64_to_bf16_is_one_rounding():
    x = _randn((100000,), 2) * torch.exp(_randn((100000,), 3) * 20)
    x = torch.cat([x, R.f32_from_bits(CAST_TABLE[:9]).to(F64), R.f32_from_bits(CAST_TABLE[14:]).to(F64)])
    f32 = x.to(torch.float32)
    # on f32-representable values the two roundings coincide with torch's
    assert torch.equal(R.round_f64_to_bf16(f32.to(F64)), f32.to(torch.bfloat16).to(F64))
    # just above a tie in f64, below f32 resolution: through f32 it would round to even (down), directly it goes up
    t = torch.tensor([1.00390625 + 2.0 ** -40, 2.0 ** -127 + 2.0 ** -134 + 2.0 ** -170], dtype=F64)
    assert torch.equal(R.round_f64_to_bf16(t), torch.tensor([1.0078125, 2.0 ** -127 + 2.0 ** -133], dtype=F64))


@pytest.mark.parametrize("dy_bf16", [False, True])
@pytest.mark.parametrize("name", R.ACTS)
def test_dact_numpy_f32_emulation_stays_under_the_mismatch_cap(name, dy_bf16):
    """The f32 pipeline of dact_kernel (act' in f32 - for GELU the A&S emulation, below x = -4 the Mills-ratio form of
    gelu_grad_tail -, one f32 product, RNE to bf16) on the activation grid against bf16(f64 product): never outside the
    tolerance interval; bits equal to the reference's or one bf16 step away, the differing ones capped at 0.1 % of the
    grid.  Measured: GELU 4 (f32 dy) / 9 (bf16 dy) of 60 009 differ, each by one step; relu / celu / softplus none.
    (With the A&S form alone 8096 differ, 5686 by more than a step: its absolute error of 1.5e-7 is per cents of
    GELU'(x) below x = -4.)"""
    x = R.act_grid()
    aux = x.to(torch.bfloat16)
    dy = _randn((x.numel(),), 5, torch.float32)
    d = dy.to(torch.bfloat16).float() if dy_bf16 else dy
    g = R.dact_gelu_grad_as_f32(aux.float()) if name == "gelu" else R.act_grad(aux.float(), name).float()
    bits = R.bf16_rne_bits(R.f32_bits(d * g))
    outside, differ, far = R.dact_check(bits, dy, aux, name, dy_bf16)
    print(f"{name} dy_bf16={dy_bf16}: outside {outside}, differ {differ}, more than one step {far} of {x.numel()}")
    assert outside == 0
    assert far == 0
    assert differ <= 0.001 * x.numel()


def test_axpby_and_colsum():
    a, b = _randn((1000,), 6), _randn((1000,), 7)
    assert torch.allclose(R.axpby(a, b, 0.37), torch.add(a, b, alpha=0.37), rtol=1e-15, atol=1e-16)
    assert torch.equal(R.axpby(None, b, 0.37), 0.37 * b)
    x = _randn((113, 17), 8)
    s, sa = R.colsum(x)
    assert torch.equal(s, x.sum(0)) and torch.equal(sa, x.abs().sum(0))


def test_embedding_equals_f_embedding_with_autograd():
    B, L, V, d = 3, 7, 40, 12
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, V, (B, L), generator=g)
    ids[1, 2] = 5
    table = _randn((V, d), 10).requires_grad_(True)
    rs = torch.tensor([0.88, 1.0, 1.1], dtype=F64)
    mask = (torch.rand(B, L, generator=g) > 0.3).to(torch.uint8)
    w = rs.view(B, 1, 1) * mask.unsqueeze(-1) * (ids != 5).unsqueeze(-1)
    x = F.embedding(ids, table) * w
    dx = _randn((B, L, d), 11)
    (dt,) = torch.autograd.grad((x * dx).sum(), table)
    assert torch.equal(R.embed_fwd(ids, table.detach(), rs, mask, 5), x.detach())
    got, scale = R.embed_bwd(ids, dx, V, rs, mask, 5)
    assert torch.allclose(got, dt, rtol=1e-14, atol=1e-15) and (scale >= got.abs() - 1e-15).all()
    # plain form, and ids outside the table: NaN rows forward, nothing backward
    assert torch.equal(R.embed_fwd(ids, table.detach()), F.embedding(ids, table).detach())
    bad = ids.clone()
    bad[0, 0], bad[2, 3], bad[1, 1] = -1, V, 2 ** 32 + 3
    xb = R.embed_fwd(bad, table.detach())
    ok = (bad >= 0) & (bad < V)
    assert torch.isnan(xb[~ok]).all() and torch.equal(xb[ok], F.embedding(ids, table).detach()[ok])
    keep = ok.to(F64).unsqueeze(-1)
    want = torch.zeros(V, d, dtype=F64).index_add_(0, ids.view(-1), (dx * keep).view(B * L, d))
    assert torch.allclose(R.embed_bwd(bad, dx, V)[0], want, rtol=1e-14, atol=1e-15)


@pytest.mark.parametrize("masked", [False, True])
def test_pooling_equals_torch_with_autograd(masked):
    B, L, d = 4, 9, 8
    x = _randn((B, L, d), 12).requires_grad_(True)
    dy = _randn((B, d), 13)
    mask = None
    m = torch.ones(B, L, dtype=F64)
    if masked:
        mask = (torch.arange(L)[None] < torch.tensor([9, 4, 0, 1])[:, None]).to(torch.uint8)     # sequence 2: no token
        m = mask.to(F64)
    y0 = x[:, 0]
    n = m.sum(1, keepdim=True)
    y1 = (x * m.unsqueeze(-1)).sum(1) / n.clamp(min=1.0)
    for mode, y in ((0, y0), (1, y1)):
        (dx,) = torch.autograd.grad((y * dy).sum(), x, retain_graph=True)
        assert torch.allclose(R.pool_fwd(x.detach().view(B * L, d), B, L, mask, mode), y.detach(), rtol=1e-15, atol=0)
        assert torch.allclose(R.pool_bwd(dy, B, L, mask, mode), dx, rtol=1e-15, atol=0)
    if masked:
        assert (R.pool_fwd(x.detach(), B, L, mask, 1)[2] == 0).all() and (R.pool_bwd(dy, B, L, mask, 1)[2] == 0).all()


def test_l2norm_equals_f_normalize_with_autograd_including_the_clamp():
    x = _randn((6, 16), 14)
    x[1] = 0.0
    x[2] *= 1e-13 / x[2].norm()                            # below eps: the clamp is active
    x = x.requires_grad_(True)
    dy = _randn((6, 16), 15)
    y = F.normalize(x, dim=-1, eps=1e-12)
    (dx,) = torch.autograd.grad((y * dy).sum(), x)
    ry, rn, rdx = R.l2norm(x.detach(), dy, 1e-12)
    assert torch.allclose(ry, y.detach(), rtol=1e-14, atol=0) and torch.allclose(rn, x.detach().norm(dim=-1), rtol=1e-14, atol=0)
    keep = [0, 3, 4, 5]
    assert torch.allclose(rdx[keep], dx[keep], rtol=1e-12, atol=1e-14)
    # inside the clamp y = x / eps exactly: dx = dy / eps.  (autograd of clamp_min passes the norm's gradient through at
    # a zero row as 0 and differentiates the 1e-13 row as clamped: both give dy / eps.)
    assert torch.allclose(rdx[[1, 2]], dy[[1, 2]] / 1e-12, rtol=1e-14, atol=0)
    assert torch.allclose(dx[[1, 2]], dy[[1, 2]] / 1e-12, rtol=1e-12, atol=0)


@pytest.mark.parametrize("grad_scale,gnorm", [(1.0, 30.0), (0.125, 30.0), (1.0, 0.5)])
def test_adamw_step_equals_torch_adamw_after_clip_grad_norm(grad_scale, gnorm):
    """Three steps; (1, 0.5): the coefficient clamps to 1 (nothing clipped); 1/8: the clipped norm is the scaled one."""
    n = 1000
    w0, g = _randn((n,), 16), _randn((n,), 17)
    g = g * (gnorm / g.norm())
    g[:3] = 0.0                                             # v = 0: the denominator is eps
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    p = torch.nn.Parameter(w0.clone())
    opt = torch.optim.AdamW([p], **hp)
    w, m, v = w0.clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for step in (1, 2, 3):
        p.grad = g * grad_scale
        torch.nn.utils.clip_grad_norm_([p], 1.0)
        opt.step()
        w, m, v = R.adamw_step(w, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, max_norm=1.0, grad_scale=grad_scale)
        assert torch.allclose(w, p.detach(), rtol=1e-12, atol=1e-14), (w - p.detach()).abs().max()
        assert torch.isfinite(w).all()
    # without clipping
    p2 = torch.nn.Parameter(w0.clone())
    opt2 = torch.optim.AdamW([p2], **hp)
    p2.grad = g.clone()
    opt2.step()
    w2, _, _ = R.adamw_step(w0, g, torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64), 1e-3, 0.9, 0.999, 1e-8, 0.01, 1)
    assert torch.allclose(w2, p2.detach(), rtol=1e-12, atol=1e-14)
    assert abs(R.sumsq(g) - float((g * g).sum())) <= 1e-12 * R.sumsq(g)
