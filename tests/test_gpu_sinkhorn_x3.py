"""GPU: the bf16x3 Sinkhorn half-iteration (include/clipk.h: clipk_sim_lse_bias_x3; ops.sim_lse_bias_x3) and
ot.sinkhorn(..., precision="bf16x3") on top of it, against the f64 restatement of tests/sinkhorn_x3_ref.py.

Bounds (none taken from what the kernel gives; u = 2^-24):
  * half-iteration against the f64 LSE over the SPLIT products: row i may deviate by
        scale (accumulation term of eps_rel) |x_i| max|y|  +  64 u magnitude_i,
    the first for the f32 accumulation of the 3 P exact bf16 products in the MFMA (include/clipk.h, "Certificate"), the
    second for the f32 arithmetic of the running (max, sum) and the finalize, magnitude_i = the largest of |logit_ij|,
    |logw_i| and |nv_i| of the row (the floor of test_gpu_sinkhorn.py, per row);
  * half-iteration against the f64 LSE over the TRUE products: eta = max_i eta_i of the rows in the call;
  * solves: the three bounds DESIGN.md derives, which tests/test_sinkhorn_x3_host.py re-checks in f64.
The measured / bound ratios are printed before each assertion."""
import math

import pytest
import torch

from clip_dplm_amd import flow, ops, ot

import sinkhorn_ref as ref
import sinkhorn_x3_ref as x3

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F64, F32 = torch.float64, torch.float32


def _scalar(v, dev):
    return torch.tensor([v], dtype=F32, device=dev)


def _planes(t):
    hi = torch.empty((t.shape[0], ops.plane_pitch(t.shape[1])), dtype=torch.bfloat16, device=t.device)
    lo = torch.empty_like(hi)
    ops.split_bf16(t, hi, lo)
    return hi, lo


def _ratio(name, got, want, bound):
    """max_i |got - want| / bound_i, printed; got must be finite."""
    got, want = got.detach().double().cpu().reshape(-1), torch.as_tensor(want).detach().double().cpu().reshape(-1)
    bound = torch.as_tensor(bound, dtype=F64).cpu().reshape(-1).expand_as(want)
    assert got.shape == want.shape and torch.isfinite(got).all(), name
    dev_ = (got - want).abs()
    # a row whose bound is zero (a zero query against one key, no bias) must be met exactly
    r = float(torch.where(bound > 0, dev_ / bound.clamp_min(1e-300), torch.where(dev_ == 0, 0.0, math.inf)).max())
    print(f"{name}: measured / bound = {r:.3e}  (largest deviation {float((got - want).abs().max()):.3e})")
    return r


def _close(name, got, r64, r32):
    """The tolerance rule of test_gpu_sinkhorn.py: 8 x the f32 restatement's deviation, floor 64 u x magnitude."""
    got, r64, r32 = (torch.as_tensor(t).detach().double().cpu() for t in (got, r64, r32))
    dev_k, dev_32 = float((got - r64).abs().max()), float((r32 - r64).abs().max())
    bound = max(8 * dev_32, 64 * U * float(r64.abs().max()))
    print(f"{name}: kernel {dev_k:.3e}  f32 restatement {dev_32:.3e}  bound {bound:.3e}")
    assert torch.isfinite(got).all() and dev_k <= bound, (name, dev_k, bound)


# ------------------------------------------------------------------------------------------------ 1: half-iteration
def _half_inputs(P, Ny, rdev):
    """1000 query rows of norms 0.01 ... 100 (log-uniform; rows 0, 1, 2 have norms 100, 0.01 and 0, so that every Mx > 2
    holds the extremes and eta = max_i eta_i is that of the norm-100 row in every call), Ny unit keys, bias of spread
    +-20, random logw, and the noise that makes `prev` of the updated potential."""
    g = torch.Generator().manual_seed(1000 * P + Ny)
    x, y = ref.unit_clouds(1000, Ny, P, 7 * P + Ny)
    norms = 10.0 ** (torch.rand(1000, generator=g, dtype=F64) * 4 - 2)
    norms[0], norms[1], norms[2] = 100.0, 0.01, 0.0
    x = (x.double() * norms[:, None]).float()
    bias = (torch.rand(Ny, generator=g, dtype=F64) * 40 - 20).float()
    logw = torch.randn(1000, generator=g, dtype=F64).float() - 5
    noise = 0.1 * torch.randn(1000, generator=g, dtype=F64)
    x, y, bias, logw, noise = (t.to(rdev) for t in (x, y, bias, logw, noise))
    return x, y, bias, logw, noise


@pytest.mark.parametrize("P", [4, 60, 512, 768])
@pytest.mark.parametrize("Ny", [1, 63, 129, 4097, 20011])
def test_half_iteration(dev, P, Ny):
    """Rows are independent, so one reference of 1000 queries serves Mx = 1, 127, 129 (the 128-query block's edges) and
    1000.  The f64 references of the two largest key counts are formed on the device (seconds less per case)."""
    scale = 10.0
    rdev = dev if Ny >= 4097 else torch.device("cpu")
    x, y, bias, logw, noise = _half_inputs(P, Ny, rdev)
    A = scale * x3.product(x, y) + bias.double()[None, :]                  # split logits, f64
    T = scale * (x.double() @ y.double().T) + bias.double()[None, :]       # true logits, f64
    lseA, lseT = torch.logsumexp(A, dim=1), torch.logsumexp(T, dim=1)
    xn, yn = x.double().norm(dim=1), float(y.double().norm(dim=1).max())
    # the same rows without bias and logw
    lseA0 = torch.logsumexp(A - bias.double()[None, :], dim=1)
    mag0 = torch.maximum((A - bias.double()[None, :]).abs().amax(1), lseA0.abs())
    nvA, nvT = logw.double() - lseA, logw.double() - lseT
    mag = torch.maximum(torch.maximum(A.abs().amax(1), logw.double().abs()), nvA.abs())
    acc = scale * x3.accumulation_term(P) * xn * yn
    b_split, b_split0 = acc + 64 * U * mag, acc + 64 * U * mag0
    eta_i = scale * xn * yn * x3.eps_rel(P) + (scale * P * (xn + yn + 1.0) + 1.0) * 2.0 ** -120
    prev = (nvA + noise).float()
    xd, yd, bd, lwd, sd = x.to(dev), y.to(dev), bias.to(dev), logw.to(dev), _scalar(scale, dev)
    yh, yl = _planes(yd)
    split_seen = False
    for Mx in (1, 127, 129, 1000):
        tag = f"Mx={Mx} Ny={Ny} P={P}"
        xh, xl = _planes(xd[:Mx].contiguous())
        nqb, ks = ops.sim_lse_bias_x3_plan(Mx, Ny)
        assert nqb == (Mx + 127) // 128 and 1 <= ks <= (Ny + 63) // 64
        split_seen |= ks > 1
        lw, pv = lwd[:Mx].contiguous(), prev[:Mx].to(dev).contiguous()
        out = ops.sim_lse_bias_x3(xh, xl, yh, yl, P, sd, bias=bd, logw=lw)
        assert _ratio(f"lse vs split products {tag}", out, nvA[:Mx], b_split[:Mx]) <= 1.0
        eta = float(eta_i[:Mx].max())
        assert _ratio(f"lse vs true products (eta = {eta:.3e}) {tag}", out, nvT[:Mx], eta) <= 1.0
        # and per row: eta_i for the products (LSE is non-expansive), the floor above for the f32 arithmetic of the LSE
        assert _ratio(f"lse vs true products, per row {tag}", out, nvT[:Mx], eta_i[:Mx] + 64 * U * mag[:Mx]) <= 1.0
        bare = ops.sim_lse_bias_x3(xh, xl, yh, yl, P, sd)
        assert _ratio(f"lse (no bias, no logw) {tag}", bare, -lseA0[:Mx], b_split0[:Mx]) <= 1.0
        assert torch.equal(out, ops.sim_lse_bias_x3(xh, xl, yh, yl, P, sd, bias=bd, logw=lw)), tag      # reruns: same bits
        # with prev: averaged, the error added onto what the scalar held; in place (prev == out) gives the same bits
        err = torch.zeros(1, dtype=F32, device=dev)
        avg = ops.sim_lse_bias_x3(xh, xl, yh, yl, P, sd, bias=bd, logw=lw, prev=pv, average=True, err=err)
        p64 = prev[:Mx].double()
        assert _ratio(f"averaged {tag}", avg, 0.5 * (p64 + nvA[:Mx]), 0.5 * b_split[:Mx] + 2 * U * mag[:Mx]) <= 1.0
        # error scalar: | |e^{d + t} - 1| - |e^d - 1| | <= e^d (e^{|t|} - 1) per row, d = prev - nv, |t| <= the row's bound;
        # 64 u of the summed magnitudes for the f32 arithmetic of the terms and their sum
        w, d = logw[:Mx].double().exp(), p64 - nvA[:Mx]
        e64 = (w * (d.exp() - 1).abs()).sum()
        eb = (w * d.exp() * torch.expm1(b_split[:Mx])).sum() + 64 * U * (w * (d.exp() + 1)).sum()
        assert _ratio(f"error scalar {tag}", err, e64, eb) <= 1.0
        err2 = torch.full((1,), 0.5, dtype=F32, device=dev)
        inplace = pv.clone()
        ops.sim_lse_bias_x3(xh, xl, yh, yl, P, sd, bias=bd, logw=lw, prev=inplace, average=True, out=inplace, err=err2)
        assert torch.equal(inplace, avg) and torch.equal(err2, err + 0.5), tag
        plain = ops.sim_lse_bias_x3(xh, xl, yh, yl, P, sd, bias=bd, logw=lw, prev=pv)   # prev without averaging
        assert torch.equal(plain, out), tag
    if Ny >= 4097:
        assert split_seen, "no shape of this case splits the key range"


def test_half_iteration_tiny_magnitudes(dev):
    """Clouds of magnitude 1e-30: the products vanish (the lo plane is subnormal or flushed), the result is finite and
    the LSE of the bias to within eta and the f32 floor."""
    P, Ny, Mx, scale = 60, 63, 129, 10.0
    x, y, bias, logw, _ = _half_inputs(P, Ny, torch.device("cpu"))
    x, y = (x[:Mx] * 1e-30).contiguous(), (y * 1e-30).contiguous()
    xh, xl = _planes(x.to(dev))
    yh, yl = _planes(y.to(dev))
    out = ops.sim_lse_bias_x3(xh, xl, yh, yl, P, _scalar(scale, dev), bias=bias.to(dev), logw=logw[:Mx].to(dev))
    want = logw[:Mx].double() - torch.logsumexp(bias.double(), dim=0)
    eta = x3.logit_error_bound(x, y, scale)
    assert eta < 1e-30
    assert _ratio("tiny magnitudes", out, want, eta + 64 * U * torch.maximum(want.abs(), bias.double().abs().max())) <= 1.0


# ------------------------------------------------------------------------------------------------ 2: full solves
# 100 split iterations + 1 exact one.  The f64 restatement's split iteration has a marginal error below 1e-7 after 25
# (eps = 0.5) or 50 (eps = 0.05) iterations at both shapes, uniform and weighted (measured on the CPU; asserted below for
# the 100 the tests run).
N_SPLIT = 100


def _check_split_solve(r, x, y, eps, a, b, tag, symmetric=False):
    r64 = x3.solve(x, y, eps, a=a, b=b, n_split=N_SPLIT, n_exact=1, symmetric=symmetric)
    print(f"{tag}: restatement's split marginal error after {N_SPLIT} iterations {r64.split_error:.3e}, eta {r64.eta:.3e}")
    assert r64.split_error < 1e-7
    exact = ref.solve(x, y, eps, a=a, b=b, n_iters=4 * N_SPLIT, symmetric=symmetric)
    assert float(ref.marginal_error(exact)) < 1e-7
    r32 = ref.solve(x, y, eps, a=a, b=b, n_iters=N_SPLIT + 1, symmetric=symmetric, dtype=F32)
    assert r.n_iters == N_SPLIT + 1 and r.precision == "bf16x3"
    eta = r64.eta
    got_eta = float(r.logit_error_bound)
    print(f"{tag}: logit_error_bound {got_eta:.6e}, restated {eta:.6e}")
    assert r.logit_error_bound.dim() == 0 and r.logit_error_bound.is_cuda
    assert eta * (1 - 1e-6) <= got_eta <= eta * (1 + 1e-5)       # the norms are rounded upward, the arithmetic is f32
    rows, cols = r.marginals()
    bound = math.expm1(2 * eta) + r64.split_error
    merr = float(r.marginal_error)
    row_l1 = float((rows.double().cpu() - r64.a).abs().sum())
    col_l1 = float((cols.double().cpu() - r64.b).abs().sum())
    print(f"{tag}: marginal_error {merr:.3e}, row marginal off {row_l1:.3e}, column marginal off {col_l1:.3e} (restatement's "
          f"row error {float(ref.marginal_error(r64)):.3e}), bound {bound:.3e}")
    assert 0 <= merr <= bound and row_l1 <= bound
    if symmetric:                                    # the averaged update: the plan is symmetric, columns as the rows
        assert col_l1 <= bound
    else:                                            # exact after the last (exact) v update: the f32 solve's tolerance
        _close(f"column marginal {tag}", cols, r64.b, ref.plan(r32).sum(0))
    assert _ratio(f"value {tag}", r.value, exact.value, 4 * eps * eta) <= 1.0
    if symmetric:
        assert r.v is r.u and r.g is r.f


@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("eps", [0.5, 0.05])
@pytest.mark.parametrize("M,N,P", [(300, 500, 64), (1000, 1000, 128)])
def test_full_solve(dev, M, N, P, eps, uniform):
    x, y = ref.unit_clouds(M, N, P, M + N + P)
    a, b = (None, None) if uniform else (ref.random_weights(M, 1), ref.random_weights(N, 2))
    ad, bd = (None, None) if uniform else (a.to(dev), b.to(dev))
    r = ot.sinkhorn(x.to(dev), y.to(dev), eps=eps, a=ad, b=bd, n_iters=N_SPLIT + 1, tol=None, precision="bf16x3")
    _check_split_solve(r, x, y, eps, a, b, f"M={M} N={N} P={P} eps={eps} uniform={uniform}")


@pytest.mark.parametrize("eps", [0.5, 0.05])
def test_symmetric_solve(dev, eps):
    x, _ = ref.unit_clouds(257, 1, 64, 5)
    a = ref.random_weights(257, 3)
    xd, ad = x.to(dev), a.to(dev)
    r = ot.sinkhorn(xd, xd, eps=eps, a=ad, b=ad, n_iters=N_SPLIT + 1, tol=None, symmetric=True, precision="bf16x3")
    _check_split_solve(r, x, x, eps, a, a, f"symmetric eps={eps}", symmetric=True)


# ------------------------------------------------------------------------------------------------ 3: stopping
@pytest.mark.parametrize("symmetric", [False, True])
def test_stops_on_tol(dev, symmetric):
    """Wherever the f32 solve returns with marginal_error < tol, the split solve does, by the same (exact) measure."""
    x, y = ref.unit_clouds(130, 257, 64, 31)
    tol = 1e-4
    xd = x.to(dev)
    yd = xd if symmetric else y.to(dev)
    kw = dict(eps=0.05, n_iters=1000, tol=tol, check_every=5, symmetric=symmetric)
    r32 = ot.sinkhorn(xd, yd, **kw)
    r = ot.sinkhorn(xd, yd, precision="bf16x3", **kw)
    print(f"symmetric={symmetric}: f32 stops after {r32.n_iters} iterations at {float(r32.marginal_error):.3e}; bf16x3 after "
          f"{r.n_iters} at {float(r.marginal_error):.3e}")
    assert float(r32.marginal_error) < tol and r32.n_iters < 1000
    assert float(r.marginal_error) < tol and 2 <= r.n_iters < 1000 and r.precision == "bf16x3"
    # n_iters = 2: the split phase ends at its first look (iteration 1 never looks), then one exact iteration
    r2 = ot.sinkhorn(xd, yd, precision="bf16x3", **dict(kw, n_iters=2))
    assert r2.n_iters == 2


# ------------------------------------------------------------------------------------------------ 4: graph capture
def test_fixed_iteration_split_solve_is_capturable(dev):
    """tol=None: two split launches, nine split iterations and one exact one are a linear chain of launches in a graph;
    replayed on new inputs copied into the captured buffers it gives the eager call's bits."""
    M, N, P = 130, 257, 64
    x0, y0 = ref.unit_clouds(M, N, P, 41)
    x1, y1 = ref.unit_clouds(M, N, P, 42)
    sx, sy = x0.to(dev), y0.to(dev)

    def run(xs=None, ys=None):
        r = ot.sinkhorn(sx if xs is None else xs, sy if ys is None else ys, eps=0.5, n_iters=10, tol=None, precision="bf16x3")
        return r.u, r.v, r.value, r.marginal_error, r.logit_error_bound

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph, keep = torch.cuda.CUDAGraph(), []
    with ops.owned_by_capture(keep), torch.cuda.graph(graph):
        out = run()
    for xs, ys in ((x1, y1), (x0, y0)):
        sx.copy_(xs.to(dev))
        sy.copy_(ys.to(dev))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in out]
        for got, want in zip(replayed, run(xs.to(dev), ys.to(dev))):
            assert torch.equal(got, want)
    assert float(out[2]) > 0 and float(out[4]) > 0


# ------------------------------------------------------------------------------------------------ 5: the default
def test_default_precision_is_unchanged(dev):
    x, y = ref.unit_clouds(130, 257, 64, 51)
    a, b = ref.random_weights(130, 1).to(dev), ref.random_weights(257, 2).to(dev)
    xd, yd = x.to(dev), y.to(dev)
    for kw in (dict(n_iters=20, tol=None), dict(n_iters=200, tol=1e-4, check_every=5), dict(n_iters=20, tol=None, a=a, b=b)):
        r0 = ot.sinkhorn(xd, yd, eps=0.05, **kw)
        r1 = ot.sinkhorn(xd, yd, eps=0.05, precision="f32", **kw)
        for n in ("u", "v", "f", "g", "value", "marginal_error", "eps"):
            assert torch.equal(getattr(r0, n), getattr(r1, n)), n
        assert r0.n_iters == r1.n_iters and r0.precision == r1.precision == "f32"
        assert float(r0.logit_error_bound) == 0.0 and r0.logit_error_bound.is_cuda
    r3 = ot.sinkhorn(xd, yd, eps=0.05, n_iters=20, tol=None, precision="bf16x3")
    assert not torch.equal(r3.u, r0.u) or not torch.equal(r3.v, r0.v)        # the split iterations did run


# ------------------------------------------------------------------------------------------------ 6: pass-through
def test_divergence_value_and_gradients(dev):
    """sinkhorn_divergence(..., precision="bf16x3") against the converged f64 restatement: three solves, each within
    4 eps eta of its OT_eps; row i's gradient within the sum of the two terms' gradient bounds."""
    M, N, P, eps = 300, 500, 64, 0.5
    x, y = ref.unit_clouds(M, N, P, 2 * M + N + P)
    a, b = ref.random_weights(M, 4), ref.random_weights(N, 5)
    d64, gx64, gy64, _ = ref.divergence_envelope_gradients(x, y, eps, a=a, b=b, n_iters=4 * N_SPLIT)
    xd, yd = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    d = ot.sinkhorn_divergence(xd, yd, eps=eps, a=a.to(dev), b=b.to(dev), n_iters=N_SPLIT + 1, tol=None, precision="bf16x3")
    d.backward()
    scale = 2.0 / eps
    e_xy, e_xx, e_yy = (x3.logit_error_bound(p, q, scale) for p, q in ((x, y), (x, x), (y, y)))
    assert _ratio("divergence", d, d64, 4 * eps * (e_xy + 0.5 * e_xx + 0.5 * e_yy)) <= 1.0
    xn, yn = x.double().norm(dim=1), y.double().norm(dim=1)
    bx = 2.0 * a.double() * (math.expm1(4 * e_xy) * (xn + yn.max()) + math.expm1(4 * e_xx) * (xn + xn.max()))
    by = 2.0 * b.double() * (math.expm1(4 * e_xy) * (yn + xn.max()) + math.expm1(4 * e_yy) * (yn + yn.max()))
    assert _ratio("d/dx rows", (xd.grad.double().cpu() - gx64).norm(dim=1), torch.zeros(M, dtype=F64), bx) <= 1.0
    assert _ratio("d/dy rows", (yd.grad.double().cpu() - gy64).norm(dim=1), torch.zeros(N, dtype=F64), by) <= 1.0
    assert float(d64) > 1e-3


def test_schrodinger_matcher_and_evaluate_transport_pass_precision(dev):
    g = torch.Generator().manual_seed(8)
    x0 = torch.randn(200, 64, generator=g).to(dev)
    x1 = (torch.randn(300, 64, generator=g) * 0.8 + 0.3).to(dev)
    m = flow.SchrodingerBridgeConditionalFlowMatcher(1.0, n_iters=20, precision="bf16x3")
    t, xt, ut, (i, j) = m.sample_location_and_conditional_flow(x0, x1, return_indices=True, seed=3)
    assert t.shape == (200,) and xt.shape == (200, 64) and ut.shape == (200, 64)
    assert i.shape == j.shape == (200,) and i.dtype == j.dtype == torch.int64
    assert int(i.min()) >= 0 and int(i.max()) < 200 and int(j.min()) >= 0 and int(j.max()) < 300
    assert torch.isfinite(xt).all() and torch.isfinite(ut).all()
    # evaluate_transport hands its keyword arguments to sinkhorn_divergence: the split solve's bits, not the f32 solve's
    tgt = x1[:200].contiguous()
    kw = dict(n_iters=30, tol=None)
    res = ot.evaluate_transport(lambda s: 0.8 * s + 0.3, x0, tgt, precision="bf16x3", **kw)
    res32 = ot.evaluate_transport(lambda s: 0.8 * s + 0.3, x0, tgt, **kw)
    assert res["sinkhorn_divergence"] == float(ot.sinkhorn_divergence(0.8 * x0 + 0.3, tgt, precision="bf16x3", **kw))
    assert res32["sinkhorn_divergence"] == float(ot.sinkhorn_divergence(0.8 * x0 + 0.3, tgt, **kw))
    print(f"evaluate_transport: sinkhorn_divergence {res['sinkhorn_divergence']:.7f} (f32 solve {res32['sinkhorn_divergence']:.7f})")
    assert math.isfinite(res["sinkhorn_divergence"]) and res["mse"] == res32["mse"]
