"""GPU: the fused Sinkhorn kernels (include/clipk.h: clipk_sim_lse_bias, clipk_sinkhorn_apply; ops.sim_lse_bias,
ops.sinkhorn_apply) and clip_dplm_amd.ot on top of them against the restatement of tests/sinkhorn_ref.py.

Tolerance rule of every comparison (`_close`): the f64 restatement, run for the same number of iterations, is the
reference; the kernel may deviate from it by at most 8 x the deviation of the f32 restatement on the same inputs (the
factor covers the different summation order), with a floor of 64 * 2^-24 x the quantity's magnitude (the largest
entry of the reference).  A wrong formula is off by 1e-2 or more.  The measured deviations
are printed before each assertion.  Potentials are compared after removing the gauge (u + c, v - c give the same plan)."""
import math

import pytest
import torch

from clip_dplm_amd import icnn, ops, ot

import sinkhorn_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F64, F32 = torch.float64, torch.float32


def _close(name, got, r64, r32):
    got, r64, r32 = (torch.as_tensor(t).detach().double().cpu() for t in (got, r64, r32))
    assert got.shape == r64.shape, (name, got.shape, r64.shape)
    assert torch.isfinite(got).all(), name
    dev_k, dev_32 = float((got - r64).abs().max()), float((r32 - r64).abs().max())
    mag = float(r64.abs().max())
    bound = max(8 * dev_32, 64 * U * mag)
    print(f"{name}: kernel {dev_k:.3e}  f32 restatement {dev_32:.3e}  magnitude {mag:.3e}  bound {bound:.3e}")
    assert dev_k <= bound, (name, dev_k, bound)


def _gauge(u, v, eps=None):
    """(u - c, v + c) with c = (mean u - mean v) / 2: the representative with equal means (times eps for the duals)."""
    c = (u.double().mean() - v.double().mean()) / 2
    return u.double() - c, v.double() + c


def _scalar(v, dev):
    return torch.tensor([v], dtype=F32, device=dev)


# ------------------------------------------------------------------------------------------------ 1: half-iteration
@pytest.mark.parametrize("P", [4, 60, 512, 768])
@pytest.mark.parametrize("Ny", [1, 63, 4097, 100003])
def test_half_iteration(dev, P, Ny):
    """ops.sim_lse_bias: rows are independent, so the reference of 1000 queries serves Mx = 1, 63, 65, 1000.  Random
    bias of spread +-20 and random logw; with prev: the averaged update and the error scalar; two runs bit-identical."""
    g = torch.Generator().manual_seed(1000 * P + Ny)
    x_all, y = ref.unit_clouds(1000, Ny, P, 7 * P + Ny)
    scale = 10.0
    bias = (torch.rand(Ny, generator=g, dtype=F64) * 40 - 20).float()
    logw = torch.randn(1000, generator=g, dtype=F64).float() - 5
    nv64 = ref.half_iteration(x_all.double(), y.double(), scale, bias.double(), logw.double())
    nv32 = ref.half_iteration(x_all, y, scale, bias, logw)
    nb64 = ref.half_iteration(x_all.double(), y.double(), scale)                 # no bias, no logw
    nb32 = ref.half_iteration(x_all, y, scale)
    prev = (nv64 + 0.1 * torch.randn(1000, generator=g, dtype=F64)).float()
    yd, bd, sd = y.to(dev), bias.to(dev), _scalar(scale, dev)
    split_seen = False
    for Mx in (1, 63, 65, 1000):
        tag = f"Mx={Mx} Ny={Ny} P={P}"
        xd, lwd, pvd = x_all[:Mx].to(dev), logw[:Mx].to(dev), prev[:Mx].to(dev)
        nqb, ks = ops.sim_lse_bias_plan(Mx, Ny)
        assert nqb == (Mx + 63) // 64 and 1 <= ks <= (Ny + 63) // 64
        split_seen |= ks > 1
        out = ops.sim_lse_bias(xd, yd, sd, bias=bd, logw=lwd)
        _close(f"lse {tag}", out, nv64[:Mx], nv32[:Mx])
        _close(f"lse (no bias, no logw) {tag}", ops.sim_lse_bias(xd, yd, sd), nb64[:Mx], nb32[:Mx])
        assert torch.equal(out, ops.sim_lse_bias(xd, yd, sd, bias=bd, logw=lwd)), tag
        # with prev: averaged, the error added onto what the scalar held; in place (prev == out) gives the same bits
        err = torch.zeros(1, dtype=F32, device=dev)
        avg = ops.sim_lse_bias(xd, yd, sd, bias=bd, logw=lwd, prev=pvd, average=True, err=err)
        p64 = prev[:Mx].double()
        _close(f"averaged {tag}", avg, 0.5 * (p64 + nv64[:Mx]), 0.5 * (prev[:Mx] + nv32[:Mx]))
        e64 = ref.marginal_error_term(logw[:Mx].double(), p64, nv64[:Mx])
        e32 = ref.marginal_error_term(logw[:Mx], prev[:Mx], nv32[:Mx])
        _close(f"error scalar {tag}", err[0], e64, e32)
        err2 = torch.full((1,), 0.5, dtype=F32, device=dev)
        inplace = pvd.clone()
        ops.sim_lse_bias(xd, yd, sd, bias=bd, logw=lwd, prev=inplace, average=True, out=inplace, err=err2)
        assert torch.equal(inplace, avg) and torch.equal(err2, err + 0.5), tag
        plain = ops.sim_lse_bias(xd, yd, sd, bias=bd, logw=lwd, prev=pvd)         # prev without averaging: the plain update
        assert torch.equal(plain, out), tag
    if Ny >= 4097:
        assert split_seen, "no shape of this case splits the key range"


# ------------------------------------------------------------------------------------------------ 2: plan sums
def _apply_all(xd, yd, sd, ud, vd, nxd, nyd):
    mass, bary, cost = ops.sinkhorn_apply(xd, yd, sd, ud, vd, nxd, nyd)
    # each output alone (the others null) gives the same bits
    m1, b0, c0 = ops.sinkhorn_apply(xd, yd, sd, ud, vd, want_bary=False, want_cost=False)
    assert b0 is None and c0 is None and torch.equal(m1, mass)
    m0, b1, c0 = ops.sinkhorn_apply(xd, yd, sd, ud, vd, want_mass=False, want_cost=False)
    assert m0 is None and c0 is None and torch.equal(b1, bary)
    m0, b0, c1 = ops.sinkhorn_apply(xd, yd, sd, ud, vd, nxd, nyd, want_mass=False, want_bary=False)
    assert m0 is None and b0 is None and torch.equal(c1, cost)
    return mass, bary, cost


@pytest.mark.parametrize("P", [4, 60, 512])
@pytest.mark.parametrize("Ny", [1, 63, 4097, 100003])
def test_plan_sums(dev, P, Ny):
    """ops.sinkhorn_apply with (a) arbitrary, non-converged potentials - rows independent: one reference of 1000 rows
    serves every Mx - and (b) the potentials of the f64 restatement after 20 iterations, per Mx."""
    g = torch.Generator().manual_seed(77 * P + Ny)
    x_all, y = ref.unit_clouds(1000, Ny, P, 3 * P + Ny)
    if Ny > 4097:                                   # the restatement of 1000 x 100003 problems on the device: seconds less
        x_all, y = x_all.to(dev), y.to(dev)
    rdev = x_all.device
    eps = 0.5
    scale = 2.0 / eps
    yd, sd = y.to(dev), _scalar(scale, dev)
    nyd = (yd * yd).sum(1)
    u_all = (torch.randn(1000, generator=g, dtype=F64) - math.log(1000)).float().to(rdev)
    v = (torch.randn(Ny, generator=g, dtype=F64) - math.log(Ny) - scale).float().to(rdev)
    r64 = ref.plan_sums(x_all.double(), y.double(), scale, u_all.double(), v.double())
    r32 = ref.plan_sums(x_all, y, scale, u_all, v)
    S_all = scale * (x_all.double() @ y.double().T)
    for Mx in (1, 63, 65, 1000):
        tag = f"Mx={Mx} Ny={Ny} P={P}"
        xd = x_all[:Mx].to(dev)
        nxd = (xd * xd).sum(1)
        got = _apply_all(xd, yd, sd, u_all[:Mx].to(dev), v.to(dev), nxd, nyd)
        for name, k, a, b in zip(("mass", "bary", "cost"), got, r64, r32):
            _close(f"{name} (arbitrary potentials) {tag}", k, a[:Mx], b[:Mx])
        # (b) 20 iterations of the restatement in f64 on the scaled similarity of these rows
        S = S_all[:Mx]
        loga = torch.full((Mx,), -math.log(Mx), dtype=F64, device=rdev)
        logb = torch.full((Ny,), -math.log(Ny), dtype=F64, device=rdev)
        vv = logb
        for _ in range(20):
            uu = loga - torch.logsumexp(S + vv[None, :], dim=1)
            vv = logb - torch.logsumexp(S + uu[:, None], dim=0)
        uf, vf = uu.float(), vv.float()                      # what the kernel is given; the references read the same values
        c64 = ref.plan_sums(x_all[:Mx].double(), y.double(), scale, uf.double(), vf.double())
        c32 = ref.plan_sums(x_all[:Mx], y, scale, uf, vf)
        got = _apply_all(xd, yd, sd, uf.to(dev), vf.to(dev), nxd, nyd)
        for name, k, a, b in zip(("mass", "bary", "cost"), got, c64, c32):
            _close(f"{name} (20 iterations) {tag}", k, a, b)
        print(f"mass total {float(got[0].double().sum()):.9f}")


# ------------------------------------------------------------------------------------------------ 3, 4: full solves
def _check_solve(r, r64, r32, tag, symmetric=False):
    _close(f"marginal_error {tag}", r.marginal_error, ref.marginal_error(r64), ref.marginal_error(r32))
    _close(f"value {tag}", r.value, r64.value, r32.value)
    _close(f"eps {tag}", r.eps, r64.eps, r32.eps)
    _close(f"cost {tag}", r.cost(), ref.transport_cost(r64), ref.transport_cost(r32))
    _close(f"barycentric_map {tag}", r.barycentric_map(), ref.barycentric_map(r64), ref.barycentric_map(r32))
    rows, cols = r.marginals()
    _close(f"row marginal {tag}", rows, ref.plan(r64).sum(1), ref.plan(r32).sum(1))
    _close(f"column marginal {tag}", cols, ref.plan(r64).sum(0), ref.plan(r32).sum(0))
    if symmetric:
        assert r.v is r.u and r.g is r.f
        _close(f"u {tag}", r.u, r64.u, r32.u)
        _close(f"f {tag}", r.f, r64.f, r32.f)
        return
    (uk, vk), (u64, v64), (u32, v32) = _gauge(r.u, r.v), _gauge(r64.u, r64.v), _gauge(r32.u, r32.v)
    _close(f"u {tag}", uk, u64, u32)
    _close(f"v {tag}", vk, v64, v32)
    (fk, gk), (f64, g64), (f32, g32) = _gauge(r.f, r.g), _gauge(r64.f, r64.g), _gauge(r32.f, r32.g)
    _close(f"f {tag}", fk, f64, f32)
    _close(f"g {tag}", gk, g64, g32)


SOLVE_SHAPES = [(130, 257, 64), (1000, 1000, 128), (65, 4097, 60)]


@pytest.mark.parametrize("uniform", [True, False])
@pytest.mark.parametrize("eps", [0.5, 0.05])
@pytest.mark.parametrize("M,N,P", SOLVE_SHAPES)
def test_full_solve_unit_vectors(dev, M, N, P, eps, uniform):
    x, y = ref.unit_clouds(M, N, P, M + N + P)
    a, b = (None, None) if uniform else (ref.random_weights(M, 1), ref.random_weights(N, 2))
    r64 = ref.solve(x, y, eps, a=a, b=b, n_iters=100)
    r32 = ref.solve(x, y, eps, a=a, b=b, n_iters=100, dtype=F32)
    e64 = float(ref.marginal_error(r64))
    # (f32 weights sum to 1 only to rounding: the row error cannot fall below the difference of the two sums)
    gap = 0.0 if uniform else abs(float(a.double().sum() - b.double().sum()))
    print(f"f64 restatement marginal error after 100 iterations: {e64:.3e} (weight sums differ by {gap:.3e})")
    assert e64 <= 1e-11 + 2 * gap
    ad, bd = (None, None) if uniform else (a.to(dev), b.to(dev))
    r = ot.sinkhorn(x.to(dev), y.to(dev), eps=eps, a=ad, b=bd, n_iters=100, tol=None)
    assert r.n_iters == 100
    _check_solve(r, r64, r32, f"M={M} N={N} P={P} eps={eps} uniform={uniform}")


@pytest.mark.parametrize("eps", [0.5, 0.05])
def test_symmetric_solve(dev, eps):
    """The averaged update of a cloud with itself: one potential, the restatement's symmetric iteration."""
    x, _ = ref.unit_clouds(257, 1, 64, 5)
    a = ref.random_weights(257, 3)
    r64 = ref.solve(x, x, eps, a=a, b=a, n_iters=100, symmetric=True)
    r32 = ref.solve(x, x, eps, a=a, b=a, n_iters=100, symmetric=True, dtype=F32)
    xd, ad = x.to(dev), a.to(dev)
    r = ot.sinkhorn(xd, xd, eps=eps, a=ad, b=ad, n_iters=100, tol=None, symmetric=True)
    _check_solve(r, r64, r32, f"symmetric eps={eps}", symmetric=True)


def test_unnormalised_inputs_relative_eps(dev):
    """Rows of norm about sqrt(512), as the transport maps' LayerNorm outputs; eps = 0.05 x the mean cost, which the
    product takes from the closed form and the restatement from the explicit matrix."""
    g = torch.Generator().manual_seed(11)
    M, N, P = 200, 300, 512
    x = torch.randn(M, P, generator=g)
    y = (torch.randn(N, P, generator=g, dtype=F64) * 0.9 + 0.2).float()
    r64 = ref.solve(x, y, None, eps_rel=0.05, n_iters=100)
    r32 = ref.solve(x, y, None, eps_rel=0.05, n_iters=100, dtype=F32)
    print(f"row norms {float(x.norm(dim=1).mean()):.2f}, eps {float(r64.eps):.4f}")
    r = ot.sinkhorn(x.to(dev), y.to(dev), eps=None, eps_rel=0.05, n_iters=100, tol=None)
    _check_solve(r, r64, r32, "unnormalised")


# ------------------------------------------------------------------------------------------------ 5: divergence
@pytest.mark.parametrize("eps", [0.5, 0.1])
@pytest.mark.parametrize("M,N,P", SOLVE_SHAPES)
def test_divergence_value_and_gradients(dev, M, N, P, eps):
    """Value and both gradients against f64 autograd THROUGH the 100 unrolled iterations of the restatement; the
    yardstick is the restatement's envelope gradient in f32.  The incoming gradient is 3, not 1."""
    x, y = ref.unit_clouds(M, N, P, 2 * M + N + P)
    a, b = ref.random_weights(M, 4), ref.random_weights(N, 5)
    if max(M, N) > 2048:                            # a 4097 x 4097 self problem unrolled under autograd: on the device
        x, y, a, b = x.to(dev), y.to(dev), a.to(dev), b.to(dev)
    x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
    d64 = ref.divergence(x64, y64, eps, a=a, b=b, n_iters=100)
    (3.0 * d64).backward()
    with torch.no_grad():
        d32, gx32, gy32, ot32 = ref.divergence_envelope_gradients(x, y, eps, a=a, b=b, n_iters=100, dtype=F32)
    xd, yd = x.to(dev).clone().requires_grad_(True), y.to(dev).clone().requires_grad_(True)
    d = ot.sinkhorn_divergence(xd, yd, eps=eps, a=a.to(dev), b=b.to(dev), n_iters=100, tol=None)
    (3.0 * d).backward()
    tag = f"M={M} N={N} P={P} eps={eps}"
    assert float(d64.detach()) > 1e-3
    _close(f"divergence {tag}", d, d64.detach(), d32)
    _close(f"d/dx {tag}", xd.grad, x64.grad, 3.0 * gx32)
    _close(f"d/dy {tag}", yd.grad, y64.grad, 3.0 * gy32)


def test_divergence_of_a_cloud_with_itself(dev):
    x, _ = ref.unit_clouds(130, 1, 64, 9)
    a = ref.random_weights(130, 6)
    xd, ad = x.to(dev).requires_grad_(True), a.to(dev)
    d = ot.sinkhorn_divergence(xd, xd, eps=0.1, a=ad, b=ad, n_iters=100, tol=None)
    d.backward()
    self64 = ref.solve(x, x, 0.1, a=a, b=a, n_iters=100, symmetric=True)
    gmag = float(ref.envelope_gradients(self64)[0].abs().max())
    print(f"S(x, x) = {float(d):.3e}, max |grad| = {float(xd.grad.abs().max()):.3e} (one term's gradient: {gmag:.3e})")
    assert abs(float(d)) <= 64 * U * float(self64.value.abs())
    assert float(xd.grad.abs().max()) <= 64 * U * gmag
    # an equal cloud in another tensor takes the general path (alternating cross term): the restatement's figure
    x2 = xd.detach().clone().requires_grad_(True)
    d2 = ot.sinkhorn_divergence(xd, x2, eps=0.1, a=ad, b=ad.clone(), n_iters=100, tol=None)
    d64 = ref.divergence(x, x.clone(), 0.1, a=a, b=a, n_iters=100)
    d32 = ref.divergence(x, x.clone(), 0.1, a=a, b=a, n_iters=100, dtype=F32)
    _close("divergence of equal clouds", d2, d64, d32)


def test_sinkhorn_loss_gradients(dev):
    """sinkhorn_loss: OT_eps itself, gradients against f64 autograd through the unrolled solve."""
    M, N, P = 130, 257, 64
    x, y = ref.unit_clouds(M, N, P, 21)
    x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
    v64 = ref.solve(x64, y64, 0.5, n_iters=100).value
    v64.backward()
    with torch.no_grad():
        r32 = ref.solve(x, y, 0.5, n_iters=100, dtype=F32)
        gx32, gy32 = ref.envelope_gradients(r32)
    xd, yd = x.to(dev).requires_grad_(True), y.to(dev).requires_grad_(True)
    v = ot.sinkhorn_loss(xd, yd, eps=0.5, n_iters=100, tol=None)
    v.backward()
    _close("loss", v, v64.detach(), r32.value)
    _close("loss d/dx", xd.grad, x64.grad, gx32)
    _close("loss d/dy", yd.grad, y64.grad, gy32)


# ------------------------------------------------------------------------------------------------ 6: stopping
def test_stops_on_tol(dev):
    M, N, P = 130, 257, 64
    x, y = ref.unit_clouds(M, N, P, 31)
    tol, every = 1e-4, 5
    r = ot.sinkhorn(x.to(dev), y.to(dev), eps=0.05, n_iters=1000, tol=tol, check_every=every)
    errs = [float(ref.marginal_error(ref.solve(x, y, 0.05, n_iters=k))) for k in (max(1, r.n_iters - 1 - every), r.n_iters - 1, r.n_iters)]
    print(f"stopped after {r.n_iters} iterations, marginal error {float(r.marginal_error):.3e}; f64 restatement after "
          f"{r.n_iters - 1 - every} / {r.n_iters - 1} / {r.n_iters} iterations: {errs[0]:.3e} / {errs[1]:.3e} / {errs[2]:.3e}")
    assert every < r.n_iters < 1000 and r.n_iters % every == 0
    # the check at iteration k reads the error of the plan after k - 1 iterations: below tol there, not yet a check earlier
    assert errs[1] < tol <= errs[0]
    assert float(r.marginal_error) < tol
    r64 = ref.solve(x, y, 0.05, n_iters=r.n_iters)
    r32 = ref.solve(x, y, 0.05, n_iters=r.n_iters, dtype=F32)
    _close("value at the stop", r.value, r64.value, r32.value)


# ------------------------------------------------------------------------------------------------ 7: graph capture
def test_fixed_iteration_solve_is_capturable(dev):
    """tol=None: no host read anywhere, so ten iterations are one linear chain of launches in a graph; replayed on new
    inputs copied into the captured buffers it gives the eager call's bits."""
    M, N, P = 130, 257, 64
    x0, y0 = ref.unit_clouds(M, N, P, 41)
    x1, y1 = ref.unit_clouds(M, N, P, 42)
    sx, sy = x0.to(dev), y0.to(dev)

    def run():
        r = ot.sinkhorn(sx, sy, eps=0.5, n_iters=10, tol=None)
        return r.u, r.v, r.value, r.marginal_error

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
        eager = ot.sinkhorn(xs.to(dev), ys.to(dev), eps=0.5, n_iters=10, tol=None)
        for got, want in zip(replayed, (eager.u, eager.v, eager.value, eager.marginal_error)):
            assert torch.equal(got, want)
    assert float(out[2]) > 0


# ------------------------------------------------------------------------------------------------ 8: transport maps
def test_evaluate_transport(dev):
    torch.manual_seed(5)
    m = icnn.SingleCellTransport(64, 64, icnn.ICNNConfig(input_dim=64, hidden_dims=[64, 32])).to(dev).eval()
    g = torch.Generator().manual_seed(8)
    src = torch.randn(300, 64, generator=g)
    tgt = torch.randn(300, 64, generator=g) * 0.8 + 0.3
    res = ot.evaluate_transport(m, src.to(dev), tgt.to(dev), batch_size=128, n_iters=100, tol=None)
    assert set(res) == {"mse", "sinkhorn_divergence", "identity_divergence"}
    with torch.no_grad():
        moved = torch.cat([m(src[i:i + 128].to(dev)) for i in range(0, 300, 128)]).cpu()
    per_batch = [float(((moved[i:i + 128].double() - tgt[i:i + 128].double()) ** 2).mean()) for i in range(0, 300, 128)]
    mse = sum(per_batch) / len(per_batch)
    print(f"mse {res['mse']:.6f} (restated {mse:.6f})")
    assert abs(res["mse"] - mse) <= 1e-5 * mse
    for key, cloud in (("sinkhorn_divergence", moved), ("identity_divergence", src)):
        d64 = ref.divergence(cloud, tgt, None, n_iters=100)
        d32 = ref.divergence(cloud, tgt, None, n_iters=100, dtype=F32)
        _close(key, torch.tensor(res[key]), d64, d32)
    assert res["sinkhorn_divergence"] > 0 and res["identity_divergence"] > 0
    assert icnn.compute_transport_error(m, src.to(dev), tgt.to(dev), 128) == res["mse"]
