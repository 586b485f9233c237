"""GPU: the fused Gaussian-mixture kernel sums (include/clipk.h: clipk_kernel_sums; ops.kernel_sums) and
clip_dplm_amd.distribution on top of them against the restatement of tests/mmd_ref.py.

Tolerance rule of every comparison (`_close`, the rule of tests/test_gpu_sinkhorn.py): the f64 restatement (d2 from
coordinate differences) is the reference; the kernel may deviate from it by at most 8 x the deviation of the f32
restatement (d2 from the norm expansion, as in the kernel) on the same inputs - the factor covers the different
summation order - with a floor of 64 * 2^-24 x the quantity's magnitude (the largest entry of the reference).  The
measured deviations are printed before each assertion.  Inputs are unit-norm clouds with gammas in {0.25, 1, 4}: d2 lies
in [0, 4], the kernel values spread over (e^-16, 1], and a wrong formula is off by far more than the bound."""
import pytest
import torch

from clip_dplm_amd import distribution, ops

import mmd_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F64, F32 = torch.float64, torch.float32

# B = 1, 3, 8: gammas from {0.25, 1, 4}, unequal weights, one of them negative (the backward pass may pass any sign)
MIXTURES = {
    1: ([1.0], [0.75]),
    3: ([0.25, 1.0, 4.0], [0.5, -0.25, 1.0]),
    8: ([0.25, 1.0, 4.0, 0.25, 1.0, 4.0, 0.25, 1.0], [0.3, 0.2, -0.15, 0.1, 0.25, 0.05, 0.4, 0.35]),
}


def _close(name, got, r64, r32):
    got, r64, r32 = (torch.as_tensor(t).detach().double().cpu() for t in (got, r64, r32))
    assert got.shape == r64.shape, (name, got.shape, r64.shape)
    assert torch.isfinite(got).all(), name
    dev_k, dev_32 = float((got - r64).abs().max()), float((r32 - r64).abs().max())
    mag = float(r64.abs().max())
    bound = max(8 * dev_32, 64 * U * mag)
    print(f"{name}: kernel {dev_k:.3e}  f32 restatement {dev_32:.3e}  magnitude {mag:.3e}  bound {bound:.3e}")
    assert dev_k <= bound, (name, dev_k, bound)


def _vec(v, dev):
    return torch.tensor(v, dtype=F32, device=dev)


# ------------------------------------------------------------------------------------------------ 1: ops.kernel_sums
@pytest.mark.parametrize("P", [4, 60, 512])
@pytest.mark.parametrize("Ny", [1, 63, 65, 4097])
def test_kernel_sums(dev, P, Ny):
    """Rows are independent, so the distance matrices of 1000 queries (one in f64, one in f32) serve Mx = 1, 63, 65, 1000,
    every mixture and every diagonal offset.  ksum alone and ksum + kbary; diag_offset = Ny skips nothing and equals -1
    bit for bit; two runs bit-identical; Ny = 4097 splits the key range."""
    x_all, y = ref.unit_clouds(1000, Ny, P, 13 * P + Ny)
    if Ny > 65:                                     # the restatement of the 1000 x 4097 cases on the device: seconds less
        x_all, y = x_all.to(dev), y.to(dev)
    d64, d32 = ref.sq_dists(x_all.double(), y.double()), ref.sq_dists(x_all, y)
    yd = y.to(dev)
    nyd = (yd * yd).sum(1)
    split_seen = False
    for B, (gammas, weights) in MIXTURES.items():
        gd, wd = _vec(gammas, dev), _vec(weights, dev)
        plain = {}
        for diag in (-1, 0, 61, Ny):
            s64, b64 = ref.kernel_sums_from(d64, y.double(), gammas, weights, diag)
            s32, b32 = ref.kernel_sums_from(d32, y, gammas, weights, diag)
            for Mx in (1, 63, 65, 1000):
                tag = f"Mx={Mx} Ny={Ny} P={P} B={B} diag={diag}"
                nqb, ks = ops.kernel_sums_plan(Mx, Ny)
                assert nqb == (Mx + 63) // 64 and 1 <= ks <= (Ny + 63) // 64
                split_seen |= ks > 1
                xd = x_all[:Mx].to(dev)
                nxd = (xd * xd).sum(1)
                ksum, none = ops.kernel_sums(xd, yd, gd, wd, nxd, nyd, diag_offset=diag)
                assert none is None
                _close(f"ksum alone {tag}", ksum, s64[:Mx], s32[:Mx])
                ksum2, kbary = ops.kernel_sums(xd, yd, gd, wd, nxd, nyd, diag_offset=diag, want_bary=True)
                _close(f"ksum {tag}", ksum2, s64[:Mx], s32[:Mx])
                _close(f"kbary {tag}", kbary, b64[:Mx], b32[:Mx])
                none, kbary1 = ops.kernel_sums(xd, yd, gd, wd, diag_offset=diag, want_sum=False, want_bary=True)
                assert none is None and torch.equal(kbary1, kbary), tag          # (and the norms computed by the wrapper)
                again = ops.kernel_sums(xd, yd, gd, wd, nxd, nyd, diag_offset=diag, want_bary=True)
                assert torch.equal(again[0], ksum2) and torch.equal(again[1], kbary), tag
                assert torch.equal(ops.kernel_sums(xd, yd, gd, wd, nxd, nyd, diag_offset=diag)[0], ksum), tag
                if diag == -1:
                    plain[Mx] = (ksum, ksum2, kbary)
                if diag == Ny:                      # every skipped key is out of range
                    assert all(torch.equal(a, b) for a, b in zip(plain[Mx], (ksum, ksum2, kbary))), tag
    if Ny >= 4097:
        assert split_seen, "no shape of this case splits the key range"


# ------------------------------------------------------------------------------------------------ 2: the diagonal rule
def test_diagonal_is_dropped_not_subtracted(dev):
    """y is x, diag_offset = 0, B = 1, rows of norm 30: the computed d2_ii = nx_i + nx_i - 2 <x_i, x_i> is rounding noise of
    the size of an ulp of 1800 (~1e-4), not 0.  gamma = 1 / 1800 (one over the mean squared distance, the bandwidth such
    clouds are looked at with) makes the off-diagonal terms ~ e^-1 each and gamma d2_ii a few 2^-24, so that the full row
    sum minus the row sum without the diagonal is the weight to within 4 ulp of ksum: the right key is skipped, once."""
    M, P, w = 200, 64, 0.75
    g = torch.Generator().manual_seed(2)
    x = torch.nn.functional.normalize(torch.randn(M, P, generator=g, dtype=F64), dim=1).mul(30.0).float().to(dev)
    nx = (x * x).sum(1)
    gd, wd = _vec([1.0 / 1800.0], dev), _vec([w], dev)
    full, _ = ops.kernel_sums(x, x, gd, wd, nx, nx, diag_offset=-1)
    skip, _ = ops.kernel_sums(x, x, gd, wd, nx, nx, diag_offset=0)
    d2_ii = (2.0 * nx.double() - 2.0 * (x.double() * x.double()).sum(1)).abs().max()
    ulp = torch.exp2(torch.floor(torch.log2(full.double())) - 23)                     # spacing of f32 at each ksum
    dev_ulp = ((full.double() - skip.double() - w).abs() / ulp).max()
    print(f"diagonal rule: ksum in [{float(full.min()):.3f}, {float(full.max()):.3f}], |d2_ii| of f32 norms up to "
          f"{float(d2_ii):.3e}, (full - skipped - weight) up to {float(dev_ulp):.3f} ulp of ksum")
    assert float(dev_ulp) <= 4.0
    # gamma = 1: every off-diagonal term is exp(-~1800) = 0, so the skipped row sums are exactly 0 - no trace of the
    # computed d2_ii, which a sum formed in full and corrected by weight x 1 would leave (the full sums show it)
    g1 = _vec([1.0], dev)
    full1, _ = ops.kernel_sums(x, x, g1, wd, nx, nx, diag_offset=-1)
    skip1, sb1 = ops.kernel_sums(x, x, g1, wd, nx, nx, diag_offset=0, want_bary=True)
    print(f"diagonal rule, gamma = 1: {int((full1 != w).sum())} of {M} full sums differ from the weight (by up to "
          f"{float((full1 - w).abs().max()):.3e}); skipped sums: max |.| = {float(skip1.abs().max()):.3e}")
    assert torch.equal(skip1, torch.zeros_like(skip1)) and torch.equal(sb1, torch.zeros_like(sb1))


# ------------------------------------------------------------------------------------------------ 3: mmd2 value
GAMMAS = [0.25, 1.0, 4.0]


@pytest.mark.parametrize("M,N,P", [(2, 2, 4), (130, 67, 60), (1000, 4097, 128)])
def test_mmd2_value(dev, M, N, P):
    x, y = ref.unit_clouds(M, N, P, M + N + P)
    xd, yd = x.to(dev), y.to(dev)
    rx, ry = (xd, yd) if N > 1000 else (x, y)       # the 4097 x 4097 self block of the restatement on the device
    with torch.no_grad():
        for unbiased in (True, False):
            tag = f"M={M} N={N} P={P} unbiased={unbiased}"
            r64, r32 = ref.mmd2(rx, ry, GAMMAS, None, unbiased), ref.mmd2(rx, ry, GAMMAS, None, unbiased, dtype=F32)
            got = distribution.mmd2(xd, yd, gammas=GAMMAS, unbiased=unbiased)
            assert got.dim() == 0 and got.dtype == F32
            _close(f"mmd2 {tag}", got, r64, r32)
            _close(f"mmd2 (gamma tensor) {tag}", distribution.mmd2(xd, yd, gammas=_vec(GAMMAS, dev), unbiased=unbiased), r64, r32)
            w = [0.2, 0.5, 0.3]
            _close(f"mmd2 (weights) {tag}", distribution.mmd2(xd, yd, gammas=GAMMAS, weights=w, unbiased=unbiased),
                   ref.mmd2(rx, ry, GAMMAS, w, unbiased), ref.mmd2(rx, ry, GAMMAS, w, unbiased, dtype=F32))
            # gammas=None: 1 / (multiplier x mean cost); the reference takes the f64 closed form, the yardstick the f32 one
            g64, g32 = ref.default_gammas(rx.double(), ry.double()), ref.default_gammas(rx, ry)
            _close(f"mmd2 (default bandwidths) {tag}", distribution.mmd2(xd, yd, unbiased=unbiased),
                   ref.mmd2(rx, ry, g64, None, unbiased), ref.mmd2(rx, ry, g32, None, unbiased, dtype=F32))
        # the V-statistic of a cloud with itself is 0: within the floor, whose magnitude is that of the terms (the mean
        # kernel value of the self block), both for the same tensor and for a copy
        kxx = float(ref.mixture(ref.sq_dists(rx.double(), rx.double()), GAMMAS, [1 / 3] * 3).mean())
        for name, other in (("x, x", xd), ("x, copy of x", xd.clone())):
            v = float(distribution.mmd2(xd, other, gammas=GAMMAS, unbiased=False))
            print(f"biased mmd2({name}) M={M} P={P}: {v:.3e}  floor {64 * U * kxx:.3e}")
            assert abs(v) <= 64 * U * kxx


# ------------------------------------------------------------------------------------------------ 4: gradients
@pytest.mark.parametrize("M,N,P", [(130, 67, 60), (65, 65, 512)])
@pytest.mark.parametrize("unbiased", [True, False])
def test_mmd2_gradients(dev, M, N, P, unbiased):
    x, y = ref.unit_clouds(M, N, P, 3 * M + N + P)

    def ref_grads(dtype):
        a, b = x.clone().to(dtype).requires_grad_(True), y.clone().to(dtype).requires_grad_(True)
        return torch.autograd.grad(ref.mmd2(a, b, GAMMAS, None, unbiased, dtype=dtype), (a, b))

    (gx64, gy64), (gx32, gy32) = ref_grads(F64), ref_grads(F32)
    for need in ("x", "y", "xy"):
        tag = f"M={M} N={N} P={P} unbiased={unbiased} grads of {need}"
        xd = x.clone().to(dev).requires_grad_("x" in need)
        yd = y.clone().to(dev).requires_grad_("y" in need)
        v = distribution.mmd2(xd, yd, gammas=GAMMAS, unbiased=unbiased)
        grads = torch.autograd.grad(v, [t for t in (xd, yd) if t.requires_grad])
        if "x" in need:
            _close(f"d/dx {tag}", grads[0], gx64, gx32)
        if "y" in need:
            _close(f"d/dy {tag}", grads[-1], gy64, gy32)


def test_mmd2_gradient_of_a_cloud_with_its_copy(dev):
    """y = x.clone(), unbiased: every point has a partner at distance 0 in the cross block.  Finite, and the self-block
    factor 2 right: the gradient with respect to x alone matches autograd through the restatement."""
    M, P = 130, 60
    x, _ = ref.unit_clouds(M, 1, P, 41)

    def ref_grad(dtype):
        a = x.clone().to(dtype).requires_grad_(True)
        b = x.clone().to(dtype)
        return torch.autograd.grad(ref.mmd2(a, b, GAMMAS, None, True, dtype=dtype), a)[0]

    xd = x.clone().to(dev).requires_grad_(True)
    yd = x.clone().to(dev).requires_grad_(True)
    gx, gy = torch.autograd.grad(distribution.mmd2(xd, yd, gammas=GAMMAS), (xd, yd))
    assert torch.isfinite(gx).all() and torch.isfinite(gy).all()
    _close("d/dx, y = x.clone()", gx, ref_grad(F64), ref_grad(F32))
    assert torch.equal(gx, gy)                      # the two clouds hold the same numbers: so do their gradients
    # the same tensor on both sides: autograd adds the two arguments' gradients
    xs = x.clone().to(dev).requires_grad_(True)
    gs = torch.autograd.grad(distribution.mmd2(xs, xs, gammas=GAMMAS), xs)[0]
    assert torch.equal(gs, gx + gy)


# ------------------------------------------------------------------------------------------------ 5: graph capture
def test_mmd2_graph_capture(dev):
    M, N, P = 130, 67, 60
    x, y = ref.unit_clouds(M, N, P, 77)
    xd, yd, gd = x.to(dev), y.to(dev), _vec(GAMMAS, dev)
    with torch.no_grad():
        eager = distribution.mmd2(xd, yd, gammas=gd).clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            distribution.mmd2(xd, yd, gammas=gd)
        torch.cuda.current_stream().wait_stream(side)
        graph, keep = torch.cuda.CUDAGraph(), []
        with ops.owned_by_capture(keep), torch.cuda.graph(graph):                   # one stream, no parallel branches
            out = distribution.mmd2(xd, yd, gammas=gd)
        for _ in range(2):
            out.fill_(-1.0)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
    r64, r32 = ref.mmd2(x, y, GAMMAS), ref.mmd2(x, y, GAMMAS, dtype=F32)
    _close("captured mmd2", out, r64, r32)


# ------------------------------------------------------------------------------------------------ 6: the metric separates
def test_metric_separates(dev):
    g = torch.Generator().manual_seed(123)
    a, b = torch.randn(512, 16, generator=g), torch.randn(512, 16, generator=g)
    c = torch.randn(512, 16, generator=g) + 0.5
    ad, bd, cd = a.to(dev), b.to(dev), c.to(dev)
    gam = ref.default_gammas(a.double(), c.double())                  # one set of bandwidths for both pairs
    gam32 = [float(t) for t in _vec([float(t) for t in gam], dev)]   # as the kernel reads them
    vals = {}
    for name, (p, q, pd, qd) in {"matched": (a, b, ad, bd), "shifted": (a, c, ad, cd)}.items():
        with torch.no_grad():
            got = distribution.mmd2(pd, qd, gammas=gam32)
        r64, r32 = ref.mmd2(p, q, gam32), ref.mmd2(p, q, gam32, dtype=F32)
        _close(f"mmd2 {name}", got, r64, r32)
        vals[name] = (float(got), float(r64))
    print(f"matched {vals['matched']}, shifted {vals['shifted']}")
    assert vals["shifted"][1] > vals["matched"][1] and vals["shifted"][0] > vals["matched"][0]
    out = distribution.evaluate_distributions(ad, cd, n_iters=50, tol=None)
    assert list(out) == ["wasserstein", "mmd", "fid"]
    assert all(isinstance(v, float) and v == v and abs(v) != float("inf") for v in out.values()), out
    want = distribution.frechet_distance(a, c)
    assert abs(out["fid"] - want) <= 1e-6 * abs(want), (out["fid"], want)
    assert out["mmd"] == float(distribution.mmd2(ad, cd))
    with pytest.raises(ValueError):
        distribution.evaluate_distributions(ad, cd, metrics=("mmd", "kid"))
