"""Host-side tests of the bf16x3 Sinkhorn (ot.sinkhorn(..., precision="bf16x3"); include/clipk.h: clipk_sim_lse_bias_x3):
argument errors before any launch, the refusals of the three C entry points (they return before any launch, so they run
without a device), the bound on the split products on adversarial data, and - in the f64 restatement of
tests/sinkhorn_x3_ref.py - the three bounds DESIGN.md derives for a converged split solve that ends in one exact iteration
(row-marginal error, value, envelope gradient), which the GPU tests then assert of the kernels."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import sinkhorn_ref as ref
import sinkhorn_x3_ref as x3

F64 = torch.float64
BAD, UNSUP = -1, -2


@pytest.fixture
def no_launch(monkeypatch):
    """Any use of the library after this point is a failure: the argument checks come before every launch."""
    from clip_dplm_amd import ops

    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "_lib", boom)


def test_exports_and_result_fields():
    from clip_dplm_amd import flow, ops, ot
    assert ot.PRECISIONS == ("f32", "bf16x3")
    for n in ("precision", "logit_error_bound"):
        assert n in ot.SinkhornResult.__dataclass_fields__
    assert callable(ops.sim_lse_bias_x3) and callable(ops.sim_lse_bias_x3_plan)
    assert flow.SchrodingerBridgeConditionalFlowMatcher(0.5, precision="bf16x3").precision == "bf16x3"
    assert flow.SchrodingerBridgeConditionalFlowMatcher(0.5).precision == "f32"


def test_precision_argument_errors(no_launch):
    from clip_dplm_amd import flow, ot
    x, y = torch.zeros(6, 8), torch.zeros(5, 8)
    meta = torch.zeros(6, 8, device="meta")
    for bad in ("bf16", "fp32", None, 32):
        for fn in (ot.sinkhorn, ot.sinkhorn_loss, ot.sinkhorn_divergence):
            with pytest.raises(ValueError, match="precision"):
                fn(meta, meta, eps=0.5, precision=bad)          # refused before the device check would refuse the tensors
        with pytest.raises(ValueError, match="precision"):
            flow.SchrodingerBridgeConditionalFlowMatcher(0.5, precision=bad)
        with pytest.raises(ValueError, match="precision"):
            ot.evaluate_transport(lambda s: s, x, x + 1.0, precision=bad)
    for fn in (ot.sinkhorn, ot.sinkhorn_loss, ot.sinkhorn_divergence):
        with pytest.raises(ValueError):
            fn(x, y, eps=0.5, precision="bf16x3")               # host tensors: there is no CPU fallback
        with pytest.raises(TypeError):
            fn(x.double(), y, eps=0.5, precision="bf16x3")
        with pytest.raises(ValueError):
            fn(torch.zeros(6, 772), torch.zeros(5, 772), eps=0.5, precision="bf16x3")
    with pytest.raises(ValueError):
        flow.SchrodingerBridgeConditionalFlowMatcher(0.5, precision="bf16x3").sample_location_and_conditional_flow(x, y)


def test_ops_argument_errors(no_launch):
    from clip_dplm_amd import ops
    bf = torch.bfloat16
    xh, yh, s = torch.zeros(6, 32, dtype=bf), torch.zeros(5, 32, dtype=bf), torch.ones(1)
    u, v = torch.zeros(6), torch.zeros(5)
    call = lambda *a, **kw: ops.sim_lse_bias_x3(*a, **kw)       # noqa: E731
    with pytest.raises(TypeError):
        call(xh.float(), xh, yh, yh, 8, s)                      # planes are 2-byte tensors
    with pytest.raises(TypeError):
        call(xh, xh, yh, yh, 8, 1.0)
    with pytest.raises(TypeError):
        call(xh, xh, yh, yh, 8, s, bias=v.double())
    for P in (6, 0, 772):
        with pytest.raises(ValueError):
            call(xh, xh, yh, yh, P, s)
    with pytest.raises(ValueError):
        call(xh, xh, yh, yh, 60, s)                             # pitch of P = 60 is 64
    with pytest.raises(ValueError):
        call(xh, torch.zeros(5, 32, dtype=bf), yh, yh, 8, s)    # hi and lo of one cloud differ
    with pytest.raises(ValueError):
        call(xh, xh, yh, torch.zeros(32, 5, dtype=bf).t(), 8, s)   # not contiguous
    for kw in (dict(bias=u), dict(logw=v), dict(prev=v), dict(out=v), dict(average=True), dict(err=torch.zeros(1))):
        with pytest.raises(ValueError):
            call(xh, xh, yh, yh, 8, s, **kw)
    with pytest.raises(ValueError):
        call(xh, xh, yh, yh, 8, s)                              # host tensors


# ---- the C entries: every refusal returns before any launch
def _entry(lib, **kw):
    fake = C.c_void_p(4096)
    d = dict(xh=fake, xl=fake, Mx=8, yh=fake, yl=fake, Ny=8, P=64, scale=fake, bias=None, logw=None, prev=None, average=0,
             out=fake, err=None, ws=fake, wsb=1 << 30, st=None)
    d.update(kw)
    return lib.clipk_sim_lse_bias_x3(*[d[k] for k in ("xh", "xl", "Mx", "yh", "yl", "Ny", "P", "scale", "bias", "logw",
                                                    "prev", "average", "out", "err", "ws", "wsb", "st")])


@pytest.mark.parametrize("Mx,Ny,P", [(0, 8, 8), (8, 0, 8), (-1, 8, 8), (8, -3, 8), (8, 8, 0), (8, 8, 6), (8, 8, 772),
                                     (8, 8, 1028)])
def test_entry_points_refuse_shapes(Mx, Ny, P):
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    assert lib.clipk_sim_lse_bias_x3_workspace(Mx, Ny, P) == 0
    want = UNSUP if Mx > 0 and Ny > 0 and P > 0 else BAD
    assert _entry(lib, Mx=Mx, Ny=Ny, P=P) == want
    nqb, ks = C.c_int(0), C.c_int(0)
    rc = lib.clipk_sim_lse_bias_x3_plan(Mx, Ny, C.byref(nqb), C.byref(ks))
    assert rc == (BAD if Mx < 1 or Ny < 1 else 0)


def test_entry_points_refuse_pointers_and_workspace():
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    odd = C.c_void_p(4104)
    for name in ("xh", "xl", "yh", "yl", "scale", "out", "ws"):
        assert _entry(lib, **{name: None}) == BAD, name                # NULL
    for name in ("xh", "xl", "yh", "yl", "ws"):
        assert _entry(lib, **{name: odd}) == BAD, name                 # not 16-byte aligned
    assert _entry(lib, average=1) == BAD                                # averaging without prev
    assert _entry(lib, err=C.c_void_p(4096)) == BAD                     # the error scalar without prev
    need = lib.clipk_sim_lse_bias_x3_workspace(8, 8, 64)
    assert need == (8 * 2 + 8) * 4
    assert _entry(lib, wsb=need - 1) == BAD and _entry(lib, wsb=0) == BAD
    assert lib.clipk_sim_lse_bias_x3_plan(8, 8, None, None) == BAD
    assert lib.clipk_sim_lse_bias_x3_workspace(8, 8, 768) > 0 and lib.clipk_sim_lse_bias_x3_workspace(1, 1, 4) > 0
    assert lib.clipk_version() == _ffi.ABI_VERSION                      # entries only added


def test_plan():
    from clip_dplm_amd import ops
    assert ops.sim_lse_bias_x3_plan(1, 1) == (1, 1)
    assert ops.sim_lse_bias_x3_plan(128, 64) == (1, 1) and ops.sim_lse_bias_x3_plan(129, 65) == (2, 2)
    nqb, ks = ops.sim_lse_bias_x3_plan(1000, 4097)
    assert nqb == 8 and 1 < ks <= 65
    assert ops.sim_lse_bias_x3_plan(65536, 65536) == (512, 1)
    assert ops.sim_lse_bias_x3_plan(8192, 8192) == (64, 8)
    # every split holds at least one tile and the workspace holds every split's partials
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    for Mx, Ny in ((1, 20011), (127, 4097), (1000, 129), (3, 10 ** 7)):
        nqb, ks = ops.sim_lse_bias_x3_plan(Mx, Ny)
        nt = (Ny + 63) // 64
        tps = (nt + ks - 1) // ks
        assert nqb == (Mx + 127) // 128 and 1 <= ks <= 65535 and (ks - 1) * tps < nt <= ks * tps
        assert lib.clipk_sim_lse_bias_x3_workspace(Mx, Ny, 64) == (ks * Mx * 2 + Mx) * 4


# ---- |A - S| <= eps_rel |x| |y| on the adversarial data of the prefilter's host test
def _datasets(P, rng):
    n = 64
    rnd = rng.standard_normal((n, P)).astype(np.float32)
    centres = rng.standard_normal((4, P))
    clustered = (centres[rng.integers(0, 4, n)] + 1e-3 * rng.standard_normal((n, P))).astype(np.float32)
    u = rng.standard_normal((n, P // 2))
    cancel_y = np.concatenate([u, u], 1).astype(np.float32)
    v = rng.standard_normal((n, P // 2))
    cancel_x = np.concatenate([v, -v + 1e-3 * rng.standard_normal((n, P // 2))], 1).astype(np.float32)
    tiny = (rnd * 2.0 ** -120).astype(np.float32)                         # subnormal lo parts
    return [("random", rnd, rnd[::-1].copy()), ("clustered", clustered, clustered[::-1].copy()),
            ("cancellation", cancel_x, cancel_y), ("scaled", rnd * 1e3, tiny[::-1].copy() * 2.0 ** 100)]


@pytest.mark.parametrize("P", [4, 60, 120, 512, 768])
def test_eps_rel_bounds_the_split_products(P):
    from clip_dplm_amd import retrieval
    assert x3.eps_rel(P) == retrieval.prefilter_eps_rel(P, "bf16x3")
    rng = np.random.default_rng(P + 11)
    for name, x, y in _datasets(P, rng):
        xt, yt = torch.from_numpy(x), torch.from_numpy(y)
        A = x3.product(xt, yt)
        S = xt.double() @ yt.double().T
        norms = xt.double().norm(dim=1)[:, None] * yt.double().norm(dim=1)[None, :]
        ratio = float(((A - S).abs() / norms).max())
        print(f"P={P} {name}: max |A - S| / (|x| |y|) = {ratio:.3e}, eps_rel = {x3.eps_rel(P):.3e}")
        assert ((A - S).abs() <= x3.eps_rel(P) * norms).all(), name
        # and eta bounds the scaled logits for any scale
        for scale in (4.0, 40.0):
            assert float((scale * (A - S)).abs().max()) <= x3.logit_error_bound(xt, yt, scale)
    # the split of a value: hi + lo differs from x by at most 2^-16 |x|, hi and lo are bf16 numbers
    xt = torch.from_numpy(_datasets(P, rng)[0][1])
    hi, lo = x3.split(xt)
    assert torch.equal(hi.float().bfloat16().double(), hi) and torch.equal(lo.float().bfloat16().double(), lo)
    assert ((hi + lo - xt.double()).abs() <= 2.0 ** -16 * xt.double().abs()).all()


# ---- the three bounds of a converged split solve that ends in one exact iteration, in f64
def _converged_split(x, y, eps, a, b, symmetric=False):
    """The restatement iterated on A until its marginal error is below 1e-9, then one exact iteration."""
    n = 25
    while True:
        r = x3.solve(x, y, eps, a=a, b=b, n_split=n, n_exact=1, symmetric=symmetric)
        if r.split_error < 1e-9:
            return r, n
        n *= 2
        assert n <= 6400, "the split iteration does not converge"


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("eps", [0.5, 0.05])
@pytest.mark.parametrize("M,N,P", [(96, 160, 64), (40, 30, 512)])
def test_derived_bounds_hold_in_f64(M, N, P, eps, weighted):
    x, y = ref.unit_clouds(M, N, P, M + N + P)
    x, y = 1.7 * x, 0.6 * y                                    # norms away from 1: the bound scales with them
    a, b = (ref.random_weights(M, 1), ref.random_weights(N, 2)) if weighted else (None, None)
    if weighted:                                               # sums of exactly 1 to f64 rounding
        a, b = a.double() / a.double().sum(), b.double() / b.double().sum()
    r, n = _converged_split(x, y, eps, a, b)
    eta = r.eta
    exact = ref.solve(x, y, eps, a=a, b=b, n_iters=4 * n)
    assert float(ref.marginal_error(exact)) < 1e-9
    # 1. rows: L1 error of the returned (exact-kernel) plan; columns exact after the last v update
    p = ref.plan(r)
    row = float((p.sum(1) - r.a).abs().sum())
    assert float((p.sum(0) - r.b).abs().sum()) < 1e-12
    # 2. the value, 3. the envelope gradient of every row
    dv = abs(float(r.value - exact.value))
    gx, _ = ref.envelope_gradients(r)
    ex, _ = ref.envelope_gradients(exact)
    gerr = (gx - ex).norm(dim=1)
    gb = x3.gradient_bound(r)
    print(f"M={M} N={N} P={P} eps={eps} weighted={weighted}: {n} split iterations, eta {eta:.3e}; row error {row:.3e} "
          f"(bound {math.expm1(2 * eta):.3e}); value off {dv:.3e} (bound {4 * eps * eta:.3e}); gradient off / bound "
          f"{float((gerr / gb).max()):.3e}")
    assert 0 < eta < 0.1
    assert row <= math.expm1(2 * eta) + 1e-9
    assert dv <= 4 * eps * eta + 1e-9
    assert (gerr <= gb + 1e-9).all()
    assert float(r.value) <= float(exact.value) + 1e-9        # a dual value with exact columns: a lower bound


def test_derived_bounds_hold_for_the_symmetric_solve():
    x, _ = ref.unit_clouds(96, 1, 64, 5)
    a = ref.random_weights(96, 3).double()
    a = a / a.sum()
    for eps in (0.5, 0.05):
        r, n = _converged_split(x, x, eps, a, a, symmetric=True)
        exact = ref.solve(x, x, eps, a=a, b=a, n_iters=4 * n, symmetric=True)
        row = float((ref.plan(r).sum(1) - r.a).abs().sum())
        dv = abs(float(r.value - exact.value))
        print(f"symmetric eps={eps}: eta {r.eta:.3e}, row error {row:.3e}, value off {dv:.3e}")
        assert row <= math.expm1(2 * r.eta) + 1e-9 and dv <= 4 * eps * r.eta + 1e-9


def test_restatement_with_no_split_iterations_is_the_exact_one():
    x, y = ref.unit_clouds(37, 50, 12, 0)
    r = x3.solve(x, y, 0.5, n_split=0, n_exact=30)
    e = ref.solve(x, y, 0.5, n_iters=30)
    assert torch.equal(r.u, e.u) and torch.equal(r.v, e.v) and torch.equal(r.value, e.value)
    nv = x3.half_iteration(x, y, 4.0, bias=e.v, logw=e.loga)
    assert float((nv - ref.half_iteration(x.double(), y.double(), 4.0, e.v, e.loga)).abs().max()) <= x3.logit_error_bound(x, y, 4.0)
