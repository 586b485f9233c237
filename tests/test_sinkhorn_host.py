"""Host-side tests of the Sinkhorn optimal transport (clip_dplm_amd.ot): exports, every argument error before any launch,
the closed-form mean cost, the refusals of the C entry points (they return before any launch, so they run without a
device), compute_transport_error on a stub map, and the properties of the restatement tests/sinkhorn_ref.py in f64 that
the GPU tests rely on."""
import pytest
import torch

import sinkhorn_ref as ref

F64 = torch.float64


def test_exports():
    import clip_dplm_amd as K
    from clip_dplm_amd import icnn, ops, ot
    assert K.ot is ot and K.sinkhorn is ot.sinkhorn and K.sinkhorn_divergence is ot.sinkhorn_divergence
    assert K.SinkhornResult is ot.SinkhornResult
    for n in ("ot", "sinkhorn", "sinkhorn_divergence", "SinkhornResult"):
        assert n in K.__all__
    for n in ("sinkhorn", "sinkhorn_loss", "sinkhorn_divergence", "SinkhornResult", "evaluate_transport", "mean_cost"):
        assert hasattr(ot, n)
    for n in ("f", "g", "u", "v", "eps", "value", "n_iters", "marginal_error"):
        assert n in ot.SinkhornResult.__dataclass_fields__
    for n in ("marginals", "cost", "barycentric_map"):
        assert callable(getattr(ot.SinkhornResult, n))
    assert callable(ops.sim_lse_bias) and callable(ops.sinkhorn_apply) and callable(icnn.compute_transport_error)


@pytest.fixture
def no_launch(monkeypatch):
    """Any use of the library after this point is a failure: the argument checks come before every launch."""
    from clip_dplm_amd import ops

    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "_lib", boom)


def test_sinkhorn_argument_errors(no_launch):
    from clip_dplm_amd import ot
    x, y = torch.zeros(6, 8), torch.zeros(5, 8)
    a, b = torch.full((6,), 1 / 6), torch.full((5,), 0.2)
    meta = torch.zeros(6, 8, device="meta")
    cases = [
        (TypeError, dict(x=x.double())), (TypeError, dict(y=y.half())), (TypeError, dict(x=[[0.0] * 8])),
        (ValueError, dict(y=torch.zeros(5, 12))),                                      # width mismatch
        (ValueError, dict(x=torch.zeros(6, 6), y=torch.zeros(5, 6))),                   # P % 4
        (ValueError, dict(x=torch.zeros(6, 772), y=torch.zeros(5, 772))),               # P > 768
        (ValueError, dict(x=torch.zeros(8))), (ValueError, dict(x=torch.zeros(0, 8))),
        (ValueError, dict(a=torch.full((5,), 0.2))), (ValueError, dict(b=torch.full((6,), 1 / 6))),     # wrong length
        (ValueError, dict(a=torch.tensor([0.5, 0.5, 0.0, 0.0, 0.0, 0.0]))),             # not positive
        (ValueError, dict(b=torch.tensor([1.5, -0.5, 0.0, 0.0, 0.0]))),
        (TypeError, dict(a=a.double())),
        (ValueError, dict(eps=0.0)), (ValueError, dict(eps=-1.0)), (ValueError, dict(eps=float("nan"))),
        (ValueError, dict(eps_rel=0.0)), (ValueError, dict(n_iters=0)), (ValueError, dict(tol=0.0)),
        (ValueError, dict(symmetric=True)),                                             # y is not x
        (ValueError, dict(y=x.clone(), symmetric=True)),                                # an equal tensor is not x either
        (ValueError, dict(y=x, b=torch.full((6,), 1 / 6), symmetric=True)),             # b is not a
        (ValueError, dict()),                                                           # host tensors: not on the device
        (ValueError, dict(y=meta)),
    ]
    for exc, kw in cases:
        args = dict(x=x, y=y, a=a, b=b, eps=0.5)
        args.update(kw)
        xx, yy = args.pop("x"), args.pop("y")
        with pytest.raises(exc):
            ot.sinkhorn(xx, yy, **args)
    for fn in (ot.sinkhorn_loss, ot.sinkhorn_divergence):
        for exc, kw in ((TypeError, dict(x=x.double())), (ValueError, dict(eps=0.0)), (ValueError, dict())):
            args = dict(x=x, y=y, eps=0.5)
            args.update(kw)
            xx, yy = args.pop("x"), args.pop("y")
            with pytest.raises(exc):
                fn(xx, yy, **args)
    # gradients need the apply kernel's width
    wide = torch.zeros(4, 768, requires_grad=True)
    with pytest.raises(ValueError):
        ot.sinkhorn_divergence(wide, torch.zeros(4, 768), eps=0.5)


def test_ops_argument_errors(no_launch):
    from clip_dplm_amd import ops
    x, y, s = torch.zeros(6, 8), torch.zeros(5, 8), torch.ones(1)
    u, v = torch.zeros(6), torch.zeros(5)
    with pytest.raises(TypeError):
        ops.sim_lse_bias(x.double(), y, s)
    with pytest.raises(TypeError):
        ops.sim_lse_bias(x, y, 1.0)
    with pytest.raises(TypeError):
        ops.sim_lse_bias(x, y, s, bias=v.double())
    for kw in (dict(bias=u), dict(logw=v), dict(prev=v), dict(out=v), dict(average=True), dict(err=torch.zeros(1))):
        with pytest.raises(ValueError):
            ops.sim_lse_bias(x, y, s, **kw)
    with pytest.raises(ValueError):
        ops.sim_lse_bias(x, torch.zeros(5, 12), s)
    with pytest.raises(ValueError):
        ops.sim_lse_bias(torch.zeros(6, 772), torch.zeros(5, 772), s)
    with pytest.raises(ValueError):
        ops.sim_lse_bias(x, y, s)                                   # host tensors
    with pytest.raises(ValueError):
        ops.sinkhorn_apply(torch.zeros(6, 516), torch.zeros(5, 516), s, u, v, want_cost=False)      # P > 512
    with pytest.raises(ValueError):
        ops.sinkhorn_apply(x, y, s, v, u, want_cost=False)          # potentials of the wrong lengths
    with pytest.raises(ValueError):
        ops.sinkhorn_apply(x, y, s, u, v)                           # cost without the squared norms
    with pytest.raises(ValueError):
        ops.sinkhorn_apply(x, y, s, u, v, want_mass=False, want_bary=False, want_cost=False)
    with pytest.raises(TypeError):
        ops.sinkhorn_apply(x, y, s, u.double(), v, want_cost=False)
    with pytest.raises(ValueError):
        ops.sinkhorn_apply(x, y, s, u, v, want_cost=False)          # host tensors


def _lse(lib, Mx, Ny, P):
    return lib.clipk_sim_lse_bias(None, Mx, None, Ny, P, None, None, None, None, 0, None, None, None, 0, None)


def _apply(lib, Mx, Ny, P):
    return lib.clipk_sinkhorn_apply(None, Mx, None, Ny, P, None, None, None, None, None, None, None, None, None, 0, None)


@pytest.mark.parametrize("Mx,Ny,P", [(0, 8, 8), (8, 0, 8), (-1, 8, 8), (8, 8, 0), (8, 8, 6), (8, 8, 772), (8, 8, 1028)])
def test_entry_points_refuse(Mx, Ny, P):
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    assert lib.clipk_sim_lse_bias_workspace(Mx, Ny, P) == 0
    assert lib.clipk_sinkhorn_apply_workspace(Mx, Ny, P) == 0
    want = (-2,) if Mx > 0 and Ny > 0 and P > 0 else (-1,)
    assert _lse(lib, Mx, Ny, P) in want
    assert _apply(lib, Mx, Ny, P) in want


def test_entry_points_limits_and_null_pointers():
    from clip_dplm_amd import _ffi, ops
    lib = _ffi.load()
    assert lib.clipk_sim_lse_bias_workspace(8, 8, 768) > 0 and lib.clipk_sim_lse_bias_workspace(1, 1, 4) > 0
    assert lib.clipk_sinkhorn_apply_workspace(8, 8, 512) > 0
    assert lib.clipk_sinkhorn_apply_workspace(8, 8, 516) == 0 and _apply(lib, 8, 8, 516) == -2      # the LSE pass goes on to 768
    assert lib.clipk_sim_lse_bias_workspace(8, 8, 516) > 0
    # a supported shape with null pointers is a bad argument, not a launch
    assert _lse(lib, 8, 8, 64) == -1 and _apply(lib, 8, 8, 64) == -1
    assert ops.SIM_LSE_BIAS_MAX_P == 768 and ops.SINKHORN_APPLY_MAX_P == 512
    assert ops.sim_lse_bias_plan(1, 1) == (1, 1)
    nqb, ks = ops.sim_lse_bias_plan(1000, 4097)
    assert nqb == 16 and 1 < ks <= 65
    assert ops.sim_lse_bias_plan(65536, 65536) == (1024, 1)
    assert lib.clipk_version() == _ffi.ABI_VERSION


@pytest.mark.parametrize("weighted", [False, True])
def test_mean_cost_closed_form(weighted):
    from clip_dplm_amd import ot
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(37, 12, generator=g, dtype=F64), torch.randn(50, 12, generator=g, dtype=F64) + 0.5
    a = ref.random_weights(37, 1).double() if weighted else None
    b = ref.random_weights(50, 2).double() if weighted else None
    if weighted:                                    # the closed form is that of weights that sum to 1: exactly, here
        a, b = a / a.sum(), b / b.sum()
    want = ref.mean_cost_explicit(x, y, a, b)
    if not weighted:
        assert abs(float(want) - float(ref.cost_matrix(x, y).mean())) < 1e-12
    assert abs(float(ot.mean_cost(x, y, a, b)) - float(want)) < 1e-12 * float(want)


def test_compute_transport_error_on_a_stub_map():
    from clip_dplm_amd import icnn
    g = torch.Generator().manual_seed(4)
    src, tgt = torch.randn(300, 8, generator=g), torch.randn(300, 8, generator=g)
    stub = lambda s: 2.0 * s + 1.0
    per_batch = [torch.nn.functional.mse_loss(stub(src[i:i + 128]), tgt[i:i + 128]).item() for i in range(0, 300, 128)]
    assert len(per_batch) == 3
    want = sum(per_batch) / 3                       # the reference's mean of batch means: the short last batch counts in full
    assert icnn.compute_transport_error(stub, src, tgt, batch_size=128) == want
    assert icnn.compute_transport_error(stub, src, tgt) == want
    assert abs(want - float(((stub(src) - tgt) ** 2).mean())) > 1e-6


# ---- the restatement's own properties in f64 (M = 37, N = 50, P = 12, non-uniform weights)
def _problem():
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(37, 12, generator=g, dtype=F64) * 0.3, torch.randn(50, 12, generator=g, dtype=F64) * 0.3 + 0.1
    a, b = ref.random_weights(37, 1).double(), ref.random_weights(50, 2).double()
    return x, y, a / a.sum(), b / b.sum()              # sums of exactly 1, to f64 rounding


def test_restatement_marginals_and_primal_equals_dual():
    x, y, a, b = _problem()
    r = ref.solve(x, y, 0.5, a=a, b=b, n_iters=300)
    p = ref.plan(r)
    assert float((p.sum(1) - a).abs().sum()) < 1e-13 and float((p.sum(0) - b).abs().sum()) < 1e-13
    assert float(ref.marginal_error(r)) < 1e-13
    kl = (p * (p / (a[:, None] * b[None, :])).log()).sum()
    primal = (p * ref.cost_matrix(x, y)).sum() + r.eps * kl
    assert abs(float(primal - r.value)) < 1e-13
    assert abs(float(ref.transport_cost(r) - (p * ref.cost_matrix(x, y)).sum())) < 1e-15
    # one more u update measures the same marginal error as the plan itself
    nv = ref.half_iteration(x, y, 2.0 / r.eps, r.v, r.loga)
    r5 = ref.solve(x, y, 0.5, a=a, b=b, n_iters=5)
    nv5 = ref.half_iteration(x, y, 2.0 / r5.eps, r5.v, r5.loga)
    assert abs(float(ref.marginal_error_term(r5.loga, r5.u, nv5) - ref.marginal_error(r5))) < 1e-14
    assert float((nv - r.u).abs().max()) < 1e-12


def test_restatement_envelope_gradient_equals_autograd():
    x, y, a, b = _problem()
    x1, y1 = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    d = ref.divergence(x1, y1, 0.5, a=a, b=b, n_iters=300)
    d.backward()
    _, gx, gy, _ = ref.divergence_envelope_gradients(x, y, 0.5, a=a, b=b, n_iters=300)
    assert float((gx - x1.grad).abs().max()) < 1e-14 and float((gy - y1.grad).abs().max()) < 1e-14
    assert float(d.detach()) > 0
    x2, y2 = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    r = ref.solve(x2, y2, 0.5, a=a, b=b, n_iters=300)
    r.value.backward()
    ex, ey = ref.envelope_gradients(ref.solve(x, y, 0.5, a=a, b=b, n_iters=300))
    assert float((ex - x2.grad).abs().max()) < 1e-14 and float((ey - y2.grad).abs().max()) < 1e-14


def test_restatement_symmetric_update():
    x, _, a, _ = _problem()
    r = ref.solve(x, x, 0.1, a=a, b=a, n_iters=10, symmetric=True)
    p = ref.plan(r)
    assert r.v is r.u
    assert float((p - p.T).abs().max()) < 1e-15
    assert float(ref.marginal_error(r)) < 1e-13              # ten averaged iterations
    # the alternating update on the same problem is what the averaged one replaces: still far away after 300 iterations
    alt = ref.solve(x, x, 0.1, a=a, b=a, n_iters=300)
    print(f"alternating update after 300 iterations: marginal error {float(ref.marginal_error(alt)):.2e}, value "
          f"{float(alt.value):.9f} against {float(r.value):.9f}")
    assert float(ref.marginal_error(alt)) > 1e-6
    # a fixed point of the alternating update too
    nv = ref.half_iteration(x, x, 2.0 / r.eps, r.u, r.loga)
    assert float((nv - r.u).abs().max()) < 1e-13


def test_restatement_divergence_of_a_cloud_with_itself_is_zero():
    x, _, a, _ = _problem()
    x1 = x.clone().requires_grad_(True)
    d = ref.divergence(x1, x1, 0.1, a=a, b=a, n_iters=30)
    d.backward()
    assert abs(float(d.detach())) < 1e-13 and float(x1.grad.abs().max()) < 1e-13
