"""Host-side tests of the plan sampler (clipk_sim_sample, ops.sim_sample, SinkhornResult.sample_targets / sample_pairs,
clip_dplm_amd.flow): the noise contract restated in tests/sinkhorn_sample_ref.py (Philox known answer, the construction
is a correct sampler), the exports and signatures, the refusals of the C entry (it returns before any launch, so it runs
without a device), every argument error before any launch, and flow.conditional_flow against its formulae in f64."""
import math

import numpy as np
import pytest
import torch

import sinkhorn_sample_ref as sref

ref = sref.ref
F64 = torch.float64


# ------------------------------------------------------------------------------------------------ the noise contract
def test_philox_known_answer():
    want = (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert tuple(int(v) for v in sref.philox4x32_10(0, 0, 0, 0, 0, 0)) == want
    z = torch.zeros(1, dtype=torch.int64)
    assert tuple(int(v) for v in sref.philox4x32_10_torch(z, z, z, z, 0, 0)) == want


def test_philox_torch_restatement_equals_numpy():
    rng = np.random.default_rng(0)
    c = [rng.integers(0, 1 << 32, 4096, dtype=np.uint64) for _ in range(4)]
    c[0][:4] = (0, 0xFFFFFFFF, 0xFFFF, 0x10000)                          # the halves of the split product at their ends
    c[2][:4] = (0xFFFFFFFF, 0, 0x10000, 0xFFFF)
    for seed in (0, 777, -1, (1 << 63) + 12345):
        k0, k1 = sref._split64(seed)
        a = sref.philox4x32_10(*c, k0, k1)
        b = sref.philox4x32_10_torch(*(torch.from_numpy(v.astype(np.int64)) for v in c), k0, k1)
        for x, y in zip(a, b):
            assert np.array_equal(x.astype(np.int64), y.numpy())


def test_counter_layout_and_uniforms():
    """Key j reads word j & 3 of the counter (j >> 2, stream lo, stream hi, 0); U is exact in f32 and inside (0, 1)."""
    seed, stream = (5 << 32) + 9, (3 << 32) + 7
    w = sref.words(seed, [stream], 11)[0]
    for j in range(11):
        assert int(w[j]) == int(sref.philox4x32_10(j >> 2, 7, 3, 0, 9, 5)[j & 3])
    u = sref.uniforms(np.array([0, 0x1FF, 0x200, 0xFFFFFFFF], dtype=np.uint64))
    assert u[0] == u[1] == 2.0 ** -24 and u[2] == 3 * 2.0 ** -24 and u[3] == 1 - 2.0 ** -24
    many = sref.uniforms(sref.words(1, [0, 1], 4096))
    assert np.array_equal(many.astype(np.float32).astype(np.float64), many)
    # the torch path gives the numpy path's noise, for streams on both sides of 2^32 and a negative (wrapped) seed
    for s0 in (0, (1 << 32) - 2, (1 << 40) + 3):
        g_np = sref.gumbel_numpy(-3, [s0 + k for k in range(4)], 63)
        assert np.array_equal(g_np, sref.gumbel(-3, s0, 4, 63, F64).numpy())


def test_gumbel_argmax_is_a_correct_sampler():
    """4 unit rows, 63 keys, P = 4, scale 3, 20000 draws per row (streams 4 k + row), seed 777: the counts against the
    softmax by Pearson's chi-square at 62 degrees of freedom (mean 62, sd sqrt(124) = 11.1); threshold mean + 5 sd."""
    x, y = ref.unit_clouds(4, 63, 4, 1)
    lg = 3.0 * (x.double() @ y.double().T).numpy()
    for row in range(4):
        g = sref.gumbel_numpy(777, [4 * k + row for k in range(20000)], 63)
        counts = np.bincount((lg[row][None, :] + g).argmax(1), minlength=63)
        p = np.exp(lg[row] - lg[row].max())
        p /= p.sum()
        chi = sref.chi_square(counts, p)
        print(f"row {row}: chi-square {chi:.1f}, smallest expected count {20000 * p.min():.1f}")
        assert 20000 * p.min() > 5 and chi < 118


def test_restatement_draw_agrees_with_direct_argmax():
    x, y = ref.unit_clouds(9, 65, 8, 2)
    bias = torch.linspace(-2, 2, 65)
    d = sref.draw(x, y, 4.0, bias, seed=11, stream0=100, rows=4)
    g = sref.gumbel_numpy(11, [100 + k for k in range(9)], 65)
    z = (4.0 * (x.double() @ y.double().T) + bias.double()[None, :]).numpy() + g
    assert np.array_equal(d.idx.numpy(), z.argmax(1)) and np.allclose(d.score.numpy(), z.max(1), rtol=0, atol=1e-13)
    srt = np.sort(z, axis=1)
    assert np.allclose(d.gap.numpy(), srt[:, -1] - srt[:, -2], rtol=0, atol=1e-13)
    got, best = sref.values_at(x[2:4], y, 4.0, bias, 11, [102, 103], [5, int(d.idx[3])])
    assert abs(float(got[0]) - z[2, 5]) < 1e-13 and float(got[1]) == float(best[1]) == float(d.score[3])
    # equal maxima go to the lower key
    one = sref.draw(torch.zeros(1, 4), torch.zeros(1, 4), 1.0)
    assert int(one.idx[0]) == 0 and math.isinf(float(one.gap[0]))


def test_restatement_passes_the_statistical_checks():
    """What tests/test_gpu_sinkhorn_sample.py asks of the kernel's draws (column counts by chi-square, per-row means
    against the barycentric map), asked of the f64 restatement alone with the same seed."""
    x, y, eps, rows, seed = sref.statistics_problem()
    r64 = ref.solve(x, y, eps, n_iters=100)
    assert float(ref.marginal_error(r64)) < 1e-12
    d = sref.draw(x[rows], y, float(2.0 / r64.eps), r64.v, seed, 0, F64, rows=8192)
    sref.check_statistics(d.idx, rows, y, r64)


# ------------------------------------------------------------------------------------------------ exports, C entry
def test_exports_and_signatures():
    import clip_dplm_amd as K
    from clip_dplm_amd import _ffi, flow, ops, ot
    lib = _ffi.load()
    assert lib.clipk_version() == _ffi.ABI_VERSION == 7
    for n in ("clipk_sim_sample_workspace", "clipk_sim_sample"):
        assert n in _ffi.SIGNATURES and hasattr(lib, n)
    assert len(_ffi.SIGNATURES["clipk_sim_sample"][1]) == 13 and len(_ffi.SIGNATURES["clipk_sim_sample_workspace"][1]) == 3
    assert callable(ops.sim_sample)
    assert callable(ot.SinkhornResult.sample_targets) and callable(ot.SinkhornResult.sample_pairs)
    assert K.flow is flow and K.conditional_flow is flow.conditional_flow and K.flow_matching_loss is flow.flow_matching_loss
    assert K.SchrodingerBridgeConditionalFlowMatcher is flow.SchrodingerBridgeConditionalFlowMatcher
    for n in ("flow", "SchrodingerBridgeConditionalFlowMatcher", "conditional_flow", "flow_matching_loss"):
        assert n in K.__all__


def _sample(lib, Mx, Ny, P):
    return lib.clipk_sim_sample(None, Mx, None, Ny, P, None, None, None, None, None, None, 0, None)


@pytest.mark.parametrize("Mx,Ny,P", [(0, 8, 8), (8, 0, 8), (-1, 8, 8), (8, 8, 0), (8, 8, 6), (8, 8, 772), (8, 8, 1028)])
def test_entry_point_refuses(Mx, Ny, P):
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    assert lib.clipk_sim_sample_workspace(Mx, Ny, P) == 0
    assert _sample(lib, Mx, Ny, P) == (-2 if Mx > 0 and Ny > 0 and P > 0 else -1)


def test_entry_point_limits_and_null_pointers():
    from clip_dplm_amd import _ffi, ops
    lib = _ffi.load()
    assert lib.clipk_sim_sample_workspace(8, 8, 768) > 0 and lib.clipk_sim_sample_workspace(1, 1, 4) > 0
    assert _sample(lib, 8, 8, 64) == -1                            # a supported shape with null pointers: no launch
    # one (value, key) pair per row and key split of the LSE pass's plan
    for Mx, Ny in ((1, 1), (1000, 4097), (65, 100003)):
        _, ks = ops.sim_lse_bias_plan(Mx, Ny)
        assert lib.clipk_sim_sample_workspace(Mx, Ny, 64) == ks * Mx * 8


# ------------------------------------------------------------------------------------------------ argument errors
@pytest.fixture
def no_launch(monkeypatch):
    """Any use of the library after this point is a failure: the argument checks come before every launch."""
    from clip_dplm_amd import ops

    def boom():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "_lib", boom)


def test_ops_argument_errors(no_launch):
    from clip_dplm_amd import ops
    x, y, s = torch.zeros(6, 8), torch.zeros(5, 8), torch.ones(1)
    with pytest.raises(TypeError):
        ops.sim_sample(x.double(), y, s)
    with pytest.raises(TypeError):
        ops.sim_sample(x, y, 1.0)
    with pytest.raises(TypeError):
        ops.sim_sample(x, y, s, bias=torch.zeros(5, dtype=F64))
    with pytest.raises(ValueError):
        ops.sim_sample(x, y, s, bias=torch.zeros(6))
    with pytest.raises(ValueError):
        ops.sim_sample(x, torch.zeros(5, 12), s)
    with pytest.raises(ValueError):
        ops.sim_sample(torch.zeros(6, 772), torch.zeros(5, 772), s)
    with pytest.raises(ValueError):
        ops.sim_sample(torch.zeros(6, 6), torch.zeros(5, 6), s)
    with pytest.raises(ValueError):
        ops.sim_sample(x, y, s)                                     # host tensors
    for bad in (1.5, "7", None, True, torch.zeros(2, dtype=torch.int32), torch.zeros(3, dtype=torch.int64),
                torch.zeros(1, 2, dtype=torch.int64)):
        with pytest.raises(TypeError):
            ops.sim_sample(x, y, s, seed=bad)
    with pytest.raises(TypeError):
        ops.sim_sample(x, y, s, stream_offset=0.5)
    with pytest.raises(ValueError):
        ops.sim_sample(x, y, s, seed=torch.zeros(2, dtype=torch.int64), stream_offset=3)
    with pytest.raises(ValueError):
        ops.sim_sample(x, y, s, seed=torch.zeros(2, dtype=torch.int64))         # the seed tensor on the host
    # Python ints of any size are taken modulo 2^64
    assert ops._seed_offset(-1, 1 << 64) is None and ops._seed_offset((1 << 63) + 5, 7) is None


def _host_result(M=6, N=5, P=8, a=None):
    from clip_dplm_amd import ot
    z = torch.zeros
    return ot.SinkhornResult(f=z(M), g=z(N), u=z(M), v=z(N), eps=torch.tensor(0.5), value=z(()), n_iters=1,
                             marginal_error=z(()), _x=z(M, P), _y=z(N, P), _scale=torch.ones(1), _nx=z(M), _ny=z(N), _a=a)


def test_ot_argument_errors(no_launch):
    r = _host_result()
    with pytest.raises(TypeError):
        r.sample_targets(rows=[0, 1])
    with pytest.raises(TypeError):
        r.sample_targets(rows=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(TypeError):
        r.sample_targets(rows=torch.zeros(2, 2, dtype=torch.int64))
    with pytest.raises(TypeError):
        r.sample_targets(rows=torch.zeros(0, dtype=torch.int64))
    with pytest.raises(ValueError):
        r.sample_targets(rows=torch.zeros(3, dtype=torch.int64, device="meta"))
    for bad in (torch.tensor([0, 6]), torch.tensor([-1, 2])):
        with pytest.raises(IndexError):
            r.sample_targets(rows=bad)
    with pytest.raises(TypeError):
        r.sample_targets(seed=0.5)
    with pytest.raises(ValueError):
        r.sample_targets()                                          # host clouds: refused by the op, before the library
    with pytest.raises(ValueError):
        r.sample_targets(rows=torch.tensor([0, 0, 5]))
    with pytest.raises(ValueError):
        r.sample_pairs(n=0)
    with pytest.raises(TypeError):
        r.sample_pairs(seed="3")
    with pytest.raises(ValueError):
        r.sample_pairs()
    with pytest.raises(ValueError):
        _host_result(a=torch.full((6,), 1 / 6)).sample_pairs(n=4)


def test_flow_argument_errors(no_launch):
    from clip_dplm_amd import flow
    M = flow.SchrodingerBridgeConditionalFlowMatcher
    for kw in (dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=0.5, reg=0.0),
               dict(sigma=0.5, n_iters=0), dict(sigma=0.5, tol=0.0)):
        with pytest.raises(ValueError):
            M(**kw)
    m = M(0.5)
    assert m.reg == 0.5 and m.n_iters == 50 and m.tol is None and M(0.1, reg=3.0).reg == 3.0
    x0, x1 = torch.zeros(6, 8), torch.zeros(5, 8)
    with pytest.raises(ValueError):
        m.sample_location_and_conditional_flow(x0, x1)              # host tensors
    with pytest.raises(TypeError):
        m.sample_location_and_conditional_flow(x0.double(), x1)
    with pytest.raises(ValueError):
        m.sample_location_and_conditional_flow(x0, x1, t=torch.zeros(5))
    with pytest.raises(TypeError):
        m.sample_location_and_conditional_flow(x0, x1, seed=1.5)
    z = torch.zeros(4, 3)
    with pytest.raises(ValueError):
        flow.conditional_flow(z, torch.zeros(4, 2), 0.5, z, 1.0)
    with pytest.raises(ValueError):
        flow.conditional_flow(z, z, torch.zeros(3), z, 1.0)
    with pytest.raises(TypeError):
        flow.conditional_flow(z, z, 0.5, None, 1.0)


# ------------------------------------------------------------------------------------------------ the flow arithmetic
def test_conditional_flow_formulae():
    from clip_dplm_amd import flow
    g = torch.Generator().manual_seed(0)
    n, P, sigma = 33, 12, 0.7
    x0, x1, noise = (torch.randn(n, P, generator=g, dtype=F64) for _ in range(3))
    t = torch.rand(n, generator=g, dtype=F64)
    t[0], t[1] = 0.0, 0.5
    xt, ut = flow.conditional_flow(x0, x1, t, noise, sigma)
    assert xt.dtype == F64 and xt.shape == ut.shape == (n, P)
    for k in range(n):
        tk = float(t[k])
        mu = tk * x1[k] + (1 - tk) * x0[k]
        want_x = mu + sigma * math.sqrt(tk * (1 - tk)) * noise[k]
        want_u = (1 - 2 * tk) / (2 * tk * (1 - tk) + 1e-8) * (want_x - mu) + x1[k] - x0[k]
        assert float((xt[k] - want_x).abs().max()) < 1e-14 and float((ut[k] - want_u).abs().max()) < 1e-12
    assert torch.equal(xt[0], x0[0]) and torch.equal(ut[0], x1[0] - x0[0])       # t = 0: the source point, the chord
    assert torch.equal(ut[1], x1[1] - x0[1])                                      # t = 1/2: the bridge term vanishes
    xs, us = flow.conditional_flow(x0, x1, 0.25, noise, sigma)                    # one time for every row
    xr, ur = flow.conditional_flow(x0, x1, torch.full((n,), 0.25, dtype=F64), noise, sigma)
    assert torch.equal(xs, xr) and torch.equal(us, ur)
    v = torch.randn(n, P, generator=g, dtype=F64)
    assert abs(float(flow.flow_matching_loss(v, ut)) - float(((v - ut) ** 2).mean())) < 1e-12 * float((ut ** 2).mean())
