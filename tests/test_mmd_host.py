"""CPU: the host side of clip_dplm_amd.distribution (multi-bandwidth MMD, Frechet distance, evaluate_distributions), the
C ABI of clipk_kernel_sums as far as it goes without a device, and the restatement of tests/mmd_ref.py against literal
loops and textbook formulae."""
import math

import numpy as np
import pytest
import torch

import mmd_ref as ref

F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("diag_offset", [-1, 0, 2, 5])
def test_restated_kernel_sums_against_double_loop(diag_offset):
    g = torch.Generator().manual_seed(11)
    x, y = torch.randn(7, 4, generator=g, dtype=F64), torch.randn(5, 4, generator=g, dtype=F64)
    gammas, weights = [0.3, 1.7], [0.6, -0.25]
    ksum, kbary = torch.zeros(7, dtype=F64), torch.zeros(7, 4, dtype=F64)
    for i in range(7):
        for j in range(5):
            if diag_offset >= 0 and j == i + diag_offset:
                continue
            d2 = sum((float(x[i, p]) - float(y[j, p])) ** 2 for p in range(4))
            k = sum(w * math.exp(-gm * d2) for gm, w in zip(gammas, weights))
            ksum[i] += k
            kbary[i] += k * y[j]
    got = ref.kernel_sums(x, y, gammas, weights, diag_offset)
    assert torch.allclose(got[0], ksum, rtol=0, atol=1e-13) and torch.allclose(got[1], kbary, rtol=0, atol=1e-13)
    # the f32 form (norm expansion) is the same quantity to f32 accuracy
    got32 = ref.kernel_sums(x.float(), y.float(), gammas, weights, diag_offset)
    assert torch.allclose(got32[0].double(), ksum, rtol=0, atol=1e-5) and torch.allclose(got32[1].double(), kbary, rtol=0, atol=1e-5)
    if diag_offset == 5:                            # every skipped key lies beyond N: nothing is skipped
        full = ref.kernel_sums(x, y, gammas, weights, -1)
        assert torch.equal(got[0], full[0]) and torch.equal(got[1], full[1])


@pytest.mark.parametrize("unbiased", [True, False])
def test_restated_mmd2_against_textbook(unbiased):
    g = torch.Generator().manual_seed(5)
    x, y = torch.randn(6, 4, generator=g, dtype=F64), torch.randn(9, 4, generator=g, dtype=F64) + 0.4
    gammas, weights = [0.2, 0.9, 2.0], [0.5, 0.3, 0.2]

    def k(a, b):
        d2 = float(((a - b) ** 2).sum())
        return sum(w * math.exp(-gm * d2) for gm, w in zip(gammas, weights))

    M, N = 6, 9
    if unbiased:
        sxx = sum(k(x[i], x[j]) for i in range(M) for j in range(M) if i != j) / (M * (M - 1))
        syy = sum(k(y[i], y[j]) for i in range(N) for j in range(N) if i != j) / (N * (N - 1))
    else:
        sxx = sum(k(x[i], x[j]) for i in range(M) for j in range(M)) / (M * M)
        syy = sum(k(y[i], y[j]) for i in range(N) for j in range(N)) / (N * N)
    sxy = sum(k(x[i], y[j]) for i in range(M) for j in range(N)) / (M * N)
    want = sxx + syy - 2 * sxy
    assert abs(float(ref.mmd2(x, y, gammas, weights, unbiased)) - want) < 1e-13
    assert abs(float(ref.mmd2(x, y, gammas, weights, unbiased, dtype=F32)) - want) < 1e-5
    if not unbiased:
        assert float(ref.mmd2(x, x, gammas, weights, False)) == 0.0 and want > 0


# ------------------------------------------------------------------------------------------------ Frechet distance
def _frechet_sqrtm(x, y):
    from scipy.linalg import sqrtm
    x, y = x.double().numpy(), y.double().numpy()
    cx, cy = np.cov(x, rowvar=False), np.cov(y, rowvar=False)
    d = x.mean(0) - y.mean(0)
    return float(d @ d + np.trace(cx) + np.trace(cy) - 2.0 * np.trace(sqrtm(cx @ cy)).real), float(np.trace(cx) + np.trace(cy))


@pytest.mark.parametrize("P", [8, 32])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_frechet_against_sqrtm(P, dtype):
    from clip_dplm_amd import distribution
    g = torch.Generator().manual_seed(P)
    mix = torch.randn(P, P, generator=g, dtype=F64) / math.sqrt(P)
    x = (torch.randn(200, P, generator=g, dtype=F64) @ mix).to(dtype)
    y = (torch.randn(200, P, generator=g, dtype=F64) * 1.3 + 0.25).to(dtype)
    want, trace = _frechet_sqrtm(x, y)
    got = distribution.frechet_distance(x, y)
    assert isinstance(got, float) and got > 0
    # both sides work in f64 on the same (dtype-rounded) inputs; sqrtm's Schur form is good to ~1e-12 of the trace here
    assert abs(got - want) <= 1e-9 * trace, (got, want)
    assert abs(got - ref.frechet(x, y)) <= 1e-9 * trace
    # identical clouds: 0 within 1e-9 of the trace
    assert abs(distribution.frechet_distance(x, x.clone())) <= 1e-9 * trace


def test_frechet_rank_deficient():
    """Fewer rows than columns: the covariances have P - n + 1 null eigenvalues, each known to ~u |C| only, so its root
    to sqrt(u |C|) with u = 2^-52: the bound is P sqrt(u) x the trace (~5e-7 of the metric).  sqrtm of a singular product
    is the weaker side; the comparison is with the eigenvalue form in f64 (numpy, on the symmetrised product)."""
    from clip_dplm_amd import distribution
    P = 32
    g = torch.Generator().manual_seed(9)
    x = torch.randn(10, P, generator=g, dtype=F64)
    y = torch.randn(12, P, generator=g, dtype=F64) + 0.5
    xn, yn = x.numpy(), y.numpy()
    cx, cy = np.cov(xn, rowvar=False), np.cov(yn, rowvar=False)
    lam, vec = np.linalg.eigh(cx)
    rx = (vec * np.sqrt(np.maximum(lam, 0))) @ vec.T
    inner = rx @ cy @ rx
    cross = np.sqrt(np.maximum(np.linalg.eigvalsh(0.5 * (inner + inner.T)), 0)).sum()
    d = xn.mean(0) - yn.mean(0)
    trace = float(np.trace(cx) + np.trace(cy))
    want = float(d @ d + trace - 2 * cross)
    got = distribution.frechet_distance(x, y)
    bound = P * math.sqrt(2.0 ** -52) * trace
    assert math.isfinite(got) and abs(got - want) <= bound, (got, want, bound)
    assert abs(got - ref.frechet(x, y)) <= bound
    assert abs(distribution.frechet_distance(x, x)) <= bound


def test_frechet_argument_errors():
    from clip_dplm_amd import distribution
    x = torch.zeros(5, 8)
    with pytest.raises(TypeError):
        distribution.frechet_distance(x.numpy(), x)
    with pytest.raises(TypeError):
        distribution.frechet_distance(x.long(), x)
    with pytest.raises(ValueError):
        distribution.frechet_distance(x, torch.zeros(5, 12))
    with pytest.raises(ValueError):
        distribution.frechet_distance(x[:1], x)                    # n - 1 = 0
    with pytest.raises(ValueError):
        distribution.frechet_distance(x[0], x)


# ------------------------------------------------------------------------------------------------ mmd2 / evaluate arguments
def test_mmd2_argument_errors():
    from clip_dplm_amd import distribution, ops
    mmd2 = distribution.mmd2
    x, y = torch.zeros(6, 8), torch.zeros(5, 8)
    with pytest.raises(TypeError):
        mmd2(x.numpy(), y)
    with pytest.raises(TypeError):
        mmd2(x, [[0.0] * 8] * 5)
    with pytest.raises(TypeError):
        mmd2(x.double(), y)
    with pytest.raises(TypeError):
        mmd2(x, y.bfloat16())
    with pytest.raises(ValueError):
        mmd2(x[0], y)                                               # not 2-D
    with pytest.raises(ValueError):
        mmd2(x[:0], y)                                              # empty
    with pytest.raises(ValueError):
        mmd2(x, torch.zeros(5, 12))                                 # widths differ
    with pytest.raises(ValueError):
        mmd2(torch.zeros(6, 6), torch.zeros(5, 6))                  # not a multiple of 4
    with pytest.raises(ValueError):
        mmd2(torch.zeros(6, 516), torch.zeros(5, 516))              # above 512
    with pytest.raises(ValueError):
        mmd2(x, y, gammas=[])                                       # B = 0
    with pytest.raises(ValueError):
        mmd2(x, y, gammas=[1.0] * 9)                                # B = 9
    with pytest.raises(ValueError):
        mmd2(x, y, gammas=torch.ones(9))
    with pytest.raises(ValueError):
        mmd2(x, y, multipliers=[1.0] * 9)
    with pytest.raises(ValueError):
        mmd2(x, y, gammas=[1.0, 0.0])                               # non-positive bandwidths given as numbers
    with pytest.raises(ValueError):
        mmd2(x, y, gammas=[1.0, -2.0])
    with pytest.raises(ValueError):
        mmd2(x, y, multipliers=[1.0, -1.0])
    with pytest.raises(ValueError):
        mmd2(x, y, gammas=[1.0, 2.0], weights=[1.0])                # one weight per bandwidth
    with pytest.raises(ValueError):
        mmd2(x, y, gammas=torch.ones(2, 2))
    with pytest.raises(TypeError):
        mmd2(x, y, gammas=3)                                        # not a sequence
    with pytest.raises(ValueError):
        mmd2(x[:1], y)                                              # the unbiased estimator needs 2 rows
    with pytest.raises(ValueError):
        mmd2(x, y[:1], unbiased=True)
    with pytest.raises(ValueError, match="device"):
        mmd2(x[:1], y, unbiased=False)                              # allowed as such: what is left is the host tensors
    with pytest.raises(ValueError, match="device"):
        mmd2(x, y)                                                  # host tensors: no CPU fallback
    with pytest.raises(ValueError, match="device"):
        mmd2(x, y, gammas=[0.5, 1.0], weights=[0.5, 0.5], unbiased=False)
    assert ops.KERNEL_SUMS_MAX_P == 512 and ops.KERNEL_SUMS_MAX_B == 8


def test_kernel_sums_wrapper_argument_errors():
    from clip_dplm_amd import ops
    x, y = torch.zeros(6, 8), torch.zeros(5, 8)
    gm, w = torch.ones(2), torch.ones(2)
    with pytest.raises(TypeError):
        ops.kernel_sums(x.double(), y, gm, w)
    with pytest.raises(TypeError):
        ops.kernel_sums(x, y, [1.0, 1.0], w)
    with pytest.raises(TypeError):
        ops.kernel_sums(x, y, gm.double(), w)
    with pytest.raises(ValueError):
        ops.kernel_sums(x, torch.zeros(5, 12), gm, w)
    with pytest.raises(ValueError):
        ops.kernel_sums(torch.zeros(6, 516), torch.zeros(5, 516), gm, w)
    with pytest.raises(ValueError):
        ops.kernel_sums(x, y, torch.ones(9), torch.ones(9))
    with pytest.raises(ValueError):
        ops.kernel_sums(x, y, gm, torch.ones(3))
    with pytest.raises(ValueError):
        ops.kernel_sums(x, y, gm, w, nx=torch.zeros(5))
    with pytest.raises(ValueError):
        ops.kernel_sums(x, y, gm, w, diag_offset=-2)
    with pytest.raises(ValueError):
        ops.kernel_sums(x, y, gm, w, want_sum=False, want_bary=False)
    with pytest.raises(ValueError):
        ops.kernel_sums(x, y, gm, w)                                # host tensors


def test_evaluate_distributions_names():
    from clip_dplm_amd import distribution
    x, y = torch.randn(20, 8), torch.randn(20, 8)
    with pytest.raises(ValueError, match="unknown metric"):
        distribution.evaluate_distributions(x, y, metrics=("fid", "energy"))
    with pytest.raises(TypeError):
        distribution.evaluate_distributions(x, y, metrics=("fid",), bandwidth=1.0)
    out = distribution.evaluate_distributions(x, y, metrics=("fid",))        # the one metric that runs on the host
    assert list(out) == ["fid"] and out["fid"] == distribution.frechet_distance(x, y)
    with pytest.raises(ValueError, match="device"):
        distribution.evaluate_distributions(x, y, metrics=("mmd",))


def test_package_exports():
    import clip_dplm_amd as K
    from clip_dplm_amd import distribution
    assert K.distribution is distribution
    for name in ("mmd2", "frechet_distance", "evaluate_distributions"):
        assert getattr(K, name) is getattr(distribution, name) and name in K.__all__ and name in distribution.__all__
    assert "distribution" in K.__all__


# ------------------------------------------------------------------------------------------------ C ABI without a device
def _call(lib, Mx, Ny, P, B, diag=-1):
    return lib.clipk_kernel_sums(None, Mx, None, Ny, P, None, None, B, None, None, diag, None, None, None, 0, None)


@pytest.mark.parametrize("Mx,Ny,P,B", [(0, 8, 8, 1), (8, 0, 8, 1), (-1, 8, 8, 1), (8, 8, 0, 1), (8, 8, 6, 1), (8, 8, 516, 1),
                                       (8, 8, 8, 0), (8, 8, 8, 9), (8, 8, 8, -1)])
def test_entry_point_refuses(Mx, Ny, P, B):
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    assert lib.clipk_kernel_sums_workspace(Mx, Ny, P, B) == 0
    want = (-2,) if Mx > 0 and Ny > 0 and P > 0 and B > 0 else (-1,)
    assert _call(lib, Mx, Ny, P, B) in want


def test_entry_point_limits_and_null_pointers():
    from clip_dplm_amd import _ffi, ops
    lib = _ffi.load()
    assert lib.clipk_version() == _ffi.ABI_VERSION == 7              # entry points were added, no signature changed
    for n in ("clipk_kernel_sums", "clipk_kernel_sums_workspace"):
        assert n in _ffi.SIGNATURES and hasattr(lib, n)
    assert len(_ffi.SIGNATURES["clipk_kernel_sums"][1]) == 16 and len(_ffi.SIGNATURES["clipk_kernel_sums_workspace"][1]) == 4
    assert lib.clipk_kernel_sums_workspace(1, 1, 4, 1) > 0 and lib.clipk_kernel_sums_workspace(8, 8, 512, 8) > 0
    # a supported shape with null pointers, or a diagonal offset below -1, is a bad argument, not a launch
    assert _call(lib, 8, 8, 64, 5) == -1 and _call(lib, 8, 8, 64, 5, diag=-2) == -1
    # the slabs and the row partials of the split plan: ksplit * Mx * (P + 1) floats
    nqb, ks = ops.kernel_sums_plan(1000, 4097)
    assert (nqb, ks) == ops.sim_lse_bias_plan(1000, 4097) and nqb == 16 and ks > 1
    assert lib.clipk_kernel_sums_workspace(1000, 4097, 128, 5) == ks * 1000 * 129 * 4
