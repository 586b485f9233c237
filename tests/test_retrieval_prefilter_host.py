"""CPU: host side of the prefiltered exact top-k (clip_dplm_amd/retrieval.py prefilter=, include/clipk.h
clipk_split_bf16 / clipk_sim_topk_cand / clipk_sim_rerank): argument checks before any device work, the C entry points'
refusals, and the certificate's eps_rel against a numpy emulation of the bf16 / bf16x3 products."""
import ctypes as C

import numpy as np
import pytest
import torch

from clip_dplm_amd import _ffi, ops, retrieval


def test_prefilter_arguments_raise_before_device_work():
    x, y = torch.zeros(3, 8), torch.zeros(100, 8)            # CPU tensors: any device work would raise ClipkError
    with pytest.raises(ValueError, match="prefilter"):
        retrieval.topk(x, y, 5, prefilter="fp8")
    with pytest.raises(ValueError, match="candidates"):
        retrieval.topk(x, y, 5, prefilter="bf16", candidates=5)
    with pytest.raises(ValueError, match="candidates"):
        retrieval.topk(x, y, 5, prefilter="bf16x3", candidates=3)
    with pytest.raises(ValueError, match="candidates"):
        retrieval.topk(x, y, 5, prefilter="bf16", candidates=65)
    with pytest.raises(ValueError, match="63"):
        retrieval.topk(x, y, 64, prefilter="bf16")
    with pytest.raises(ValueError, match="63"):
        retrieval.topk(x, y, 0, prefilter="bf16x3")
    with pytest.raises(ValueError, match="needs a prefilter"):
        retrieval.topk(x, y, 5, candidates=20)
    with pytest.raises(TypeError):
        retrieval.topk(x.double(), y, 5, prefilter="bf16")
    with pytest.raises(TypeError):
        retrieval.topk(x, y.half(), 5, prefilter="bf16x3")
    with pytest.raises(ValueError, match="P % 4"):
        retrieval.topk(torch.zeros(3, 6), torch.zeros(100, 6), 5, prefilter="bf16")
    with pytest.raises(ValueError, match="exceeds"):
        retrieval.topk(x, torch.zeros(4, 8), 5, prefilter="bf16")
    with pytest.raises(ValueError, match="prefilter"):
        retrieval.EmbeddingIndex(8, device="cpu", prefilter="bf8")
    # ops level: dtype, layout and alignment of the candidate pass's operands
    hi = torch.zeros(100, 32, dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        ops.sim_topk_cand(x.double(), hi, None, 100, 8, 16)
    with pytest.raises(ValueError, match="aligned"):
        ops.sim_topk_cand(torch.zeros(3 * 8 + 1)[1:].view(3, 8), hi, None, 100, 8, 16)
    with pytest.raises(ValueError, match="planes"):
        ops.sim_topk_cand(x, torch.zeros(100, 8, dtype=torch.bfloat16), None, 100, 8, 16)
    with pytest.raises(ValueError, match="candidates"):
        ops.sim_topk_cand(x, hi, None, 100, 8, 65)
    with pytest.raises(TypeError):
        ops.split_bf16(y.double(), hi)
    with pytest.raises(ValueError, match="planes"):
        ops.split_bf16(y, torch.zeros(100, 8, dtype=torch.bfloat16))
    cs, ci = torch.zeros(3, 16), torch.zeros(3, 16, dtype=torch.int64)
    with pytest.raises(ValueError, match="candidates"):
        ops.sim_rerank(x, y, cs, ci.int(), 5, 0.01, torch.ones(1))
    with pytest.raises(ValueError, match="k <= candidates"):
        ops.sim_rerank(x, y, cs, ci, 17, 0.01, torch.ones(1))


def test_cpu_tensors_raise_without_fallback():
    x, y = torch.randn(3, 8), torch.randn(100, 8)
    for mode in ("bf16", "bf16x3"):
        with pytest.raises(_ffi.ClipkError):
            retrieval.topk(x, y, 5, prefilter=mode)
    with pytest.raises(_ffi.ClipkError):
        ops.split_bf16(y, torch.zeros(100, 32, dtype=torch.bfloat16))


def test_default_candidates():
    assert retrieval._prefilter_args(1, "bf16x3", None) == (1, 16)
    assert retrieval._prefilter_args(10, "bf16x3", None) == (10, 20)
    assert retrieval._prefilter_args(1, "bf16", None) == (1, 64)
    assert retrieval._prefilter_args(10, "bf16", None) == (10, 64)
    assert retrieval._prefilter_args(32, "bf16x3", None) == (32, 64)
    assert retrieval._prefilter_args(63, "bf16x3", None) == (63, 64)
    assert retrieval._prefilter_args(63, "bf16", 64) == (63, 64)
    assert retrieval._prefilter_args(64, None, None) == (64, None)


def test_new_c_entry_points_refuse_bad_arguments():
    lib = _ffi.load()
    assert lib.clipk_version() == 7
    assert lib.clipk_sim_topk_cand_workspace(10, 100, 64, 65, 1) == 0
    assert lib.clipk_sim_topk_cand_workspace(10, 100, 64, 0, 1) == 0
    assert lib.clipk_sim_topk_cand_workspace(10, 100, 64, 16, 3) == 0
    assert lib.clipk_sim_topk_cand_workspace(10, 100, 6, 16, 1) == 0
    assert lib.clipk_sim_topk_cand_workspace(0, 100, 64, 16, 1) == 0
    one = lib.clipk_sim_topk_cand_workspace(10, 100, 64, 16, 1)
    assert 0 < one < lib.clipk_sim_topk_cand_workspace(10, 100, 64, 16, 2)
    fake, ws, big = C.c_void_p(4096), C.c_void_p(8192), 1 << 30
    BAD, UNSUP = -1, -2
    # clipk_split_bf16(X, n_rows, P, hi, lo, norm_max, stream)
    assert lib.clipk_split_bf16(None, 4, 8, fake, None, None, None) == BAD
    assert lib.clipk_split_bf16(fake, 0, 8, fake, None, None, None) == BAD
    assert lib.clipk_split_bf16(fake, 4, 6, fake, None, None, None) == UNSUP
    assert lib.clipk_split_bf16(fake, 4, 65540, fake, None, None, None) == UNSUP
    assert lib.clipk_split_bf16(C.c_void_p(4100), 4, 8, fake, None, None, None) == BAD
    assert lib.clipk_split_bf16(fake, 4, 8, fake, C.c_void_p(4104), None, None) == BAD
    # clipk_sim_topk_cand(X, Mx, Yhi, Ylo, Ny, P, scale, kc, cand_scores, cand_idx, ws, ws_bytes, stream)
    assert lib.clipk_sim_topk_cand(None, 4, fake, None, 100, 8, 1.0, 16, fake, fake, ws, big, None) == BAD
    assert lib.clipk_sim_topk_cand(fake, 4, None, None, 100, 8, 1.0, 16, fake, fake, ws, big, None) == BAD
    assert lib.clipk_sim_topk_cand(fake, 4, fake, None, 100, 8, 1.0, 65, fake, fake, ws, big, None) == BAD
    assert lib.clipk_sim_topk_cand(fake, 4, fake, None, 100, 8, 1.0, 0, fake, fake, ws, big, None) == BAD
    assert lib.clipk_sim_topk_cand(fake, 0, fake, None, 100, 8, 1.0, 16, fake, fake, ws, big, None) == BAD
    assert lib.clipk_sim_topk_cand(fake, 4, fake, None, 100, 6, 1.0, 16, fake, fake, ws, big, None) == UNSUP
    assert lib.clipk_sim_topk_cand(fake, 4, C.c_void_p(4104), None, 100, 8, 1.0, 16, fake, fake, ws, big, None) == BAD
    assert lib.clipk_sim_topk_cand(fake, 4, fake, C.c_void_p(4104), 100, 8, 1.0, 16, fake, fake, ws, big, None) == BAD
    assert lib.clipk_sim_topk_cand(fake, 4, fake, None, 100, 8, 1.0, 16, fake, fake, ws, 16, None) == BAD
    # clipk_sim_rerank(X, Mx, Y, Ny, P, scale, cand_idx, cand_scores, kc, k, eps_rel, y_norm_max, scores, idx, cert, st)
    args = lambda **kw: [kw.get(n, d) for n, d in (  # noqa: E731
        ("X", fake), ("Mx", 4), ("Y", fake), ("Ny", 100), ("P", 8), ("scale", 1.0), ("ci", fake), ("cs", fake),
        ("kc", 16), ("k", 5), ("eps", 0.01), ("yn", fake), ("s", fake), ("i", fake), ("c", fake), ("st", None))]
    assert lib.clipk_sim_rerank(*args(X=None)) == BAD
    assert lib.clipk_sim_rerank(*args(yn=None)) == BAD
    assert lib.clipk_sim_rerank(*args(c=None)) == BAD
    assert lib.clipk_sim_rerank(*args(k=17)) == BAD
    assert lib.clipk_sim_rerank(*args(k=0)) == BAD
    assert lib.clipk_sim_rerank(*args(kc=65, k=5)) == BAD
    assert lib.clipk_sim_rerank(*args(Ny=4)) == BAD
    assert lib.clipk_sim_rerank(*args(eps=-1.0)) == BAD
    assert lib.clipk_sim_rerank(*args(eps=float("nan"))) == BAD
    assert lib.clipk_sim_rerank(*args(P=6)) == UNSUP
    assert lib.clipk_sim_rerank(*args(Y=C.c_void_p(4100))) == BAD


# ---- the bound: numpy emulation of the operands the MFMA sees
def _bf16(a):
    """Round f32 to bf16 (nearest even), returned as f32."""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32)


def _split(x, mode):
    hi = _bf16(x)
    lo = _bf16(x - hi) if mode == "bf16x3" else np.zeros_like(hi)      # x - hi is exact in f32
    return hi.astype(np.float64), lo.astype(np.float64)


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


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("P", [4, 60, 120, 512, 1028, 1280])
def test_eps_rel_bounds_the_split_products(mode, P):
    rng = np.random.default_rng(P + (7 if mode == "bf16x3" else 0))
    v = 2.0 ** -8
    operand_term = 2 * v + v * v if mode == "bf16" else 3 * v * v + 7 * v ** 3
    eps = retrieval.prefilter_eps_rel(P, mode)
    for name, x, y in _datasets(P, rng):
        xh, xl = _split(x, mode)
        yh, yl = _split(y, mode)
        exact = x.astype(np.float64) @ y.astype(np.float64).T
        approx = xh @ yh.T + (xh @ yl.T + xl @ yh.T if mode == "bf16x3" else 0.0)
        mag = np.abs(x.astype(np.float64)) @ np.abs(y.astype(np.float64)).T       # sum |x_p y_p|
        err = np.abs(approx - exact)
        assert (err <= operand_term * mag * (1 + 1e-9) + 1e-300).all(), (name, float((err / mag).max()))
        norms = np.linalg.norm(x.astype(np.float64), axis=1)[:, None] * np.linalg.norm(y.astype(np.float64), axis=1)
        assert (err <= eps * norms).all(), name
        # the products summed in f32 in index order (one admissible MFMA order) stay inside the accumulation term
        prods = (xh[:, None, :] * yh[None, :, :]).astype(np.float32)
        if mode == "bf16x3":
            prods = np.concatenate([prods, (xh[:, None, :] * yl[None, :, :]).astype(np.float32),
                                    (xl[:, None, :] * yh[None, :, :]).astype(np.float32)], 2)
        s32 = np.zeros(prods.shape[:2], dtype=np.float32)
        for p in range(prods.shape[2]):
            s32 = (s32 + prods[:, :, p]).astype(np.float32)
        n = prods.shape[2]
        assert (np.abs(s32 - approx) <= n * 2.0 ** -22 * np.abs(prods.astype(np.float64)).sum(2) + 1e-300).all()


def test_eps_rel_orders():
    for P in (4, 120, 512, 1028):
        b, b3 = retrieval.prefilter_eps_rel(P, "bf16"), retrieval.prefilter_eps_rel(P, "bf16x3")
        assert 2 * 2.0 ** -8 < b < 2.0 ** -6
        assert b3 < b / 4
    with pytest.raises(ValueError):
        retrieval.prefilter_eps_rel(64, "fp8")
