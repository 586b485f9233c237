"""GPU: the tiled InfoNCE passes on a key list whose two segments meet inside one 64-key tile.

The walk of simce_tiled.hip / simce_hard.hip (cloud_tile.h's KeyWalk<BKT, true>, key_sum_tile.h's key_sum_tile<true>)
takes keys [0, Ny) from the batch and [Ny, Ny + Nc) from the cache.  The other GPU tests of these entries have Ny = 128
with a cache (the boundary lies on a tile edge) or no cache at all; test_gpu_kernels.py::test_simce_tiled_lse_pass has one
straddling tile (1000 + 37 keys), for the plain LSE pass only.  Here, with P = 60 (a ragged last K-step, one 32-row p
tile per wave in the second product) and Mx = 65 (two query blocks, the second with one row):

  * Mx = 65, Ny = 40, Nc = 50: tile 0 holds batch keys 0..39 and cache keys 0..23, tile 1 cache keys 24..49 and the end
    of the list.  Rows 40 - off .. 64 have no diagonal key.  The class-aware and hard-negative entries require a
    diagonal key for every row (label_offset + Mx <= Ny, clipk_simce_lse_cls / clipk_simce_lse_hard return
    CLIPK_ERR_BAD_ARG otherwise), so this shape runs through ops.simce_lse / simce_grad only;
  * Mx = 65, Ny = 104, Nc = 50: the same boundary one tile further on (tile 1 holds batch keys 64..103 and cache keys
    0..23, tile 2 ends the list after 26 keys), through the plain, `_cls` and `_hard` entries.

References are f64 torch on materialised logits; tolerances are those of the same entries in test_gpu_kernels.py
(test_simce_tiled_lse_pass / test_simce_tiled_grad_pass), test_gpu_class_aware_loss.py and
test_gpu_hard_negative_loss.py (test_kernels_match_definition), whose reference functions are used as they are."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_class_aware_loss as CA  # noqa: E402
import test_gpu_hard_negative_loss as HN  # noqa: E402

pytestmark = pytest.mark.gpu

SCALE = CA.SCALE
MX, NC, P = 65, 50, 60


@pytest.mark.parametrize("off", [0, 3])
@pytest.mark.parametrize("Ny", [40, 104])
def test_plain_passes(dev, kopt, Ny, off):
    from clip_dplm_amd import ops
    kopt("simce_kernel", 2)                                  # the tiled kernels at every shape
    x, y, cache = CA._unit((MX, P), dev, 31), CA._unit((Ny, P), dev, 32), CA._unit((NC, P), dev, 33)
    sc = torch.tensor([SCALE], device=dev)
    keys = torch.cat([y, cache]).double()
    S = (x.double() @ keys.t()) * SCALE
    q = torch.arange(MX, device=dev)
    has = q + off < Ny                                       # rows with a diagonal key
    lse, pos = ops.simce_lse(x, y, sc, label_offset=off, cache=cache)
    ref_lse = torch.logsumexp(S, 1)
    assert torch.allclose(lse.double(), ref_lse, rtol=0, atol=2e-5), (lse.double() - ref_lse).abs().max()
    assert torch.allclose(pos.double()[has], S[q[has], q[has] + off], rtol=0, atol=2e-5)
    assert torch.equal(lse, ops.simce_lse(x, y, sc, label_offset=off, cache=cache)[0])
    # gradient pass with consistent LSE vectors: the rows' over all keys, the batch keys' over these queries
    wr, wc, inv_bg = 0.5, 0.5, 1.0 / Ny
    lse_x = ref_lse.float().contiguous()
    lse_y = torch.logsumexp(S[:, :Ny], 0).float().contiguous()
    G = wr * torch.exp(S - lse_x.double()[:, None])
    G[:, :Ny] += wc * torch.exp(S[:, :Ny] - lse_y.double()[None, :])
    G[q[has], q[has] + off] -= (wr + wc)
    G *= inv_bg
    ref_dx = (G @ keys) * SCALE
    ref_dsc = (G * (S / SCALE)).sum(1)
    dx, dsc = ops.simce_grad(x, y, sc, lse_x, lse_y, wr, wc, inv_bg, label_offset=off, cache=cache)
    assert torch.allclose(dx.double(), ref_dx, rtol=1e-4, atol=1e-7), (dx.double() - ref_dx).abs().max()
    assert torch.allclose(dsc.double(), ref_dsc, rtol=1e-4, atol=1e-7)
    assert torch.equal(dx, ops.simce_grad(x, y, sc, lse_x, lse_y, wr, wc, inv_bg, label_offset=off, cache=cache)[0])


def _pair(dev, Ny, off):
    a_g, b_g, cache = CA._unit((Ny, P), dev, 34), CA._unit((Ny, P), dev, 35), CA._unit((NC, P), dev, 36)
    rows = slice(off, off + MX)
    return a_g, b_g, cache, rows, a_g[rows].contiguous(), torch.tensor([SCALE], device=dev)


@pytest.mark.parametrize("off", [0, 3])
@pytest.mark.parametrize("same_class,eps", [("mask", 0.0), ("positive", 0.1)])
def test_class_aware_passes(dev, same_class, eps, off):
    from clip_dplm_amd import ops
    Ny, w_row, w_col = 104, 0.5, 0.5
    a_g, b_g, cache, rows, x, sc = _pair(dev, Ny, off)
    for pattern in ("random", "runs"):
        ids = CA._ids(pattern, Ny, dev)
        cx = ids[rows].contiguous()
        ref = CA._reference(a_g, b_g, cache, ids, same_class, eps, w_row, w_col, rows)
        lse_r, tgt_r, cnt_r = ops.simce_lse_cls(x, b_g, sc, cx, ids, same_class, eps, label_offset=off, cache=cache)
        lse_c, tgt_c, cnt_c = ops.simce_lse_cls(b_g, a_g, sc, ids, ids, same_class, eps)     # every key's own row
        assert torch.allclose(lse_r.double(), ref["lse_r"][rows], rtol=0, atol=2e-5), pattern
        assert torch.allclose(tgt_r.double(), ref["tgt_r"][rows], rtol=0, atol=2e-5), pattern
        assert torch.equal(cnt_r.double(), ref["cnt_r"][rows]), pattern
        dx, dsc = ops.simce_grad_cls(x, b_g, sc, lse_r, lse_c, cnt_r, cnt_c, w_row, w_col, 1.0 / Ny, Ny, cls_x=cx,
                                     cls_y=ids, same_class=same_class, eps=eps, label_offset=off, cache=cache)
        assert torch.allclose(dx.double(), ref["dA"], rtol=1e-4, atol=1e-6), (pattern, (dx.double() - ref["dA"]).abs().max())
        assert abs(dsc.sum().item() - ref["dscale"]) < 1e-5 * max(1.0, abs(ref["dscale"])), pattern


@pytest.mark.parametrize("off", [0, 3])
@pytest.mark.parametrize("beta", [0.5])
def test_hard_negative_passes(dev, beta, off):
    from clip_dplm_amd import ops
    Ny, w_row, w_col = 104, 0.5, 0.5
    a_g, b_g, cache, rows, x, sc = _pair(dev, Ny, off)
    bar = 2e-5 * (1 + 2 * beta)
    for pattern in (None, "random"):
        ids = HN._ids(pattern, Ny, dev)
        cx = None if ids is None else ids[rows].contiguous()
        ref = HN._reference(a_g, b_g, cache, ids, beta, w_row, w_col, rows)
        lse_r, pos_r, coef_r = ops.simce_lse_hard(x, b_g, sc, beta, cx, ids, label_offset=off, cache=cache)
        lse_c, pos_c, coef_c = ops.simce_lse_hard(b_g, a_g, sc, beta, ids, ids)          # every key's own row
        assert (lse_r.double() - ref["lse_r"][rows]).abs().max().item() <= bar, pattern
        assert (pos_r.double() - ref["pos_r"][rows]).abs().max().item() <= bar, pattern
        dx, dsc = ops.simce_grad_hard(x, b_g, sc, beta, coef_r, coef_c, w_row, w_col, 1.0 / Ny, cls_x=cx, cls_y=ids,
                                      label_offset=off, cache=cache)
        assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dsc).all()), pattern
        assert torch.allclose(dx.double(), ref["dA"], rtol=1e-4, atol=1e-6 * (1 + beta)), pattern
        assert abs(dsc.sum().item() - ref["dscale"]) < 1e-5 * max(1.0, abs(ref["dscale"])) * (1 + beta), pattern
