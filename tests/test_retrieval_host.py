"""CPU: host side of the retrieval API (clip_dplm_amd/retrieval.py) - metric reduction, embedding resolution, argument
checks, the C entry points' refusals - and no CPU fallback."""
import ctypes as C

import numpy as np
import pytest
import torch

from clip_dplm_amd import _ffi, ops, retrieval


def test_metrics_from_ranks_hand_made():
    m = retrieval.metrics_from_ranks(torch.tensor([0, 0, 1, 4, 9, 20]), ks=(1, 5, 10))
    assert m["n"] == 6
    assert m["top1"] == pytest.approx(2 / 6) and m["recall@1"] == pytest.approx(2 / 6)
    assert m["recall@5"] == pytest.approx(4 / 6) and m["recall@10"] == pytest.approx(5 / 6)
    assert m["mrr"] == pytest.approx((1 + 1 + 1 / 2 + 1 / 5 + 1 / 10 + 1 / 21) / 6)
    assert m["mean_rank"] == pytest.approx((1 + 1 + 2 + 5 + 10 + 21) / 6)
    assert m["median_rank"] == pytest.approx(3.5)
    assert retrieval.metrics_from_ranks(np.zeros(3, dtype=np.int64), ks=(2,))["recall@2"] == 1.0
    with pytest.raises(ValueError):
        retrieval.metrics_from_ranks(torch.tensor([0, -1]))
    with pytest.raises(ValueError):
        retrieval.metrics_from_ranks(torch.tensor([], dtype=torch.int64))


def test_metrics_reduce_in_f64():
    # 1 / r summed over many ranks: an f32 reduction drifts in the 7th digit, f64 does not
    r = torch.arange(200000, dtype=torch.int64)
    want = float(np.mean(1.0 / (np.arange(200000, dtype=np.float64) + 1)))
    assert retrieval.metrics_from_ranks(r)["mrr"] == want


class _WithEmbed(torch.nn.Module):
    def embed(self, a, b):
        return a + 1, b + 2

    def forward(self, a, b):
        raise AssertionError("forward must not be called when embed exists")


class _TupleOut(torch.nn.Module):          # RNARBPCLIPModel: (a, b, loss)
    def forward(self, a, b):
        return a * 2, b * 3, torch.zeros(())


class _DictOut(torch.nn.Module):           # RNAProteinCLIP wrappers
    def forward(self, a, b):
        return {"logits_per_rna_protein": a @ b.t(), "rna_embeds": a - 1, "protein_embeds": b - 2}


class _TriOut(torch.nn.Module):            # tri-modal ContrastiveModel: three embeddings, no default pairing
    def forward(self, a, b):
        return {"cell_embeds": a, "pert_embeds": b, "protein_embeds": b, "loss": torch.zeros(())}


def test_default_embed_fn_resolves_each_output_format():
    a, b = torch.ones(2, 4), torch.ones(2, 4)
    ea, eb = retrieval.default_embed_fn(_WithEmbed(), (a, b))
    assert torch.equal(ea, a + 1) and torch.equal(eb, b + 2)
    ea, eb = retrieval.default_embed_fn(_TupleOut(), (a, b))
    assert torch.equal(ea, a * 2) and torch.equal(eb, b * 3)
    ea, eb = retrieval.default_embed_fn(_DictOut(), (a, b))
    assert torch.equal(ea, a - 1) and torch.equal(eb, b - 2)
    with pytest.raises(TypeError, match="embed_fn"):
        retrieval.default_embed_fn(_TriOut(), (a, b))


def test_argument_errors_before_any_launch():
    x, y = torch.zeros(3, 8), torch.zeros(100, 8)
    with pytest.raises(ValueError, match="k must be"):
        ops.sim_topk(x, y, 65)
    with pytest.raises(ValueError, match="k must be"):
        ops.sim_topk(x, y, 0)
    with pytest.raises(ValueError, match="exceeds"):
        ops.sim_topk(x, torch.zeros(5, 8), 6)
    with pytest.raises(TypeError):
        ops.sim_topk(x.double(), y, 1)
    with pytest.raises(TypeError):
        retrieval.topk(x.half(), y, 1)
    with pytest.raises(ValueError, match="columns"):
        ops.sim_topk(x, torch.zeros(100, 12), 1)
    with pytest.raises(ValueError, match="P % 4"):
        ops.sim_topk(torch.zeros(3, 6), torch.zeros(100, 6), 1)
    with pytest.raises(ValueError):
        ops.sim_topk(torch.zeros(3, 8, 1), y, 1)
    with pytest.raises(ValueError, match="contiguous"):
        ops.sim_topk(torch.zeros(8, 3).t(), y, 1)
    with pytest.raises(ValueError, match="labels"):
        ops.sim_rank(x, y, labels=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="outside"):
        ops.sim_rank(torch.zeros(200, 8), y)                   # label_offset + i runs past the gallery
    with pytest.raises(ValueError):
        retrieval.retrieval_metrics(torch.zeros(3, 8), torch.zeros(4, 8))
    with pytest.raises(ValueError):
        retrieval.EmbeddingIndex(6, device="cpu")


def test_cpu_tensors_raise_without_fallback():
    x, y = torch.randn(3, 8), torch.randn(100, 8)
    with pytest.raises(_ffi.ClipkError):
        ops.sim_topk(x, y, 5)
    with pytest.raises(_ffi.ClipkError):
        ops.sim_rank(x, y)
    with pytest.raises(_ffi.ClipkError):
        retrieval.topk(x, y, 5)
    with pytest.raises(_ffi.ClipkError):
        retrieval.ranks(x.bfloat16(), y.bfloat16())


def test_c_entry_points_refuse_bad_arguments():
    lib = _ffi.load()
    assert lib.clipk_version() == 7
    # workspace helpers: 0 for shapes the kernels do not take, a size otherwise
    assert lib.clipk_sim_topk_workspace(10, 100, 64, 65) == 0
    assert lib.clipk_sim_topk_workspace(10, 5, 64, 6) == 0
    assert lib.clipk_sim_topk_workspace(0, 100, 64, 1) == 0
    assert lib.clipk_sim_topk_workspace(10, 100, 64, 10) > 0
    assert lib.clipk_sim_rank_workspace(10, 0, 64) == 0
    assert lib.clipk_sim_rank_workspace(10, 100, 64) > 0
    # the entry points validate before touching the device: fake (never dereferenced) pointers
    fake, ws = C.c_void_p(4096), C.c_void_p(8192)
    big = 1 << 30
    BAD, UNSUP = -1, -2
    assert lib.clipk_sim_topk(None, 4, fake, 100, 8, 1.0, 5, fake, fake, ws, big, None) == BAD
    assert lib.clipk_sim_topk(fake, 4, fake, 100, 8, 1.0, 65, fake, fake, ws, big, None) == UNSUP
    assert lib.clipk_sim_topk(fake, 4, fake, 100, 8, 1.0, 101, fake, fake, ws, big, None) == BAD
    assert lib.clipk_sim_topk(fake, 4, fake, 100, 6, 1.0, 5, fake, fake, ws, big, None) == UNSUP
    assert lib.clipk_sim_topk(fake, 0, fake, 100, 8, 1.0, 5, fake, fake, ws, big, None) == BAD
    assert lib.clipk_sim_topk(C.c_void_p(4100), 4, fake, 100, 8, 1.0, 5, fake, fake, ws, big, None) == BAD
    assert lib.clipk_sim_topk(fake, 4, fake, 100, 8, 1.0, 5, fake, fake, ws, 16, None) == BAD
    assert lib.clipk_sim_rank(fake, 4, fake, 100, 8, 1.0, None, 97, fake, fake, ws, big, None) == BAD
    assert lib.clipk_sim_rank(fake, 4, fake, 100, 8, 1.0, None, -1, fake, fake, ws, big, None) == BAD
    assert lib.clipk_sim_rank(fake, 4, fake, 100, 10, 1.0, None, 0, fake, fake, ws, big, None) == UNSUP
    assert lib.clipk_sim_rank(fake, 4, fake, 100, 8, 1.0, None, 0, None, fake, ws, big, None) == BAD


def test_split_option_changes_workspace_not_contract():
    lib = _ffi.load()
    try:
        ops.set_option("retrieval_splits", 1)
        one = lib.clipk_sim_topk_workspace(64, 64 * 100, 64, 10)
        ops.set_option("retrieval_splits", 7)
        seven = lib.clipk_sim_topk_workspace(64, 64 * 100, 64, 10)
        assert seven > one and ops.get_option("retrieval_splits") == 7
    finally:
        ops.reset_options()
    assert ops.get_option("retrieval_splits") == 0
