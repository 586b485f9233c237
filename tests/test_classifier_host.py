"""Host-side tests of the classifier probes: the f64 restatement of the fused Linear + cross-entropy entries against
torch, the CPU restatement of the four heads against the reference fixture, the ValueErrors of the binding and the
refusals of the C entry points (which return before any launch, so they run without a device)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import classifier_ref
import linear_ce_ref as R

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CTOR = {"mlp": ("MLPClassifier", (256, [64, 32], 7), {}),
        "transformer": ("TransformerClassifier", (256, 32, 7), {"num_layers": 1, "num_heads": 4}),
        "linear": ("LinearClassifier", (256, 7), {}),
        "simple": ("SimpleNonLinearClassifier", (256, 64, 7), {})}


@pytest.fixture(scope="module")
def fixture():
    return classifier_ref.load_fixture(G)


@pytest.mark.parametrize("K2", [0, 8])
def test_restatement_matches_torch_f64(K2):
    rng = np.random.default_rng(3)
    M, K1, C = 13, 12, 5
    x1, x2 = rng.standard_normal((M, K1)), (rng.standard_normal((M, K2)) if K2 else None)
    w, b = rng.standard_normal((C, K1 + K2)), rng.standard_normal(C)
    labels = rng.integers(0, C, M)
    lse, tgt, pred, z = R.fwd(x1, w, b, labels, x2)
    tx1 = torch.tensor(x1, requires_grad=True)
    tx2 = torch.tensor(x2, requires_grad=True) if K2 else None
    tw, tb = torch.tensor(w, requires_grad=True), torch.tensor(b, requires_grad=True)
    tz = F.linear(tx1 if tx2 is None else torch.cat([tx1, tx2], 1), tw, tb)
    loss = F.cross_entropy(tz, torch.tensor(labels))
    (3.0 * loss).backward()
    assert np.allclose(z, tz.detach().numpy(), rtol=0, atol=1e-13)
    assert abs(R.mean_loss(lse, tgt) - loss.item()) < 1e-13
    assert np.array_equal(pred, torch.max(tz, 1)[1].numpy())
    dW, db, dx1, dx2, _ = R.bwd(x1, w, b, labels, g=3.0, x2=x2)
    assert np.allclose(dW, tw.grad.numpy(), rtol=0, atol=1e-13) and np.allclose(db, tb.grad.numpy(), rtol=0, atol=1e-13)
    assert np.allclose(dx1, tx1.grad.numpy(), rtol=0, atol=1e-13)
    if K2:
        assert np.allclose(dx2, tx2.grad.numpy(), rtol=0, atol=1e-13)


def test_restatement_label_and_tie_rules():
    rng = np.random.default_rng(4)
    M, K, C = 9, 8, 4
    x, w, b = rng.standard_normal((M, K)), rng.standard_normal((C, K)), rng.standard_normal(C)
    w[2], b[2] = w[1], b[1]                                 # classes 1 and 2 tie on every row
    labels = rng.integers(0, C, M)
    labels[3], labels[6] = C, -1
    lse, tgt, pred, z = R.fwd(x, w, b, labels)
    assert np.isnan(tgt[[3, 6]]).all() and np.isfinite(np.delete(tgt, [3, 6])).all()
    assert np.isnan(R.mean_loss(lse, tgt))
    assert (pred != 2).all() and np.array_equal(pred, torch.max(torch.tensor(z), 1)[1].numpy())
    # the gradients are those of the batch without the two rows, at the full batch's 1 / M
    keep = np.delete(np.arange(M), [3, 6])
    dW, db, dx, _, G_ = R.bwd(x, w, b, labels)
    dWk, dbk, dxk, _, _ = R.bwd(x[keep], w, b, labels[keep], g=len(keep) / M)
    assert np.allclose(dW, dWk, atol=1e-15) and np.allclose(db, dbk, atol=1e-15)
    assert np.allclose(dx[keep], dxk, atol=1e-15) and not dx[[3, 6]].any() and not G_[[3, 6]].any()


@pytest.mark.parametrize("tag", list(classifier_ref.HEADS))
def test_head_restatement_matches_reference_fixture(fixture, tag):
    import clip_dplm_amd as K
    heads, x, labels = fixture
    f = heads[tag]
    cls, a, kw = CTOR[tag]
    m = getattr(K, cls)(*a, **kw)
    assert list(m.state_dict().keys()) == f["keys"]          # a reference checkpoint loads
    m.load_state_dict(f["sd"])
    sd = {k: v.clone().requires_grad_(True) for k, v in f["sd"].items()}
    logits = classifier_ref.HEADS[tag](sd, x)
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    # f32 rounding: the two sides are the same f32 operations up to the order of sums inside the matrix products
    assert (logits - f["logits"]).abs().max().item() < 2e-5 * max(1.0, f["logits"].abs().max().item())
    assert abs(loss.item() - f["loss"]) < 1e-5
    gmax = max(g.abs().max().item() for g in f["grads"].values())
    for k in f["keys"]:
        assert sd[k].grad is not None, k
        assert (sd[k].grad - f["grads"][k]).abs().max().item() <= 2e-5 * max(f["grads"][k].abs().max().item(), 1e-3 * gmax), k
    if tag == "transformer":
        E = 32
        for k in ("transformer_encoder.layers.0.self_attn.in_proj_weight", "transformer_encoder.layers.0.self_attn.in_proj_bias"):
            assert not sd[k].grad[:2 * E].any()              # q and k: exact zeros, not None
            # torch's own softmax backward over the single key, p (g - sum(p g)) with p = 1, leaves the residue of one f32
            # rounding instead of an exact zero: the reference's recorded q / k gradients are bounded by u = 2^-24 times
            # the size of the v gradients they sit beside (recorded: 4.7e-10 and 5.8e-10 against 4.4e-2 and 3.0e-2)
            vmax = f["grads"][k][2 * E:].abs().max().item()
            assert vmax > 0 and f["grads"][k][:2 * E].abs().max().item() <= 2.0 ** -24 * vmax


def test_linear_cross_entropy_value_errors():
    from clip_dplm_amd import functional as KF
    x, w, b = torch.zeros(6, 8), torch.zeros(3, 8), torch.zeros(3)
    lab = torch.zeros(6, dtype=torch.int64)
    bad = [
        dict(x=x.double()), dict(w=w.half()), dict(b=b.double()), dict(x2=torch.zeros(6, 4, dtype=torch.float64), w=torch.zeros(3, 12)),
        dict(lab=lab.float()), dict(lab=lab.bool()), dict(lab=torch.zeros(5, dtype=torch.int64)),
        dict(lab=torch.zeros((6, 1), dtype=torch.int64)), dict(lab=lab.to("meta")),
        dict(w=torch.zeros(65, 8), b=torch.zeros(65)), dict(x=torch.zeros(6, 6), w=torch.zeros(3, 6)),
        dict(x2=torch.zeros(6, 2), w=torch.zeros(3, 10)),
    ]
    for kw in bad:
        a = dict(x=x, w=w, b=b, lab=lab, x2=None)
        a.update(kw)
        with pytest.raises(ValueError):
            KF.linear_cross_entropy(a["x"], a["w"], a["b"], a["lab"], x2=a["x2"])


REFUSED = [(0, 8, 0, 4), (4, 8, 0, 0), (4, 8, 0, 65), (4, 6, 0, 4), (4, 8, 6, 4), (4, 4096, 4, 4), (4, 0, 0, 4), (-1, 8, 0, 4)]


@pytest.mark.parametrize("M,K1,K2,C", REFUSED)
def test_c_entry_points_refuse(M, K1, K2, C):
    """Refused shapes with null device pointers: the entries return an error before any launch, the helper returns 0."""
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    assert lib.clipk_linear_ce_workspace(M, K1, K2, C) == 0
    assert lib.clipk_linear_ce_fwd(None, K1, None, K2, None, None, None, M, C, None, None, None, None, 0, None) in (-1, -2)
    assert lib.clipk_linear_ce_bwd(None, K1, None, K2, None, None, None, M, C, None, None, 0, None, None, None, None, None, 0,
                                   None) in (-1, -2)


def test_c_entry_points_accept_and_null_pointers():
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    assert lib.clipk_linear_ce_workspace(37, 128, 128, 7) > 0
    assert lib.clipk_linear_ce_workspace(1, 4, 0, 1) > 0
    # a supported shape with null pointers is a bad argument, not a launch
    assert lib.clipk_linear_ce_fwd(None, 8, None, 0, None, None, None, 4, 4, None, None, None, None, 0, None) == -1
    assert lib.clipk_linear_ce_bwd(None, 8, None, 0, None, None, None, 4, 4, None, None, 0, None, None, None, None, None, 0,
                                   None) == -1
    assert lib.clipk_version() == 7
