"""Host-side tests of the classifier probes beyond 64 classes: the refusals of the class-tiled C entry points (they return
before any launch, so they run without a device), the ValueErrors of the binding, which entry points the heads call at 64
and at 65 classes, and the f64 restatement at the reference's 158 classes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import linear_ce_ref as R

REFUSED = [(0, 8, 0, 4), (4, 8, 0, 0), (4, 6, 0, 4), (4, 4096, 4, 4), (4, 0, 0, 4), (-1, 8, 0, 4)]


def _fwd(lib, M, K1, K2, C):
    return lib.clipk_linear_ce_tiled_fwd(None, K1, None, K2, None, None, None, M, C, None, None, None, None, 0, None)


def _bwd(lib, M, K1, K2, C):
    return lib.clipk_linear_ce_tiled_bwd(None, K1, None, K2, None, None, None, M, C, None, None, 0, None, None, None, None, None,
                                         0, None)


@pytest.mark.parametrize("M,K1,K2,C", REFUSED)
def test_tiled_entry_points_refuse(M, K1, K2, C):
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    assert lib.clipk_linear_ce_tiled_workspace(M, K1, K2, C) == 0
    assert _fwd(lib, M, K1, K2, C) in (-1, -2)
    assert _bwd(lib, M, K1, K2, C) in (-1, -2)


def test_tiled_entry_points_accept_and_null_pointers():
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    assert lib.clipk_linear_ce_tiled_workspace(4, 8, 0, 65) > 0
    assert lib.clipk_linear_ce_tiled_workspace(1, 4, 0, 1) > 0
    # a supported shape with null pointers is a bad argument, not a launch
    assert _fwd(lib, 4, 8, 0, 65) == -1
    assert _bwd(lib, 4, 8, 0, 65) == -1
    assert lib.clipk_version() == 7


def test_linear_cross_entropy_tiled_value_errors():
    from clip_dplm_amd import _ffi
    from clip_dplm_amd import functional as KF
    x, w, b = torch.zeros(6, 8), torch.zeros(3, 8), torch.zeros(3)
    lab = torch.zeros(6, dtype=torch.int64)
    bad = [
        dict(x=x.double()), dict(w=w.half()), dict(b=b.double()), dict(x2=torch.zeros(6, 4, dtype=torch.float64), w=torch.zeros(3, 12)),
        dict(lab=lab.float()), dict(lab=lab.bool()), dict(lab=torch.zeros(5, dtype=torch.int64)),
        dict(lab=torch.zeros((6, 1), dtype=torch.int64)), dict(lab=lab.to("meta")),
        dict(x=torch.zeros(6, 6), w=torch.zeros(3, 6)),
        dict(x2=torch.zeros(6, 2), w=torch.zeros(3, 10)),
    ]
    for kw in bad:
        a = dict(x=x, w=w, b=b, lab=lab, x2=None)
        a.update(kw)
        with pytest.raises(ValueError):
            KF.linear_cross_entropy_tiled(a["x"], a["w"], a["b"], a["lab"], x2=a["x2"])
    # 65 classes pass the argument checks; host tensors then fail as every ops.* call does
    with pytest.raises(_ffi.ClipkError):
        KF.linear_cross_entropy_tiled(x, torch.zeros(65, 8), torch.zeros(65), lab)
    with pytest.raises(ValueError):
        KF.linear_cross_entropy(x, torch.zeros(65, 8), torch.zeros(65), lab)          # the 64-class entry still refuses


def _heads(K, C):
    return [K.MLPClassifier(16, [8], C), K.TransformerClassifier(16, 8, C, num_layers=1, num_heads=2), K.LinearClassifier(16, C),
            K.SimpleNonLinearClassifier(16, 8, C)]


@pytest.mark.parametrize("C,tiled", [(64, False), (65, True)])
def test_heads_choose_the_entry_point_by_width(monkeypatch, C, tiled):
    """loss() goes through functional.linear_cross_entropy / _tiled, predict() through ops.linear_ce_fwd / _tiled_fwd: 64
    classes call the entries the heads called before, 65 the class-tiled ones.  The recorders stand in for the kernels, and
    features() is cut short, so nothing needs a device."""
    import clip_dplm_amd as K
    from clip_dplm_amd import functional as KF
    from clip_dplm_amd import ops
    calls = []

    def recorder(name, ret):
        def f(x, weight, *a, **kw):
            calls.append((name, weight.shape[0]))
            return ret
        return f

    monkeypatch.setattr(KF, "linear_cross_entropy", recorder("loss", "L"))
    monkeypatch.setattr(KF, "linear_cross_entropy_tiled", recorder("loss_tiled", "L"))
    monkeypatch.setattr(ops, "linear_ce_fwd", recorder("pred", (None, None, "P", None)))
    monkeypatch.setattr(ops, "linear_ce_tiled_fwd", recorder("pred_tiled", (None, None, "P")))
    x, lab = torch.zeros(3, 16), torch.zeros(3, dtype=torch.int64)
    for m in _heads(K, C):
        monkeypatch.setattr(m, "features", lambda t: t)
        calls.clear()
        assert m.loss(x, lab) == "L" and m.predict(x) == "P"
        assert m.loss(x[:, :8], lab, x2=x[:, 8:]) == "L" and m.predict(x[:, :8], x2=x[:, 8:]) == "P"
        want = [("loss_tiled" if tiled else "loss", C), ("pred_tiled" if tiled else "pred", C)] * 2
        assert calls == want, (type(m).__name__, calls)


@pytest.mark.parametrize("K2", [0, 8])
def test_restatement_matches_torch_f64_at_158_classes(K2):
    rng = np.random.default_rng(5)
    M, K1, C = 21, 12, 158
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
