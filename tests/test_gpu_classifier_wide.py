"""GPU tests of the classifier probes beyond 64 classes: the class-tiled Linear + cross-entropy kernels
(clipk_linear_ce_tiled_*) against the f64 restatement (tests/linear_ce_ref.py) within the bounds of
tests/test_gpu_classifier.py (derived from u = 2^-24; they hold for any contraction order), ties, out-of-range labels,
determinism, agreement with the 64-class kernels, the heads at 158 classes, training against f64 Adam, a captured
loss + backward, and the probe loop."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import linear_ce_ref as R
from test_gpu_classifier import _f64_adam_losses, bounds, make, n64, raw_bwd, raw_fwd

pytestmark = pytest.mark.gpu
U = 2.0 ** -24

# one row / one class / one more than a tile in rows and in classes / ragged K / the second source 4 columns wide / class
# splits (few rows, many classes) / the reference's 158 markers and 2,547 cell types
SHAPES = [(1, 4, 0, 65), (63, 36, 0, 64), (64, 32, 0, 1), (65, 132, 124, 127), (64, 256, 0, 128), (129, 64, 64, 129),
          (257, 512, 512, 158), (33, 4092, 4, 70), (32, 1024, 0, 2547), (300, 128, 128, 2547)]


def run_tiled(dev, M, K1, K2, C, g=1.0, labels=None, seed=0):
    x1, x2, w, b, lab = make(M, K1, K2, C, seed)
    lab = lab if labels is None else labels
    d = [None if t is None else t.to(dev) for t in (x1, x2, w, b, lab)]
    gd = torch.tensor([g], dtype=torch.float32, device=dev)
    fw = raw_fwd(dev, *d, tiled=True)
    bw = raw_bwd(dev, *d, fw[0], gd, tiled=True)
    return (x1, x2, w, b, lab), d, gd, fw, bw


def sure_rows(z, ez):
    """Rows whose f64 top-two gap exceeds twice the row's logit bound: every valid f32 evaluation has the f64 argmax."""
    if z.shape[1] == 1:
        return np.ones(z.shape[0], bool)
    top = np.sort(z, axis=1)[:, -2:]
    return (top[:, 1] - top[:, 0]) > 2.0 * ez.max(axis=1)


@pytest.mark.parametrize("M,K1,K2,C", SHAPES)
def test_tiled_kernels_against_f64_restatement(dev, M, K1, K2, C):
    g = 0.75
    (x1, x2, w, b, lab), d, gd, (lse, tgt, pred), (dW, db, dx1, dx2) = run_tiled(dev, M, K1, K2, C, g)
    a = [n64(t) for t in (x1, x2, w, b)]
    r_lse, r_tgt, r_pred, r_z = R.fwd(a[0], a[2], a[3], lab.numpy(), a[1])
    r_dW, r_db, r_dx1, r_dx2, _ = R.bwd(a[0], a[2], a[3], lab.numpy(), g, a[1])
    e = bounds(a[0], a[1], a[2], a[3], lab.numpy(), g)
    worst = {}

    def close(name, got, ref, bound):
        err = np.abs(n64(got) - ref)
        worst[name] = float((err / np.maximum(bound, 1e-300)).max())
        assert (err <= bound).all(), (name, float(err.max()), worst[name])

    close("lse", lse, r_lse, e["lse"])
    close("tgt", tgt, r_tgt, e["tgt"])
    close("dW", dW, r_dW, e["dW"])
    close("dbias", db, r_db, e["db"])
    close("dx1", dx1, r_dx1, e["dx"][:, :K1])
    if K2:
        close("dx2", dx2, r_dx2, e["dx"][:, K1:])
    sure = sure_rows(r_z, e["z"])
    print(f"linear_ce_tiled {(M, K1, K2, C)}: worst error / bound {worst}; pred compared on {int(sure.sum())} of {M} rows")
    assert (~sure).sum() <= 0.10 * M
    p = pred.cpu().numpy()
    assert ((p >= 0) & (p < C)).all() and np.array_equal(p[sure], r_pred[sure])


def test_ties_resolve_to_the_lower_class_across_tiles_and_splits(dev):
    """Entries k / 4: every product and every partial sum is exact in f32, so equal logits are equal bits.  Classes 3, 67
    and 130 sit in three class tiles, and at 70 rows each tile is a class split of its own."""
    M, K, C = 70, 24, 131
    g = torch.Generator().manual_seed(7)
    x = torch.randint(-4, 5, (M, K), generator=g).float() / 4
    w = torch.randint(-4, 5, (C, K), generator=g).float() / 4
    b = torch.randint(-4, 5, (C,), generator=g).float() / 4
    w[3] = torch.randint(-4, 5, (K,), generator=g).float()     # four times the others' scale: the maximum of many rows
    w[67], b[67] = w[3], b[3]
    w[130], b[130] = w[3], b[3]
    lab = torch.randint(0, C, (M,), generator=g)
    z = R.logits(x.numpy(), w.numpy(), b.numpy())
    assert np.array_equal(z, z.astype(np.float32)) and np.array_equal(z[:, 3], z[:, 67]) and np.array_equal(z[:, 3], z[:, 130])
    lse, tgt, pred = raw_fwd(dev, x.to(dev), None, w.to(dev), b.to(dev), lab.to(dev), tiled=True)
    p = pred.cpu().numpy()
    assert np.array_equal(p, R.first_argmax(z))
    assert (p == 3).sum() > 5 and not ((p == 67) | (p == 130)).any()
    assert np.array_equal(tgt.cpu().numpy().astype(np.float64), z[np.arange(M), lab.numpy()])     # exact logits


def test_out_of_range_labels(dev):
    M, K1, K2, C = 150, 64, 36, 70
    x1, x2, w, b, lab = make(M, K1, K2, C, seed=3)
    out = [17, 101, 149]
    lab[17], lab[101], lab[149] = C, -1, 2 ** 40
    _, d, gd, (lse, tgt, pred), (dW, db, dx1, dx2) = run_tiled(dev, M, K1, K2, C, 1.0, labels=lab, seed=3)   # (canaries inside)
    assert torch.isnan(tgt[out]).all() and torch.isfinite(tgt).sum().item() == M - 3
    assert not dx1[out].any() and not dx2[out].any()
    keep = [i for i in range(M) if i not in out]
    a = [n64(t) for t in (x1, x2, w, b)]
    r_lse, _, r_pred, r_z = R.fwd(a[0], a[2], a[3], lab.numpy(), a[1])
    # the gradients of the batch without the three rows, at the full batch's 1 / M
    r_dW, r_db, r_dx1, r_dx2, _ = R.bwd(a[0][keep], a[2], a[3], lab.numpy()[keep], len(keep) / M, a[1][keep])
    e = bounds(a[0], a[1], a[2], a[3], lab.numpy(), 1.0)
    assert (np.abs(n64(lse) - r_lse) <= e["lse"]).all()
    sure = sure_rows(r_z, e["z"])
    assert np.array_equal(pred.cpu().numpy()[sure], r_pred[sure])
    assert (np.abs(n64(dW) - r_dW) <= e["dW"]).all() and (np.abs(n64(db) - r_db) <= e["db"]).all()
    assert (np.abs(n64(dx1)[keep] - r_dx1) <= e["dx"][keep][:, :K1]).all()
    assert (np.abs(n64(dx2)[keep] - r_dx2) <= e["dx"][keep][:, K1:]).all()


def test_accumulate_and_determinism(dev):
    M, K1, K2, C = 300, 132, 124, 158
    _, d, gd, fw, bw = run_tiled(dev, M, K1, K2, C, 1.0)
    _, _, _, fw2, bw2 = run_tiled(dev, M, K1, K2, C, 1.0)
    assert all(torch.equal(p, q) for p, q in zip(fw, fw2)) and all(torch.equal(p, q) for p, q in zip(bw, bw2))
    # accumulate: buffer + fresh result, one rounding of the sum (1 ulp); dX is not touched by the flag
    g0 = torch.Generator().manual_seed(5)
    dW0, db0 = torch.randn(C, K1 + K2, generator=g0).to(dev), torch.randn(C, generator=g0).to(dev)
    bw3 = raw_bwd(dev, *d, fw[0], gd, init=(dW0, db0), tiled=True)
    for got, base, fresh in ((bw3[0], dW0, bw[0]), (bw3[1], db0, bw[1])):
        want = base.double() + fresh.double()
        ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126, dtype=torch.float64, device=dev)) * 2.0 ** -23
        assert ((got.double() - want).abs() <= ulp).all()
    assert torch.equal(bw3[2], bw[2]) and torch.equal(bw3[3], bw[3])


def test_backward_over_two_row_slabs_at_the_class_limit(dev):
    """C = 65536, the class limit: G's pitch is 256 KiB, so a 128 MiB backward slab holds 512 rows and 577 rows are a full
    slab and a shorter one of 65 rows (two row blocks).  The second slab runs the row offsets of labels / lse / X / dX and
    the accumulation of dW / dbias over slabs; `accumulate` on top of that adds to pre-filled buffers.  (The f64 restatement
    of 38 M logits is what this test's seconds go to; it is computed once.)"""
    M, K1, K2, C = 577, 4, 0, 65536
    g = 0.75
    (x1, x2, w, b, lab), d, gd, (lse, tgt, pred), (dW, db, dx1, _) = run_tiled(dev, M, K1, K2, C, g)
    a = [n64(t) for t in (x1, x2, w, b)]
    r_lse, r_tgt, r_pred, r_z = R.fwd(a[0], a[2], a[3], lab.numpy())
    rG = R.grad_logits(r_z, r_lse, lab.numpy(), g)
    e = bounds(a[0], None, a[2], a[3], lab.numpy(), g)
    worst = {}

    def close(name, got, ref, bound):
        err = np.abs(n64(got) - ref)
        worst[name] = float((err / np.maximum(bound, 1e-300)).max())
        assert (err <= bound).all(), (name, float(err.max()), worst[name])

    close("lse", lse, r_lse, e["lse"])
    close("tgt", tgt, r_tgt, e["tgt"])
    close("dW", dW, rG.T @ a[0], e["dW"])
    close("dbias", db, rG.sum(axis=0), e["db"])
    close("dx1", dx1, rG @ a[2], e["dx"])
    sure = sure_rows(r_z, e["z"])
    print(f"linear_ce_tiled {(M, K1, K2, C)}: worst error / bound {worst}; pred compared on {int(sure.sum())} of {M} rows")
    assert (~sure).sum() <= 0.10 * M and np.array_equal(pred.cpu().numpy()[sure], r_pred[sure])
    assert dx1[512:].any() and db.any()                      # the second slab did write
    # a second call has the same bits
    bw2 = raw_bwd(dev, *d, lse, gd, tiled=True)
    assert torch.equal(bw2[0], dW) and torch.equal(bw2[1], db) and torch.equal(bw2[2], dx1)
    # accumulate over two slabs is fl(fl(base + s1) + s2) against base + fl(s1 + s2): three roundings of at most u times
    # |base + s1|, |result| and |s1 + s2|, each below |base| + A with A = sum_i |G x| >= |s1| + |s2|
    g0 = torch.Generator().manual_seed(6)
    dW0, db0 = torch.randn(C, K1, generator=g0).to(dev), torch.randn(C, generator=g0).to(dev)
    bw3 = raw_bwd(dev, *d, lse, gd, init=(dW0, db0), tiled=True)
    for got, base, fresh, A in ((bw3[0], dW0, dW, np.abs(rG).T @ np.abs(a[0])), (bw3[1], db0, db, np.abs(rG).sum(axis=0))):
        tol = 3.0 * U * 1.001 * (np.abs(n64(base)) + A)
        assert (np.abs(n64(got) - (n64(base) + n64(fresh))) <= tol).all()


def test_each_output_alone_has_the_bits_of_the_full_call(dev):
    """dW only, dbias only, dX only: the weight-gradient kernel's null-partials branches.  Nothing is atomic, so each
    output has the bits it has when every output is asked for (canaries inside raw_bwd)."""
    _, d, gd, fw, (dW, db, dx1, dx2) = run_tiled(dev, 65, 132, 124, 127, 0.75)
    only = lambda **kw: raw_bwd(dev, *d, fw[0], gd, tiled=True, **kw)
    o = only(want_db=False, want_dx=False)
    assert torch.equal(o[0], dW) and o[1] is None and o[2] is None and o[3] is None
    o = only(want_dw=False, want_dx=False)
    assert torch.equal(o[1], db) and o[0] is None and o[2] is None and o[3] is None
    o = only(want_dw=False, want_db=False)
    assert torch.equal(o[2], dx1) and torch.equal(o[3], dx2) and o[0] is None and o[1] is None


@pytest.mark.parametrize("C", [17, 64])
def test_agreement_with_the_64_class_kernels(dev, C):
    """Both kernels are within bounds() of the exact result, so within twice the bound of each other; bits may differ."""
    M, K1, K2 = 257, 132, 124
    g = 0.75
    (x1, x2, w, b, lab), d, gd, (lse, tgt, pred), bw = run_tiled(dev, M, K1, K2, C, g)
    o_lse, o_tgt, o_pred, o_z = raw_fwd(dev, *d)
    o_bw = raw_bwd(dev, *d, o_lse, gd)
    a = [n64(t) for t in (x1, x2, w, b)]
    e = bounds(a[0], a[1], a[2], a[3], lab.numpy(), g)
    assert (np.abs(n64(lse) - n64(o_lse)) <= 2 * e["lse"]).all() and (np.abs(n64(tgt) - n64(o_tgt)) <= 2 * e["tgt"]).all()
    for got, old, bound in zip(bw, o_bw, (e["dW"], e["db"], e["dx"][:, :K1], e["dx"][:, K1:])):
        assert (np.abs(n64(got) - n64(old)) <= 2 * bound).all()
    sure = sure_rows(R.logits(a[0], a[2], a[3], a[1]), e["z"])
    assert torch.equal(pred.cpu()[sure], o_pred.cpu()[sure])


# ---- heads at the reference's 158 markers.  Bars: those of tests/test_gpu_classifier.py for the heads (the exact-f32
# models' bars of tests/test_gpu_models.py): loss 1e-4, gradients 2e-4 of the parameter's largest, floored at 1e-3 of the
# model's largest.
def _data(M=96, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, 256, generator=g), torch.randint(0, 158, (M,), generator=g)


def _check_head_against_f64(dev, m, x, labels, x2_split):
    m64 = copy.deepcopy(m).double()
    m = m.to(dev)
    xd, ld = x.to(dev), labels.to(dev)
    if x2_split:
        loss, pred = m.loss(xd[:, :128].contiguous(), ld, x2=xd[:, 128:].contiguous(), return_pred=True)
        assert torch.equal(pred, m.predict(xd[:, :128].contiguous(), x2=xd[:, 128:].contiguous()))
    else:
        loss, pred = m.loss(xd, ld, return_pred=True)
        assert torch.equal(pred, m.predict(xd))
    loss.backward()
    # f64: the torch modules of the same state dict (eval mode: no dropout)
    h = x.double()
    if hasattr(m64, "mlp"):
        h = m64.mlp(h)
    else:
        h = m64.linear(h)
    ref = F.cross_entropy(h, labels)
    ref.backward()
    assert abs(loss.item() - ref.item()) < 1e-4, (loss.item(), ref.item())
    grads = {n: p.grad for n, p in m64.named_parameters()}
    gmax = max(g.abs().max().item() for g in grads.values())
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        err = (p.grad.cpu().double() - grads[n]).abs().max().item()
        assert err <= 2e-4 * max(grads[n].abs().max().item(), 1e-3 * gmax), (n, err)
    # predict against the argmax of head(x): both evaluate the last Linear on the same features within the logit bound
    with torch.no_grad():
        feats = m.features(xd.float().contiguous())
        logits = m(xd)
    last = m._last()
    f, w, b = n64(feats), n64(last.weight), n64(last.bias)
    z = R.logits(f, w, b)
    ez = (w.shape[1] + 4) * U * R.abs_logits(f, w, b)
    sure = sure_rows(z, ez)
    assert (~sure).sum() <= 0.10 * len(sure)
    assert torch.equal(pred.cpu()[sure], logits.argmax(1).cpu()[sure])
    assert pred.dtype == torch.int64 and not pred.requires_grad


def test_linear_head_at_158_classes(dev):
    import clip_dplm_amd as K
    torch.manual_seed(0)
    x, labels = _data()
    _check_head_against_f64(dev, K.LinearClassifier(256, 158), x, labels, x2_split=True)


def test_mlp_head_at_158_classes(dev):
    import clip_dplm_amd as K
    torch.manual_seed(0)
    x, labels = _data()
    _check_head_against_f64(dev, K.MLPClassifier(256, [64], 158).eval(), x, labels, x2_split=False)


def test_training_against_f64_adam_at_158_classes(dev):
    """Ten FusedAdamW steps through the tiled loss against f64 Adam.  The bar is four times the largest gap of a float32
    CPU torch run of the same ten steps from the f64 run: two valid f32 evaluation orders differ from f64 by a small
    multiple of either's own error."""
    import clip_dplm_amd as K
    torch.manual_seed(0)
    x, labels = _data(64, seed=2)
    m = K.LinearClassifier(256, 158)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    lr, steps = 1e-3, 10
    want = _f64_adam_losses(sd, x, labels, steps, lr)
    # float32 on the CPU
    w = sd["linear.weight"].clone().requires_grad_(True)
    b = sd["linear.bias"].clone().requires_grad_(True)
    opt32 = torch.optim.Adam([w, b], lr=lr)
    cpu = []
    for _ in range(steps):
        opt32.zero_grad()
        loss = F.cross_entropy(F.linear(x, w, b), labels)
        loss.backward()
        opt32.step()
        cpu.append(loss.item())
    bar = 4.0 * max(abs(p - q) for p, q in zip(cpu, want))
    m = m.to(dev).train()
    opt = K.FusedAdamW(m, lr=lr, weight_decay=0.0, max_grad_norm=None)
    xa, xb, ld = x[:, :128].contiguous().to(dev), x[:, 128:].contiguous().to(dev), labels.to(dev)
    got = []
    for _ in range(steps):
        opt.zero_grad()
        loss = m.loss(xa, ld, x2=xb)
        loss.backward()
        opt.step()
        got.append(loss.item())
    gaps = [abs(p - q) for p, q in zip(got, want)]
    print(f"wide probe training: max |loss - f64 loss| over {steps} steps {max(gaps):.3e} (bar {bar:.3e} = 4 x the f32 CPU "
          f"run's {bar / 4:.3e}); losses {got[0]:.6f} -> {got[-1]:.6f}")
    assert want[-1] < want[0] and got[-1] < got[0]
    assert max(gaps) <= bar, (gaps, bar)


def test_captured_loss_and_backward_replay_bitwise(dev):
    import clip_dplm_amd as K
    from clip_dplm_amd import ops
    torch.manual_seed(0)
    x, labels = _data(64, seed=4)
    m = K.LinearClassifier(256, 158).to(dev)
    xa, xb, ld = x[:, :128].contiguous().to(dev), x[:, 128:].contiguous().to(dev), labels.to(dev)
    for p in m.parameters():
        p.grad = torch.zeros_like(p)                       # the kernels add into existing .grad buffers

    def body():
        for p in m.parameters():
            p.grad.zero_()
        loss = m.loss(xa, ld, x2=xb)
        loss.backward()
        return loss.detach()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            eager = body().clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ge = [p.grad.clone() for p in m.parameters()]
    graph, keep = torch.cuda.CUDAGraph(), []
    with ops.owned_by_capture(keep), torch.cuda.graph(graph):
        static_loss = body()
    for p in m.parameters():
        p.grad.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_loss, eager) and all(torch.equal(p.grad, q) for p, q in zip(m.parameters(), ge))
    assert ge[0].abs().max().item() > 0


def test_probe_loop_at_158_classes(dev):
    import clip_dplm_amd as K
    from clip_dplm_amd import probe

    class Frozen(torch.nn.Module):
        """Stands for a frozen CLIP model: hands its two inputs back as the embeddings."""

        def __init__(self):
            super().__init__()
            self.dummy = torch.nn.Parameter(torch.zeros(1))

        def forward(self, a, b):
            return {"logits_per_rna_protein": None, "rna_embeds": a, "protein_embeds": b}

    clip = Frozen().to(dev)
    torch.manual_seed(0)
    x, labels = _data(40, seed=5)
    loader = [(x[i:j, :128], x[i:j, 128:], labels[i:j]) for i, j in ((0, 14), (14, 28), (28, 40))]
    m = K.LinearClassifier(256, 158).to(dev)
    opt = K.FusedAdamW(m, lr=1e-2, weight_decay=0.0, max_grad_norm=None)
    first = m.loss(x[:, :128].contiguous().to(dev), labels.to(dev), x2=x[:, 128:].contiguous().to(dev)).item()
    last = probe.train_classifier(clip, m, loader, opt, 5, dev)
    assert torch.isfinite(last) and last.item() < first
    acc = probe.evaluate(clip, m, loader, dev)
    logits = m.eval()(x.to(dev)).cpu()
    top2 = logits.topk(2, dim=1).values
    assert ((top2[:, 0] - top2[:, 1]) > 1e-4).all()          # no row near a tie: the two argmaxes must agree
    assert acc == (logits.argmax(1) == labels).sum().item() / 40
