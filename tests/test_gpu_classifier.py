"""GPU tests of the classifier probes: the fused Linear + cross-entropy kernels against the f64 restatement
(tests/linear_ce_ref.py) with bounds derived from u = 2^-24, the four heads against the reference fixture, training
against f64 Adam, the captured step, and probe.evaluate."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import classifier_ref
import linear_ce_ref as R

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24
KSTEP = 16            # LCE_KSTEP of clip_dplm_amd/csrc/linear_ce.hip: contraction columns per main-loop step
WCOLS = 64            # LCE_WCOLS of csrc/linear_ce_bwd.h: dW columns per wave of the weight-gradient kernel
PAD = 64              # canary elements on each side of every output buffer

SHAPES = [(1, 4, 0, 1), (37, 128, 128, 7), (64, 256, 0, 16), (65, 132, 124, 17), (257, 512, 512, 64), (1000, 36, 0, 33),
          (33, KSTEP, 0, 5), (33, KSTEP + 4, 0, 5), (33, WCOLS, 0, 5), (33, WCOLS + 4, 0, 5)]


def make(M, K1, K2, C, seed=0, dev="cuda"):
    g = torch.Generator().manual_seed(1000 * seed + M + K1 + K2 + C)
    K = K1 + K2
    x1 = torch.randn(M, K1, generator=g)
    x2 = torch.randn(M, K2, generator=g) if K2 else None
    w = torch.randn(C, K, generator=g) * K ** -0.5
    b = torch.randn(C, generator=g)
    labels = torch.randint(0, C, (M,), generator=g)
    return x1, x2, w, b, labels


class Arena:
    """Output buffers with canary words on both sides, for calls straight into the C ABI."""

    def __init__(self, dev):
        self.dev, self.bufs = dev, []

    def out(self, n, dtype=torch.float32):
        canary = 12345.0 if dtype.is_floating_point else (0x5A if dtype == torch.uint8 else 0x5A5A5A5A5A5A5A5A)
        full = torch.full((n + 2 * PAD,), canary, dtype=dtype, device=self.dev)
        self.bufs.append((full, n, canary))
        return full[PAD:PAD + n]

    def intact(self):
        return all(bool((f[:PAD] == c).all()) and bool((f[PAD + n:] == c).all()) for f, n, c in self.bufs)


def raw_fwd(dev, x1, x2, w, b, labels, want_logits=True, ldz=None, tiled=False):
    """tiled: clipk_linear_ce_tiled_fwd on exactly its workspace bytes; it has no logits output, so three results."""
    from clip_dplm_amd import _ffi, ops
    lib = _ffi.load()
    M, K1 = x1.shape
    K2 = 0 if x2 is None else x2.shape[1]
    C = w.shape[0]
    ldz = C if ldz is None else ldz
    a = Arena(dev)
    lse, tgt, pred = a.out(M), a.out(M), a.out(M, torch.int64)
    head = (x1.data_ptr(), K1, _ffi.ptr(x2), K2, w.data_ptr(), _ffi.ptr(b), labels.data_ptr(), M, C, lse.data_ptr(),
            tgt.data_ptr(), pred.data_ptr())
    if tiled:
        nws = lib.clipk_linear_ce_tiled_workspace(M, K1, K2, C)
        assert nws > 0
        ws = a.out(nws, torch.uint8)                       # exactly the bytes the helper asks for, guard words around
        _ffi.check(lib.clipk_linear_ce_tiled_fwd(*head, ws.data_ptr(), nws, ops._stream()), "clipk_linear_ce_tiled_fwd")
    else:
        logits = a.out(M * ldz) if want_logits else None
        _ffi.check(lib.clipk_linear_ce_fwd(*head, _ffi.ptr(logits), ldz, ops._stream()), "clipk_linear_ce_fwd")
    torch.cuda.synchronize()
    assert a.intact()
    if tiled:
        return lse, tgt, pred
    return lse, tgt, pred, (None if logits is None else logits.view(M, ldz))


def raw_bwd(dev, x1, x2, w, b, labels, lse, g, want_dx=True, init=None, tiled=False, want_dw=True, want_db=True):
    """init: (dW0, db0) to accumulate onto.  tiled: clipk_linear_ce_tiled_bwd and its workspace helper."""
    from clip_dplm_amd import _ffi, ops
    lib = _ffi.load()
    M, K1 = x1.shape
    K2 = 0 if x2 is None else x2.shape[1]
    C, K = w.shape
    a = Arena(dev)
    dW = a.out(C * K) if want_dw else None
    db = a.out(C) if want_db else None
    if init is not None:
        dW.copy_(init[0].reshape(-1))
        db.copy_(init[1])
    dx1 = a.out(M * K1) if want_dx else None
    dx2 = a.out(M * K2) if want_dx and K2 else None
    name = "clipk_linear_ce_tiled" if tiled else "clipk_linear_ce"
    nws = getattr(lib, name + "_workspace")(M, K1, K2, C)
    assert nws > 0
    ws = a.out(nws, torch.uint8)                           # exactly the bytes the helper asks for, guard words around
    _ffi.check(getattr(lib, name + "_bwd")(x1.data_ptr(), K1, _ffi.ptr(x2), K2, w.data_ptr(), _ffi.ptr(b), labels.data_ptr(), M, C,
                                           lse.data_ptr(), g.data_ptr(), int(init is not None), _ffi.ptr(dW), _ffi.ptr(db),
                                           _ffi.ptr(dx1), _ffi.ptr(dx2), ws.data_ptr(), nws, ops._stream()), name + "_bwd")
    torch.cuda.synchronize()
    assert a.intact()
    return (None if dW is None else dW.view(C, K), db, None if dx1 is None else dx1.view(M, K1),
            None if dx2 is None else dx2.view(M, K2))


def bounds(x1, x2, w, b, labels, g):
    """Error bounds of every output from u = 2^-24 (include/clipk.h: clipk_linear_ce_*), f64 numpy.
    Logit: a chain of K fused multiply-adds and the bias addition, |Z~ - Z| <= (K + 4) u (sum |x w| + |b|) = eZ.
    lse is 1-Lipschitz in max_c |dZ|; its own exp / sum over C / log / final addition cost (C + 8) u (1 + |lse|).
    G = g/M (exp(Z - lse) - onehot): the exponent is off by d = eZ + e_lse + u |Z - lse|, expf and the three roundings
    after it by 4 u: eG = |g|/M (p (expm1(d) + 4 u) + 4 u).
    dW / dbias: sum_i eG |x| plus the summation of M terms in an order that is not pinned down (MFMA chain per split, split
    sum, optional accumulate): gamma_n = n 2^-23 with n = M + 8, relative to sum_i |G x|.  dX: the same over the C classes."""
    M, C = x1.shape[0], w.shape[0]
    K = w.shape[1]
    lse, tgt, pred, z = R.fwd(x1, w, b, labels, x2)
    eZ = (K + 4) * U * R.abs_logits(x1, w, b, x2)
    e_lse = eZ.max(axis=1) + (C + 8) * U * (1 + np.abs(lse))
    lab = np.asarray(labels)
    ok = (lab >= 0) & (lab < C)
    e_tgt = np.zeros(M)
    e_tgt[ok] = eZ[np.nonzero(ok)[0], lab[ok]]
    p = np.exp(z - lse[:, None])
    d = eZ + e_lse[:, None] + U * np.abs(z - lse[:, None])
    eG = abs(g) / M * (p * (np.expm1(d) + 4 * U) + 4 * U)
    eG[~ok] = 0.0
    Gm = np.abs(R.grad_logits(z, lse, lab, g))
    xa = np.abs(R._cat(x1, x2))
    wa = np.abs(np.asarray(w, np.float64))
    e_dW = eG.T @ xa + (M + 8) * 2.0 ** -23 * (Gm.T @ xa)
    e_db = eG.sum(0) + (M + 8) * 2.0 ** -23 * Gm.sum(0)
    e_dx = eG @ wa + (C + 4) * 2.0 ** -23 * (Gm @ wa)
    return dict(z=eZ, lse=e_lse, tgt=e_tgt, dW=e_dW, db=e_db, dx=e_dx)


def n64(t):
    return None if t is None else t.detach().cpu().double().numpy()


def run_case(dev, M, K1, K2, C, g=1.0, labels=None, seed=0):
    x1, x2, w, b, lab = make(M, K1, K2, C, seed)
    lab = lab if labels is None else labels
    d = [None if t is None else t.to(dev) for t in (x1, x2, w, b, lab)]
    gd = torch.tensor([g], dtype=torch.float32, device=dev)
    fw = raw_fwd(dev, *d)
    bw = raw_bwd(dev, *d, fw[0], gd)
    return (x1, x2, w, b, lab), d, gd, fw, bw


@pytest.mark.parametrize("M,K1,K2,C", SHAPES)
def test_kernels_against_f64_restatement(dev, M, K1, K2, C):
    g = 0.75
    (x1, x2, w, b, lab), d, gd, (lse, tgt, pred, logits), (dW, db, dx1, dx2) = run_case(dev, M, K1, K2, C, g)
    a = [n64(t) for t in (x1, x2, w, b)]
    r_lse, r_tgt, r_pred, r_z = R.fwd(a[0], a[2], a[3], lab.numpy(), a[1])
    r_dW, r_db, r_dx1, r_dx2, _ = R.bwd(a[0], a[2], a[3], lab.numpy(), g, a[1])
    e = bounds(a[0], a[1], a[2], a[3], lab.numpy(), g)
    worst = {}

    def close(name, got, ref, bound):
        err = np.abs(n64(got) - ref)
        worst[name] = float((err / np.maximum(bound, 1e-300)).max())
        assert (err <= bound).all(), (name, float(err.max()), worst[name])

    close("logits", logits, r_z, e["z"])
    close("lse", lse, r_lse, e["lse"])
    close("tgt", tgt, r_tgt, e["tgt"])
    close("dW", dW, r_dW, e["dW"])
    close("dbias", db, r_db, e["db"])
    K = K1 + K2
    close("dx1", dx1, r_dx1, e["dx"][:, :K1])
    if K2:
        close("dx2", dx2, r_dx2, e["dx"][:, K1:])
    print(f"linear_ce {(M, K1, K2, C)}: worst error / bound {worst}")
    # pred: the first-occurrence argmax of the logits the same call returned, bitwise
    assert torch.equal(pred.cpu(), torch.from_numpy(R.first_argmax(logits.cpu().numpy())))
    # the mean loss through clipk_ce_combine
    from clip_dplm_amd import ops
    loss = ops.ce_combine(lse, tgt, None, None, 1.0, 0.0, float(M)).item()
    assert abs(loss - R.mean_loss(r_lse, r_tgt)) <= (e["lse"] + e["tgt"]).mean() + (M + 4) * U * np.abs(r_lse - r_tgt).mean() + 1e-30


def test_ties_resolve_to_the_lower_class(dev):
    M, K, C = 70, 24, 19
    x1, _, w, b, lab = make(M, K, 0, C, seed=2)
    w[17], b[17] = w[3], b[3]                              # classes 3 and 17 (two class tiles) tie on every row
    w[4], b[4] = w[3], b[3]                                # and 3 and 4 inside one tile
    w[3] *= 4.0
    w[4] *= 4.0
    w[17] *= 4.0                                           # make the tied classes win on many rows
    d = [t.to(dev) for t in (x1, w, b, lab)]
    lse, tgt, pred, logits = raw_fwd(dev, d[0], None, d[1], d[2], d[3])
    z = logits.cpu()
    assert torch.equal(z[:, 3], z[:, 4]) and torch.equal(z[:, 3], z[:, 17])
    assert torch.equal(pred.cpu(), torch.max(z, 1)[1]) and torch.equal(pred.cpu(), torch.from_numpy(R.first_argmax(z.numpy())))
    assert (pred == 3).sum().item() > 5 and not ((pred == 4) | (pred == 17)).any()


def test_determinism_accumulate_and_null_outputs(dev):
    M, K1, K2, C = 300, 132, 124, 17
    _, d, gd, fw, bw = run_case(dev, M, K1, K2, C, 1.0)
    _, _, _, fw2, bw2 = run_case(dev, M, K1, K2, C, 1.0)
    assert torch.equal(fw[0], fw2[0]) and all(torch.equal(p, q) for p, q in zip(bw, bw2))
    # logits = NULL / dX = NULL: the other outputs keep their bits
    fw3 = raw_fwd(dev, *d, want_logits=False)
    assert all(torch.equal(p, q) for p, q in zip(fw[:3], fw3[:3]))
    bw3 = raw_bwd(dev, *d, fw[0], gd, want_dx=False)
    assert torch.equal(bw[0], bw3[0]) and torch.equal(bw[1], bw3[1])
    # a leading dimension wider than C
    fw4 = raw_fwd(dev, *d, ldz=C + 3)
    assert torch.equal(fw4[3][:, :C], fw[3]) and bool((fw4[3][:, C:] == 12345.0).all())
    # accumulate: buffer + fresh result, one rounding of the sum (1 ulp)
    g0 = torch.Generator().manual_seed(5)
    dW0, db0 = torch.randn(C, K1 + K2, generator=g0).to(dev), torch.randn(C, generator=g0).to(dev)
    bw5 = raw_bwd(dev, *d, fw[0], gd, init=(dW0, db0))
    for got, base, fresh in ((bw5[0], dW0, bw[0]), (bw5[1], db0, bw[1])):
        want = base.double() + fresh.double()
        ulp = torch.maximum(want.abs(), torch.tensor(2.0 ** -126, dtype=torch.float64, device=dev)) * 2.0 ** -23
        assert ((got.double() - want).abs() <= ulp).all()


def test_out_of_range_labels(dev):
    M, K1, K2, C = 150, 64, 36, 11
    x1, x2, w, b, lab = make(M, K1, K2, C, seed=3)
    lab[17], lab[101] = C, -1
    _, d, gd, (lse, tgt, pred, logits), (dW, db, dx1, dx2) = run_case(dev, M, K1, K2, C, 1.0, labels=lab, seed=3)   # (canaries inside)
    assert torch.isnan(tgt[[17, 101]]).all() and torch.isfinite(tgt).sum().item() == M - 2
    assert torch.equal(pred.cpu(), torch.max(logits.cpu(), 1)[1])
    from clip_dplm_amd import ops
    assert torch.isnan(ops.ce_combine(lse, tgt, None, None, 1.0, 0.0, float(M)))
    assert not dx1[[17, 101]].any() and not dx2[[17, 101]].any()
    # the gradients of the batch without the two rows, at the full batch's 1 / M
    keep = [i for i in range(M) if i not in (17, 101)]
    a = [n64(t) for t in (x1, x2, w, b)]
    r_dW, r_db, r_dx1, r_dx2, _ = R.bwd(a[0][keep], a[2], a[3], lab.numpy()[keep], len(keep) / M, a[1][keep])
    e = bounds(a[0], a[1], a[2], a[3], lab.numpy(), 1.0)
    assert (np.abs(n64(dW) - r_dW) <= e["dW"]).all() and (np.abs(n64(db) - r_db) <= e["db"]).all()
    assert (np.abs(n64(dx1)[keep] - r_dx1) <= e["dx"][keep][:, :K1]).all()
    assert (np.abs(n64(dx2)[keep] - r_dx2) <= e["dx"][keep][:, K1:]).all()


# ---- the four heads against the reference fixture (bars of tests/test_gpu_models.py for the exact-f32 notebook models:
# loss and values 1e-4, gradients 2e-4 of the parameter's largest, floored at 1e-3 of the model's largest)
CTOR = {"mlp": ("MLPClassifier", (256, [64, 32], 7), {}),
        "transformer": ("TransformerClassifier", (256, 32, 7), {"num_layers": 1, "num_heads": 4}),
        "linear": ("LinearClassifier", (256, 7), {}),
        "simple": ("SimpleNonLinearClassifier", (256, 64, 7), {})}


@pytest.fixture(scope="module")
def fixture():
    return classifier_ref.load_fixture(G)


@pytest.mark.parametrize("tag", list(CTOR))
def test_heads_against_reference_fixture(dev, fixture, tag):
    import clip_dplm_amd as K
    heads, x, labels = fixture
    f = heads[tag]
    cls, a, kw = CTOR[tag]
    m = getattr(K, cls)(*a, **kw)
    m.load_state_dict(f["sd"])
    m = m.to(dev).eval()
    xd, ld = x.to(dev), labels.to(dev)
    logits = m(xd)
    e_logits = (logits.detach().cpu() - f["logits"]).abs().max().item()
    loss, pred = m.loss(xd, ld, return_pred=True)
    e_loss = abs(loss.item() - f["loss"])
    print(f"{tag}: max |dlogits| {e_logits:.2e}, |dloss| {e_loss:.2e}")
    assert e_logits < 1e-4 and e_loss < 1e-4
    assert abs(F.cross_entropy(logits, ld).item() - loss.item()) < 1e-5
    assert torch.equal(pred, m.predict(xd)) and pred.dtype == torch.int64 and not pred.requires_grad
    # predictions: the argmax of the logits wherever the two best logits are further apart than the bar
    top2 = logits.detach().topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2e-4
    assert torch.equal(pred[sure], logits.detach().argmax(1)[sure])
    loss.backward()
    gmax = max(g.abs().max().item() for g in f["grads"].values())
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        ref = f["grads"][n]
        err = (p.grad.cpu() - ref).abs().max().item()
        assert err <= 2e-4 * max(ref.abs().max().item(), 1e-3 * gmax), (n, err)
    if tag == "transformer":
        for n in ("in_proj_weight", "in_proj_bias"):
            gq = getattr(m.transformer_encoder.layers[0].self_attn, n).grad
            assert not gq[:64].any() and gq[64:].any()      # q and k rows: exact zeros, not None
    if tag == "linear":                                     # two sources in place == the concatenation
        l2 = m.loss(xd[:, :128].contiguous(), ld, x2=xd[:, 128:].contiguous())
        assert torch.equal(l2, loss.detach())
    else:
        l2 = m.loss(xd[:, :128], ld, x2=xd[:, 128:])
        assert torch.equal(l2.detach(), loss.detach())


def test_input_gradients_only_where_required(dev, fixture):
    import clip_dplm_amd as K
    from clip_dplm_amd import functional as KF
    heads, x, labels = fixture
    m = K.LinearClassifier(256, 7)
    m.load_state_dict(heads["linear"]["sd"])
    m = m.to(dev)
    xa = x[:, :128].to(dev).contiguous().requires_grad_(True)
    xb = x[:, 128:].to(dev).contiguous()
    KF.linear_cross_entropy(xa, m.linear.weight, m.linear.bias, labels.to(dev), x2=xb).backward()
    xr = x.clone().requires_grad_(True)
    F.cross_entropy(F.linear(xr, heads["linear"]["sd"]["linear.weight"], heads["linear"]["sd"]["linear.bias"]), labels).backward()
    assert xb.grad is None and (xa.grad.cpu() - xr.grad[:, :128]).abs().max().item() <= 2e-4 * xr.grad.abs().max().item()
    assert (m.linear.weight.grad.cpu() - heads["linear"]["grads"]["linear.weight"]).abs().max().item() < 2e-4 * \
        heads["linear"]["grads"]["linear.weight"].abs().max().item()


# ---- training
TRAIN_GAP = 5.24e-7   # allowed |loss_gpu - loss_f64| per step: twice the 2.620e-07 measured on an MI355X (profiles/probe/README.md)


def _f64_adam_losses(sd, x, labels, steps, lr):
    w = sd["linear.weight"].double().clone().requires_grad_(True)
    b = sd["linear.bias"].double().clone().requires_grad_(True)
    opt = torch.optim.Adam([w, b], lr=lr)
    xs, lab = x.double().numpy(), labels.numpy()
    out = []
    for _ in range(steps):
        lse, tgt, _, _ = R.fwd(xs, w.detach().numpy(), b.detach().numpy(), lab)
        out.append(R.mean_loss(lse, tgt))
        dW, db, _, _, _ = R.bwd(xs, w.detach().numpy(), b.detach().numpy(), lab)
        w.grad, b.grad = torch.from_numpy(dW), torch.from_numpy(db)
        opt.step()
    return out


def _linear_head(dev, fixture):
    import clip_dplm_amd as K
    heads, x, labels = fixture
    m = K.LinearClassifier(256, 7)
    m.load_state_dict(heads["linear"]["sd"])
    m = m.to(dev).train()
    return m, K.FusedAdamW(m, lr=1e-4, weight_decay=0.0, max_grad_norm=None), x.to(dev), labels.to(dev)


def test_training_against_f64_adam(dev, fixture):
    heads, x, labels = fixture
    m, opt, xd, ld = _linear_head(dev, fixture)
    want = _f64_adam_losses(heads["linear"]["sd"], x, labels, 10, 1e-4)
    got = []
    for _ in range(10):
        opt.zero_grad()
        loss = m.loss(xd, ld)
        loss.backward()
        opt.step()
        got.append(loss.item())
    gaps = [abs(a - b) for a, b in zip(got, want)]
    print(f"probe training: max |loss - f64 loss| over 10 steps {max(gaps):.3e}; losses {got[0]:.6f} -> {got[-1]:.6f}")
    assert want[-1] < want[0] and got[-1] < got[0]
    assert max(gaps) <= TRAIN_GAP, gaps


def test_graphed_step_reproduces_eager(dev, fixture):
    import clip_dplm_amd as K
    m, opt, xd, ld = _linear_head(dev, fixture)
    eager = []
    for _ in range(3):
        opt.zero_grad()
        loss = m.loss(xd, ld)
        loss.backward()
        opt.step()
        eager.append(loss.item())
    m2, opt2, _, _ = _linear_head(dev, fixture)
    step = K.GraphedTrainStep(m2, opt2, lambda a, b: m2.loss(a, b), (xd, ld))
    replay = [step(xd, ld).item() for _ in range(3)]
    assert max(abs(a - b) for a, b in zip(eager, replay)) <= 1e-6, (eager, replay)
    assert eager[2] < eager[0]


def test_probe_evaluate_matches_host_accuracy(dev, fixture):
    import clip_dplm_amd as K
    from clip_dplm_amd import probe
    heads, x, labels = fixture

    class Frozen(torch.nn.Module):
        """Stands for a frozen CLIP model: hands its two inputs back as the embeddings."""

        def __init__(self):
            super().__init__()
            self.dummy = torch.nn.Parameter(torch.zeros(1))

        def forward(self, a, b):
            return {"logits_per_rna_protein": None, "rna_embeds": a, "protein_embeds": b}

    clip = Frozen().to(dev)
    m = K.SimpleNonLinearClassifier(256, 64, 7)
    m.load_state_dict(heads["simple"]["sd"])
    m = m.to(dev)
    loader = [(x[i:j, :128], x[i:j, 128:], labels[i:j]) for i, j in ((0, 13), (13, 26), (26, 37))]
    acc = probe.evaluate(clip, m, loader, dev)
    logits = m.eval()(x.to(dev)).cpu()
    assert acc == (logits.argmax(1) == labels).sum().item() / 37
    mlin = K.LinearClassifier(256, 7)
    mlin.load_state_dict(heads["linear"]["sd"])
    mlin = mlin.to(dev)
    opt = K.FusedAdamW(mlin, lr=1e-2, weight_decay=0.0, max_grad_norm=None)
    before = probe.evaluate(clip, mlin, loader, dev)
    probe.train_classifier(clip, mlin, loader, opt, 20, dev)
    assert probe.evaluate(clip, mlin, loader, dev) > before


def test_mixed_in_place_and_autograd_parameter_gradients(dev, fixture):
    """weight.grad exists (the kernels add into it), bias.grad does not (autograd gets a tensor): one backward call."""
    import clip_dplm_amd as K
    heads, x, labels = fixture
    f = heads["linear"]
    m = K.LinearClassifier(256, 7)
    m.load_state_dict(f["sd"])
    m = m.to(dev)
    m.linear.weight.grad = torch.ones_like(m.linear.weight)
    m.loss(x.to(dev), labels.to(dev)).backward()
    gw, gb = f["grads"]["linear.weight"], f["grads"]["linear.bias"]
    assert (m.linear.weight.grad.cpu() - 1.0 - gw).abs().max().item() <= 2e-4 * gw.abs().max().item() + 2.0 ** -23
    assert (m.linear.bias.grad.cpu() - gb).abs().max().item() <= 2e-4 * gb.abs().max().item()


@pytest.mark.parametrize("tag", ["mlp", "transformer", "simple"])
def test_train_mode_dropout(dev, fixture, tag):
    """train() mode: finite gradients of the right shapes, a fixed seed reproduces, another seed differs, and
    dropout_rate = 0 in train mode is eval mode bit for bit."""
    import clip_dplm_amd as K
    heads, x, labels = fixture
    f = heads[tag]
    cls, a, kw = CTOR[tag]
    xd, ld = x.to(dev), labels.to(dev)

    def run(p, seed, train=True):
        m = getattr(K, cls)(*a, dropout_rate=p, **kw)
        m.load_state_dict(f["sd"])
        m = m.to(dev).train(train)
        torch.manual_seed(seed)
        logits = m(xd)
        torch.manual_seed(seed)
        loss = m.loss(xd, ld)
        loss.backward()
        return m, logits.detach(), loss.detach()

    m1, z1, l1 = run(0.1, 11)
    m2, z2, l2 = run(0.1, 11)
    m3, z3, l3 = run(0.1, 12)
    assert z1.shape == (37, 7) and torch.isfinite(z1).all() and torch.isfinite(l1)
    assert torch.equal(z1, z2) and torch.equal(l1, l2) and not torch.equal(z1, z3)
    assert abs(F.cross_entropy(z1, ld).item() - l1.item()) < 1e-5       # forward() and loss() drew the same masks
    for (n, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        assert p1.grad is not None and p1.grad.shape == p1.shape and torch.isfinite(p1.grad).all(), n
        assert torch.equal(p1.grad, p2.grad), n
    assert (z1 - heads[tag]["logits"].to(dev)).abs().max().item() > 1e-3        # dropout did drop
    m0, z0, l0 = run(0.0, 11)
    me, ze, le = run(0.0, 11, train=False)
    assert torch.equal(z0, ze) and torch.equal(l0, le)
    assert all(torch.equal(p.grad, q.grad) for p, q in zip(m0.parameters(), me.parameters()))


def test_ablation_study_runs(dev):
    """train_clip -> train_classifier -> evaluate for both CLIP models and all four heads on a toy problem."""
    from types import SimpleNamespace as NS

    from clip_dplm_amd import probe
    sub = lambda h: NS(hidden_size=h, num_hidden_layers=1, layer_norm_eps=1e-12)
    cfg = NS(rna_config=sub(16), protein_config=sub(16), diffmap_config=sub(16), projection_dim=8, logit_scale_init_value=2.6592)
    g = torch.Generator().manual_seed(9)
    n = 48
    rna, prot, diff = (torch.randn(n, 16, generator=g) for _ in range(3))
    labels = torch.randint(0, 3, (n,), generator=g)
    torch.manual_seed(0)
    res = probe.ablation_study(cfg, rna, prot, diff, labels, 3, dev, num_epochs=1, batch_size=16)
    assert len(res) == 8 and all(0.0 <= v <= 1.0 for v in res.values())
    assert set(res) == {f"{c} + {h}" for c in ("RNA-Protein CLIP", "DiffMap-Protein CLIP")
                        for h in ("MLP", "Transformer", "Linear", "SimpleNonLinear")}
