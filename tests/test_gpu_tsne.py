"""GPU: the t-SNE walks (include/clipk.h: clipk_cond_entropy_sums, clipk_tsne_grad, clipk_tsne_update; ops.cond_entropy_sums,
ops.tsne_grad, ops.tsne_update) and clip_dplm_amd.manifold on top of them against the restatement of tests/tsne_ref.py.

Tolerance rule of every comparison (`_close`, the rule of tests/test_gpu_mmd.py): the f64 restatement (d from coordinate
differences) is the reference; the kernel may deviate from it by at most 8 x the deviation of the f32 restatement (d from
the norm expansion, as in the kernel) on the same inputs - the factor covers the different summation order - with a
floor of 64 * 2^-24 x the quantity's magnitude (the largest entry of the reference).  The measured deviations are
printed before each assertion.  A fixed bound would not do: the f32 norm expansion alone moves the entropy by up to 1e-4
at N = 1000, P = 128.

Shapes: N in {3, 63, 65, 130, 1000} (one row block short, one over, three key splits at 130, sixteen blocks), P in
{4, 60, 512} (one K-step, a ragged one, the limit).  The descent is chaotic - f32 and f64 runs of one problem separate
completely within 20 iterations - so steps are compared one at a time from states of the f64 run, and the end-to-end
test asks for the quality of the map, not for its coordinates."""
import functools
import math

import pytest
import torch

from clip_dplm_amd import manifold, ops

import tsne_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F64, F32 = torch.float64, torch.float32
SHAPES = [(N, P) for N in (3, 63, 65, 130, 1000) for P in (4, 60, 512)]


def _close(name, got, r64, r32):
    got, r64, r32 = (torch.as_tensor(t).detach().double().cpu() for t in (got, r64, r32))
    assert got.shape == r64.shape, (name, got.shape, r64.shape)
    assert torch.isfinite(got).all(), name
    dev_k, dev_32 = float((got - r64).abs().max()), float((r32 - r64).abs().max())
    mag = float(r64.abs().max())
    bound = max(8 * dev_32, 64 * U * mag)
    print(f"{name}: kernel {dev_k:.3e}  f32 restatement {dev_32:.3e}  magnitude {mag:.3e}  bound {bound:.3e}")
    assert dev_k <= bound, (name, dev_k, bound)


@functools.lru_cache(maxsize=None)
def _cloud(N, P):
    """(x f32, d64, d32) on the host, for N = 1000 on the device (torch's own kernels take seconds off a case); shared by
    the tests of a shape and never changed."""
    x = ref.cloud(N, P, 17 * N + P)
    if N >= 1000:
        x = x.cuda()
    return x, ref.sq_dists(x.double()), ref.sq_dists(x)


@functools.lru_cache(maxsize=None)
def _calibrated(N, P):
    """The f64 restatement's (beta, dmin, log_s0) of the shape's cloud at perplexity min(30, (N - 1) / 3) (1.5 for the
    three-point cloud, whose entropies end at log 2), rounded to f32:
    what the gradient walk is given, and what both restatements of the gradient are given."""
    x, d64, _ = _cloud(N, P)
    beta, dmin, log_s0, _, _ = ref.perplexity_bandwidths(x, min(30.0, max(1.5, (N - 1) / 3.0)), d=d64)
    return beta.float(), dmin.float(), log_s0.float()


# ------------------------------------------------------------------------------------------------ 1: cond_entropy_sums
@pytest.mark.parametrize("N,P", SHAPES)
def test_cond_entropy_sums(dev, N, P):
    """dmin alone (the first pass), then s0 and s1 for B = 1, 3, 8 per-row candidates spanning 2^+-10 around 1 / mean(d -
    m), shifted by the kernel's own dmin; each candidate column compared on its own (their magnitudes run from N to 1);
    two runs bit-identical."""
    x, d64, d32 = _cloud(N, P)
    xd = x.to(dev)
    nqb, ks = ops.cond_entropy_sums_plan(N)
    assert nqb == (N + 63) // 64 and 1 <= ks <= (N + 63) // 64
    if N == 130:
        assert ks == 3, "130 rows no longer split the key range three ways"
    dmin, none0, none1 = ops.cond_entropy_sums(xd)
    assert none0 is None and none1 is None
    _close(f"dmin N={N} P={P}", dmin, ref.row_min(d64), ref.row_min(d32))
    assert torch.equal(ops.cond_entropy_sums(xd)[0], dmin)
    shift = dmin.to(x.device)
    base = (1.0 / ref.mean_spread(x, shift)).float()
    for B in (1, 3, 8):
        octaves = torch.linspace(-10.0, 10.0, B) if B > 1 else torch.zeros(1)
        betas = (base[:, None] * torch.exp2(octaves).to(x.device)[None, :]).contiguous()
        bd = betas.to(dev)
        dm, s0, s1 = ops.cond_entropy_sums(xd, bd, shift=dmin, want_min=True)
        assert torch.equal(dm, dmin)
        r64, r32 = ref.entropy_sums(d64, betas.double(), shift.double()), ref.entropy_sums(d32, betas, shift)
        for b in range(B):
            tag = f"N={N} P={P} B={B} b={b}"
            _close(f"s0 {tag}", s0[:, b], r64[0][:, b], r32[0][:, b])
            _close(f"s1 {tag}", s1[:, b], r64[1][:, b], r32[1][:, b])
        again = ops.cond_entropy_sums(xd, bd, shift=dmin)
        assert again[0] is None and torch.equal(again[1], s0) and torch.equal(again[2], s1)
        only0 = ops.cond_entropy_sums(xd, bd, shift=dmin, want_s1=False)
        assert only0[2] is None and torch.equal(only0[1], s0)


def test_cond_entropy_diagonal_is_dropped_not_subtracted(dev):
    """Rows of norm 30, as in test_gpu_mmd.test_diagonal_is_dropped_not_subtracted: the computed d_ii is rounding noise of
    the size of an ulp of 1800, not 0.  beta = 1 / 1800: the sum with the diagonal minus the sum without it is the
    diagonal's term, 1 to within 4 ulp of s0.  beta = 1: every off-diagonal term is exp(-~1800) = 0, so the sums without
    the diagonal are exactly 0; and the minimum without it is a distance between two points, not the noise."""
    M, P = 200, 64
    g = torch.Generator().manual_seed(2)
    x = torch.nn.functional.normalize(torch.randn(M, P, generator=g, dtype=F64), dim=1).mul(30.0).float().to(dev)
    beta = torch.full((M, 1), 1.0 / 1800.0, dtype=F32, device=dev)
    mn_full, full, _ = ops.cond_entropy_sums(x, beta, diag_offset=-1, want_min=True)
    mn_skip, skip, _ = ops.cond_entropy_sums(x, beta, diag_offset=0, want_min=True)
    ulp = torch.exp2(torch.floor(torch.log2(full.double())) - 23)
    dev_ulp = ((full.double() - skip.double() - 1.0).abs() / ulp).max()
    print(f"diagonal rule: s0 in [{float(full.min()):.3f}, {float(full.max()):.3f}], (full - skipped - 1) up to "
          f"{float(dev_ulp):.3f} ulp of s0; dmin with the diagonal up to {float(mn_full.abs().max()):.3e}, without it from "
          f"{float(mn_skip.min()):.1f}")
    assert float(dev_ulp) <= 4.0
    assert float(mn_full.abs().max()) < 1.0 and float(mn_skip.min()) > 900.0
    one = torch.ones((M, 1), dtype=F32, device=dev)
    _, s0, s1 = ops.cond_entropy_sums(x, one, diag_offset=0)
    assert torch.equal(s0, torch.zeros_like(s0)) and torch.equal(s1, torch.zeros_like(s1))


# ------------------------------------------------------------------------------------------------ 2: perplexity_bandwidths
@pytest.mark.parametrize("N,P", [(63, 4), (65, 512), (130, 60), (1000, 60), (1000, 512)])
@pytest.mark.parametrize("perplexity", [5.0, 30.0])
def test_perplexity_bandwidths(dev, N, P, perplexity):
    x, d64, d32 = _cloud(N, P)
    b64, m64, l64, h64, _ = ref.perplexity_bandwidths(x, perplexity, d=d64)
    b32, m32, l32, h32, _ = ref.perplexity_bandwidths(x, perplexity, dtype=F32, d=d32)
    beta, dmin, log_s0, H = manifold.perplexity_bandwidths(x.to(dev), perplexity)
    tag = f"N={N} P={P} perplexity={perplexity}"
    assert all(t.shape == (N,) and t.dtype == F32 for t in (beta, dmin, log_s0, H))
    _close(f"log2 beta {tag}", torch.log2(beta.double()), torch.log2(b64), torch.log2(b32.double()))
    _close(f"entropy {tag}", H, h64, h32)
    _close(f"dmin {tag}", dmin, m64, m32)
    _close(f"log s0 {tag}", log_s0, l64, l32)


def test_perplexity_bandwidths_repeated_rows(dev):
    """40 rows are copies of one row, far from the rest, at perplexity 30: their entropy cannot fall below log 39.
    Everything stays finite and the copies' beta sits at the upper end of the first bracket; the other rows calibrate."""
    N, P = 200, 16
    x = ref.cloud(N, P, 7)
    x[:40] = x[0] + 10.0
    beta, dmin, log_s0, H = manifold.perplexity_bandwidths(x.to(dev), 30.0)
    assert all(bool(torch.isfinite(t).all()) for t in (beta, dmin, log_s0, H))
    top = -torch.log2(ref.mean_spread(x, dmin.cpu())) + 20.0
    got = torch.log2(beta.double().cpu())
    print(f"copies: log2 beta - bracket end in [{float((got - top)[:40].min()):.3e}, {float((got - top)[:40].max()):.3e}], "
          f"entropy from {float(H[:40].min()):.4f} (log 39 = {math.log(39):.4f}); others: |H - log 30| up to "
          f"{float((H[40:] - math.log(30.0)).abs().max()):.3e}")
    assert float((got - top)[:40].abs().max()) <= 40.0 / 9 ** 8 + 64 * U * 20.0     # the last bracket's width, f32 beta
    assert float(H[:40].min()) >= math.log(39.0) * (1 - 64 * U)
    _, _, _, h64, _ = ref.perplexity_bandwidths(x, 30.0)
    _, _, _, h32, _ = ref.perplexity_bandwidths(x, 30.0, dtype=F32)
    _close("entropy with repeated rows", H, h64, h32)


# ------------------------------------------------------------------------------------------------ 3: tsne_grad
def _device_gradient(rows, alpha):
    """The gradient as clipk_tsne_update assembles it: from update = 0, gains = 1.25 (x 0.8 = 1 exactly), momentum 0 and
    lr 1 the step leaves update = -grad.  Also (z, kl, gnorm) of the same launch."""
    N = rows.shape[0]
    y, update = torch.zeros((N, 2), device=rows.device), torch.zeros((N, 2), device=rows.device)
    gains = torch.full((N, 2), 1.25, device=rows.device)
    z, kl, gnorm = ops.tsne_update(rows, y, update, gains, alpha=alpha, momentum=0.0, lr=1.0, want_kl=True, want_gnorm=True)
    assert torch.equal(gains, torch.ones_like(gains)) and torch.equal(y, update)
    return -update, z, kl, gnorm


@pytest.mark.parametrize("N,P", SHAPES)
def test_tsne_grad(dev, N, P):
    x, d64, d32 = _cloud(N, P)
    beta, dmin, log_s0 = _calibrated(N, P)
    P64 = ref.joint(d64, beta.double(), dmin.double(), log_s0.double())
    P32 = ref.joint(d32, beta, dmin, log_s0)
    xd, bd, md, ld = (t.to(dev) for t in (x, beta, dmin, log_s0))
    nqb, ks = ops.tsne_grad_plan(N)
    assert nqb == (N + 63) // 64 and (ks == 3 if N == 130 else ks >= 1)
    g = torch.Generator().manual_seed(N + P)
    for scale in (1e-4, 1.0, 10.0):
        y = (scale * torch.randn(N, 2, generator=g, dtype=F64)).float().to(x.device)
        yd = y.to(dev)
        r64, r32 = ref.grad_rows(P64, y.double()), ref.grad_rows(P32, y)
        rows = ops.tsne_grad(xd, yd, bd, md, ld, want_kl=True)
        tag = f"N={N} P={P} |Y|~{scale:g}"
        for c, name in enumerate(("attr0", "attr1", "rep0", "rep1", "zrow", "klrow")):
            _close(f"{name} {tag}", rows[:, c], r64[:, c], r32[:, c])
        rows5 = ops.tsne_grad(xd, yd, bd, md, ld)
        assert rows5.shape == (N, 5) and torch.equal(rows5, rows[:, :5]), tag        # klrow left out: the rest bit for bit
        assert torch.equal(ops.tsne_grad(xd, yd, bd, md, ld, want_kl=True), rows), tag
        for alpha in (1.0, 12.0):
            grad, z, kl, gnorm = _device_gradient(rows, alpha)
            g64, z64 = ref.gradient(r64, alpha)
            g32, z32 = ref.gradient(r32, alpha)
            _close(f"gradient alpha={alpha:g} {tag}", grad, g64, g32)
            _close(f"|gradient| alpha={alpha:g} {tag}", gnorm, g64.norm(), g32.norm())
            _close(f"Z {tag}", z, z64, z32)
            _close(f"KL {tag}", kl, ref.kl_value(r64), ref.kl_value(r32))
            z5, none_kl, none_g = ops.tsne_update(rows5)                              # the reductions alone
            assert none_kl is None and none_g is None and torch.equal(z5, z)


# ------------------------------------------------------------------------------------------------ 4: single steps
@functools.lru_cache(maxsize=None)
def _problem():
    """The 200-point problem of tests 4 to 6: blobs, the f64 affinities, and the f64 run from init 0 with its states."""
    N, P = 200, 16
    x, labels = ref.blobs(N, P, 5)
    d64 = ref.sq_dists(x.double())
    beta, dmin, log_s0, _, _ = ref.perplexity_bandwidths(x, 30.0, d=d64)
    P64 = ref.joint(d64, beta, dmin, log_s0)
    inits = [1e-4 * torch.randn(N, 2, generator=torch.Generator().manual_seed(s), dtype=F64) for s in range(6)]
    return x, labels, d64, (beta, dmin, log_s0), P64, inits


STATES = (0, 5, 20, 100, 249, 250, 260)


def test_single_steps(dev):
    """One device step from the f64 run's state (Y, update, gains), rounded to f32, before iterations 0, 5, 20, 100, 249,
    250 and 260 - both sides of the exaggeration switch - against the restatement's step from the same state."""
    x, _, d64, (beta, dmin, log_s0), P64, inits = _problem()
    N = x.shape[0]
    lr = ref.auto_learning_rate(N)
    _, states = ref.descend(P64, inits[0], max(STATES) + 1, snapshots=STATES)
    b32, m32, l32 = beta.float(), dmin.float(), log_s0.float()
    Pa = ref.joint(d64, b32.double(), m32.double(), l32.double())                     # of the parameters the device gets
    Pb = ref.joint(ref.sq_dists(x), b32, m32, l32)
    xd, bd, md, ld = (t.to(dev) for t in (x, b32, m32, l32))
    for it in STATES:
        y, update, gains = (t.float() for t in states[it])
        early = it < 250
        alpha, momentum = (12.0, 0.5) if early else (1.0, 0.8)
        want = []
        for Pm, dt in ((Pa, F64), (Pb, F32)):
            grad, _ = ref.gradient(ref.grad_rows(Pm, y.to(dt)), alpha)
            want.append(ref.update_step(grad, y.to(dt), update.to(dt), gains.to(dt), momentum, lr))
        yd, ud, gd = y.to(dev), update.to(dev), gains.to(dev)
        rows = ops.tsne_grad(xd, yd, bd, md, ld)
        ops.tsne_update(rows, yd, ud, gd, alpha=alpha, momentum=momentum, lr=lr)
        for name, got, k in (("Y", yd, 0), ("update", ud, 1), ("gains", gd, 2)):
            _close(f"step {it}: {name}", got, want[0][k], want[1][k])


# ------------------------------------------------------------------------------------------------ 5: end to end
def test_end_to_end(dev):
    """Four blobs, 300 iterations from a given init.  The returned KL is the KL of the returned map; the map is as good as
    the f64 restatement's from six inits: KL at most 1.25 x their largest, 10-NN label purity at least their smallest
    minus 0.03; and its neighbourhoods are the cloud's, unlike those of a random permutation of it."""
    x, labels, d64, _, P64, inits = _problem()
    N = x.shape[0]
    kls, purities = [], []
    P64d = P64.to(dev)                              # the six f64 runs on the device: 1800 steps of small torch kernels
    for y0 in inits:
        y, _ = ref.descend(P64d, y0.to(dev), 300)
        kls.append(float(ref.kl_value(ref.grad_rows(P64d, y))))
        purities.append(ref.knn_purity(y.cpu(), labels))
    start = float(ref.kl_value(ref.grad_rows(P64, inits[0])))
    print(f"f64 restatement from six inits: KL {min(kls):.4f} .. {max(kls):.4f} (from {start:.4f}), purity "
          f"{min(purities):.4f} .. {max(purities):.4f}")
    xd = x.to(dev)
    res = manifold.tsne(xd, perplexity=30.0, n_iter=300, init=inits[0].float().to(dev))
    assert res.n_iter == 300 and res.learning_rate == 50.0 and res.embedding.shape == (N, 2)
    assert res.kl_divergence.dim() == 0 and res.beta.shape == (N,) and res.entropy.shape == (N,)
    y = res.embedding.cpu()
    b32, m32, l32, _, _ = ref.perplexity_bandwidths(x, 30.0, dtype=F32)
    P32 = ref.joint(ref.sq_dists(x), b32, m32, l32)
    kl64 = ref.kl_value(ref.grad_rows(P64, y.double()))
    _close("KL of the returned map", res.kl_divergence, kl64, ref.kl_value(ref.grad_rows(P32, y)))
    purity = ref.knn_purity(y, labels)
    print(f"device map: KL {float(kl64):.4f}, purity {purity:.4f}")
    assert float(kl64) <= 1.25 * max(kls) and purity >= min(purities) - 0.03
    keep = manifold.knn_preservation(xd, res.embedding, k=10)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(1))
    noise = manifold.knn_preservation(xd, res.embedding[perm.to(dev)].contiguous(), k=10)
    want = ref.knn_preservation(x, y, 10)
    print(f"10-NN preservation {float(keep):.4f} (restated {want:.4f}), of a random permutation {float(noise):.4f}")
    assert float(keep) > float(noise) and abs(float(keep) - want) <= 0.01
    spaces = manifold.embed_spaces({"protein_emb": xd, "gene_emb": xd}, n_iter=2, init="random",
                                   generator=torch.Generator().manual_seed(0))
    assert list(spaces) == ["protein_emb"] and bool(torch.isfinite(spaces["protein_emb"].embedding).all())


# ------------------------------------------------------------------------------------------------ 6: graph capture
def test_tsne_graph_capture(dev):
    x, _, _, _, _, inits = _problem()
    xd, y0 = x.to(dev), inits[1].float().to(dev)
    eager = manifold.tsne(xd, n_iter=20, init=y0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        manifold.tsne(xd, n_iter=20, init=y0)
    torch.cuda.current_stream().wait_stream(side)
    graph, keep = torch.cuda.CUDAGraph(), []
    with ops.owned_by_capture(keep), torch.cuda.graph(graph):                         # one stream, no parallel branches
        out = manifold.tsne(xd, n_iter=20, init=y0)
    for _ in range(2):
        out.embedding.fill_(-1.0)
        out.kl_divergence.fill_(-1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.embedding, eager.embedding) and torch.equal(out.kl_divergence, eager.kl_divergence)
        assert torch.equal(out.beta, eager.beta) and torch.equal(out.entropy, eager.entropy)
