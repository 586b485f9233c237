"""CPU: the restatement of tests/tsne_ref.py against literal loops and against the private functions of the library the
reference calls, the host side of clip_dplm_amd.manifold (every argument error of tsne, the learning-rate rule) and the
C ABI of the t-SNE entries as far as it goes without a device."""
import math

import numpy as np
import pytest
import torch

import tsne_ref as ref

F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------------ the restatement itself
def _loops(x, y, beta, alpha):
    """Everything by double loops over the definitions: (dmin, s0, s1, P, rows, grad, Z, KL)."""
    N = len(x)
    d = [[sum((float(x[i, p]) - float(x[j, p])) ** 2 for p in range(x.shape[1])) for j in range(N)] for i in range(N)]
    dmin = [min(d[i][j] for j in range(N) if j != i) for i in range(N)]
    s0 = [sum(math.exp(-beta[i] * (d[i][j] - dmin[i])) for j in range(N) if j != i) for i in range(N)]
    s1 = [sum((d[i][j] - dmin[i]) * math.exp(-beta[i] * (d[i][j] - dmin[i])) for j in range(N) if j != i) for i in range(N)]
    cond = [[0.0 if i == j else math.exp(-beta[i] * (d[i][j] - dmin[i])) / s0[i] for j in range(N)] for i in range(N)]
    P = [[(cond[i][j] + cond[j][i]) / (2 * N) for j in range(N)] for i in range(N)]
    rows = [[0.0] * 6 for _ in range(N)]
    for i in range(N):
        for j in range(N):
            if i == j:
                continue
            dy = [float(y[i, c]) - float(y[j, c]) for c in range(2)]
            w = 1.0 / (1.0 + dy[0] ** 2 + dy[1] ** 2)
            for c in range(2):
                rows[i][c] += P[i][j] * w * dy[c]
                rows[i][2 + c] += w * w * dy[c]
            rows[i][4] += w
            if P[i][j] > 0:
                rows[i][5] += P[i][j] * (math.log(P[i][j]) - math.log(w))
    Z = sum(r[4] for r in rows)
    grad = [[4 * (alpha * r[c] - r[2 + c] / Z) for c in range(2)] for r in rows]
    KL = sum(r[5] for r in rows) + math.log(Z)
    return dmin, s0, s1, P, rows, grad, Z, KL


@pytest.mark.parametrize("N,alpha", [(3, 1.0), (9, 12.0)])
def test_restatement_against_double_loops(N, alpha):
    g = torch.Generator().manual_seed(N)
    x, y = torch.randn(N, 4, generator=g, dtype=F64), torch.randn(N, 2, generator=g, dtype=F64)
    beta = (0.3 + torch.rand(N, generator=g, dtype=F64)).tolist()
    dmin, s0, s1, P, rows, grad, Z, KL = _loops(x, y, beta, alpha)
    t = lambda v: torch.tensor(v, dtype=F64)
    d = ref.sq_dists(x)
    assert torch.allclose(ref.row_min(d), t(dmin), rtol=0, atol=1e-13)
    r0, r1 = ref.entropy_sums(d, t(beta)[:, None], t(dmin))
    assert torch.allclose(r0[:, 0], t(s0), rtol=1e-13, atol=0) and torch.allclose(r1[:, 0], t(s1), rtol=1e-12, atol=1e-14)
    Pr = ref.joint(d, t(beta), t(dmin), torch.log(t(s0)))
    assert torch.allclose(Pr, t(P), rtol=1e-12, atol=1e-16) and abs(float(Pr.sum()) - 1.0) < 1e-13
    rr = ref.grad_rows(Pr, y)
    assert torch.allclose(rr, t(rows), rtol=1e-11, atol=1e-14)
    gr, Zr = ref.gradient(rr, alpha)
    assert torch.allclose(gr, t(grad), rtol=1e-11, atol=1e-14) and abs(float(Zr) - Z) < 1e-12 * Z
    assert abs(float(ref.kl_value(rr)) - KL) < 1e-12
    # the f32 form (norm expansion) is the same quantity to f32 accuracy
    d32 = ref.sq_dists(x.float())
    P32 = ref.joint(d32, t(beta).float(), ref.row_min(d32), torch.log(ref.entropy_sums(d32, t(beta).float()[:, None],
                                                                                        ref.row_min(d32))[0][:, 0]))
    assert torch.allclose(P32.double(), t(P), rtol=0, atol=1e-5)
    assert torch.allclose(ref.grad_rows(P32, y.float()).double(), t(rows), rtol=0, atol=1e-4)


def test_restated_update_rule_against_loops():
    g = torch.Generator().manual_seed(3)
    grad, y, update = (torch.randn(7, 2, generator=g, dtype=F64) for _ in range(3))
    gains = torch.rand(7, 2, generator=g, dtype=F64) * 0.02          # some below the floor after x 0.8
    update[0, 0] = 0.0                                                # a zero product is not "< 0": the gain shrinks
    ny, nu, ng = ref.update_step(grad, y, update, gains, 0.5, 50.0)
    for i in range(7):
        for c in range(2):
            gn = float(gains[i, c]) + 0.2 if float(update[i, c]) * float(grad[i, c]) < 0 else float(gains[i, c]) * 0.8
            gn = max(gn, 0.01)
            u = 0.5 * float(update[i, c]) - 50.0 * gn * float(grad[i, c])
            assert abs(float(ng[i, c]) - gn) < 1e-15 and abs(float(nu[i, c]) - u) < 1e-12
            assert abs(float(ny[i, c]) - (float(y[i, c]) + u)) < 1e-12
    assert float(ng[0, 0]) == max(float(gains[0, 0]) * 0.8, 0.01)


@pytest.mark.parametrize("perplexity", [5.0, 30.0])
def test_search_reaches_the_target_entropy(perplexity):
    x = ref.cloud(200, 16, 7)
    beta, dmin, log_s0, H, (lo, hi) = ref.perplexity_bandwidths(x, perplexity)
    assert float((H - math.log(perplexity)).abs().max()) < 1e-5       # the tolerance of the reference's library
    assert float((hi - lo).max()) <= 40.0 / 9 ** 8 * (1 + 1e-9)
    P = ref.joint(ref.sq_dists(x.double()), beta, dmin, log_s0)
    assert abs(float(P.sum()) - 1.0) < 1e-12 and torch.equal(P, P.T)
    # a row whose nearest neighbour is repeated more often than the perplexity: finite, at the bracket's upper end
    xd = x.clone()
    xd[:40] = x[0] + 100.0                                            # far from every other row: only the copies see it
    beta, dmin, log_s0, H, (lo, hi) = ref.perplexity_bandwidths(xd, 30.0)
    centre = -torch.log2(ref.mean_spread(xd, dmin))
    assert all(bool(torch.isfinite(v).all()) for v in (beta, dmin, log_s0, H))
    assert float((hi[:40] - (centre[:40] + 20.0)).abs().max()) < 1e-9 and float(H[:40].min()) >= math.log(39.0) - 1e-9
    assert float((H[40:] - math.log(30.0)).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------ against the library
@pytest.mark.parametrize("N,P,perplexity,seed", [(60, 8, 5.0, 1), (150, 16, 30.0, 2), (200, 32, 30.0, 3)])
def test_restatement_against_sklearn(N, P, perplexity, seed):
    """Bounds: 1e-7 absolute on P, 1e-6 relative on KL, 1e-6 of the gradient's largest entry on the gradient - above the
    library's own deviations (its search stops at 1e-5 in H and it clamps P and Q at machine epsilon), far below any
    formula error."""
    pytest.importorskip("sklearn")
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne

    x = ref.cloud(N, P, seed)
    d = ref.sq_dists(x.double())
    beta, dmin, log_s0, _, _ = ref.perplexity_bandwidths(x, perplexity)
    Pm = ref.joint(d, beta, dmin, log_s0)
    p_sk = _t_sne._joint_probabilities(d.numpy().astype(np.float32), perplexity, 0)
    dev_p = float(np.abs(squareform(p_sk) - Pm.numpy()).max())
    g = torch.Generator().manual_seed(seed)
    for scale in (1e-4, 1.0, 10.0):
        y = scale * torch.randn(N, 2, generator=g, dtype=F64)
        kl_sk, grad_sk = _t_sne._kl_divergence(y.numpy().ravel(), squareform(Pm.numpy(), checks=False), 1, N, 2)
        rows = ref.grad_rows(Pm, y)
        grad, _ = ref.gradient(rows)
        kl = float(ref.kl_value(rows))
        dev_g = float(np.abs(grad_sk.reshape(N, 2) - grad.numpy()).max()) / float(grad.abs().max())
        print(f"N={N} scale={scale}: P {dev_p:.2e}  KL {abs(kl - kl_sk) / abs(kl_sk):.2e}  gradient {dev_g:.2e}")
        assert abs(kl - kl_sk) <= 1e-6 * abs(kl_sk) and dev_g <= 1e-6
    assert dev_p <= 1e-7


# ------------------------------------------------------------------------------------------------ manifold: host side
def test_learning_rate_rule():
    from clip_dplm_amd import manifold
    assert manifold.auto_learning_rate(200) == 50.0 == ref.auto_learning_rate(200)
    assert manifold.auto_learning_rate(2400) == 50.0 and manifold.auto_learning_rate(2401) > 50.0
    assert manifold.auto_learning_rate(65536) == 65536 / 12.0 / 4.0 == ref.auto_learning_rate(65536)
    assert manifold.auto_learning_rate(65536, 4.0) == 4096.0


def test_every_value_error_of_tsne():
    """Raised before the device is touched: the clouds below live on the host."""
    import clip_dplm_amd
    from clip_dplm_amd import manifold
    assert clip_dplm_amd.tsne is manifold.tsne and clip_dplm_amd.manifold is manifold
    x = torch.zeros(100, 8)
    bad = [
        (dict(x=x, perplexity=99.0), "perplexity"), (dict(x=x, perplexity=150.0), "perplexity"),
        (dict(x=x, perplexity=0.0), "perplexity"), (dict(x=x, perplexity=-3.0), "perplexity"),
        (dict(x=torch.zeros(2, 8), perplexity=0.5), "rows"),
        (dict(x=x.double()), "float32"), (dict(x=x.bfloat16()), "float32"),
        (dict(x=x), "device"),                                        # a host tensor: there is no CPU fallback
        (dict(x=torch.zeros(100, 6)), "multiple of 4"), (dict(x=torch.zeros(100, 516)), "at most 512"),
        (dict(x=torch.zeros(100)), "2-D"), (dict(x=[[0.0] * 8] * 100), "tensor"),
    ]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            manifold.tsne(**kw)
    for kw, word in bad[:8]:
        with pytest.raises(ValueError, match=word):
            manifold.perplexity_bandwidths(kw["x"], kw.get("perplexity", 30.0))
    with pytest.raises(ValueError, match="k must"):
        manifold.knn_preservation(x, torch.zeros(100, 2), k=64)
    assert manifold.embed_spaces({"gene_emb": x}) == {}              # absent spaces are skipped: nothing is launched


# ------------------------------------------------------------------------------------------------ the C entries
def test_entry_points_refuse_without_a_launch():
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    assert lib.clipk_version() == _ffi.ABI_VERSION == 7              # entry points were added, no signature changed
    for n, nargs in (("clipk_cond_entropy_sums", 14), ("clipk_cond_entropy_sums_workspace", 3), ("clipk_tsne_grad", 14),
                     ("clipk_tsne_grad_workspace", 3), ("clipk_tsne_update", 13)):
        assert n in _ffi.SIGNATURES and hasattr(lib, n) and len(_ffi.SIGNATURES[n][1]) == nargs

    def ces(N, P, B, diag=0):
        return lib.clipk_cond_entropy_sums(None, N, P, None, None, B, None, diag, None, None, None, None, 0, None)

    def grad(N, P, diag=0):
        return lib.clipk_tsne_grad(None, N, P, None, None, None, None, None, diag, 1, None, None, 0, None)

    for N, P, B in ((0, 8, 1), (-1, 8, 1), (100, 0, 1), (100, 8, -1)):
        assert ces(N, P, B) == -1 and lib.clipk_cond_entropy_sums_workspace(N, P, B) == 0
    for N, P, B in ((2, 8, 1), (100, 6, 1), (100, 516, 1), (100, 8, 9)):
        assert ces(N, P, B) == -2 and lib.clipk_cond_entropy_sums_workspace(N, P, B) == 0
    for N, P in ((0, 8), (100, 0)):
        assert grad(N, P) == -1 and lib.clipk_tsne_grad_workspace(N, P, 1) == 0
    for N, P in ((2, 8), (100, 6), (100, 516)):
        assert grad(N, P) == -2 and lib.clipk_tsne_grad_workspace(N, P, 1) == 0
    # a supported shape with null pointers or an offset below -1: a bad argument, not a launch
    assert ces(100, 8, 8) == -1 and ces(100, 8, 0) == -1 and ces(100, 8, 1, diag=-2) == -1
    assert grad(100, 8) == -1 and grad(100, 8, diag=-2) == -1
    upd = lambda N, nc: lib.clipk_tsne_update(None, N, nc, 1.0, 0.5, 50.0, None, None, None, None, None, None, None)
    assert upd(100, 6) == -1 and upd(100, 4) == -1 and upd(0, 6) == -1 and upd(2, 6) == -2
    # workspace: the split partials (130 rows split three ways: 3 key tiles), and the records of the gradient walk
    assert lib.clipk_cond_entropy_sums_workspace(130, 8, 0) == 3 * 130 * 4
    assert lib.clipk_cond_entropy_sums_workspace(130, 8, 8) == 3 * 130 * 17 * 4
    assert lib.clipk_tsne_grad_workspace(130, 8, 1) == (130 * 8 + 3 * 130 * 6) * 4
    assert lib.clipk_tsne_grad_workspace(130, 8, 0) == (130 * 8 + 3 * 130 * 5 + 2) * 4
