"""CPU: clip_dplm_amd.diffusion without a device - every argument error before any device work, the torch glue
(connectivities, the fixed-size symmetrisation, pseudotime, Spearman) on host graphs against the loops of
tests/diffusion_ref.py, the dense-reference identities of T = S W S, and the solver's torch logic run through a torch
restatement of ops.csr_spmm."""
import math

import numpy as np
import pytest
import torch

import diffusion_ref as ref

F64 = torch.float64


def _host_graph(x, k):
    from clip_dplm_amd.neighbors import KNNGraph
    idx, d2 = ref.knn_host(x, k)
    return KNNGraph(torch.from_numpy(idx), torch.from_numpy(d2))


@pytest.fixture(scope="module")
def branch300():
    """(cloud, parameter, host KNNGraph, SymGraph, dense W, dense T, s, eigenvalues, eigenvectors) of the N = 300 cloud."""
    from clip_dplm_amd import diffusion
    x, t, _ = ref.branch_cloud(300, 4, 1)
    g = _host_graph(x, 14)
    sg = diffusion.connectivities(g)
    W = sg.to_dense().numpy()
    T, s = ref.transition_ref(W)
    lam, vec = ref.eigh_desc(T)
    return x, t, g, sg, W, T, s, lam, vec


# ------------------------------------------------------------------------------------------------ argument errors
def test_every_argument_error_before_any_device_work(monkeypatch):
    import clip_dplm_amd
    from clip_dplm_amd import diffusion, ops
    from clip_dplm_amd.neighbors import KNNGraph

    def boom():
        raise AssertionError("the device library was touched")
    monkeypatch.setattr(ops, "_lib", boom)
    assert clip_dplm_amd.diffusion_map is diffusion.diffusion_map and clip_dplm_amd.diffusion is diffusion
    assert clip_dplm_amd.SymGraph is diffusion.SymGraph and clip_dplm_amd.pseudotime is diffusion.pseudotime
    x = torch.zeros(100, 8)
    g = KNNGraph(torch.zeros(100, 14, dtype=torch.int64), torch.zeros(100, 14))
    sg = diffusion.SymGraph(torch.zeros(101, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=F64))
    bad = [
        (dict(x_or_graph=[[0.0] * 8] * 100), "tensor"), (dict(x_or_graph=x.double()), "float32"),
        (dict(x_or_graph=torch.zeros(100)), "2-D"), (dict(x_or_graph=torch.zeros(100, 6)), "multiple of 4"),
        (dict(x_or_graph=x, metric="sqeuclidean"), "metric"),
        (dict(x_or_graph=x, n_neighbors=1), "n_neighbors"), (dict(x_or_graph=x, n_neighbors=101), "n_neighbors"),
        (dict(x_or_graph=x, n_neighbors=15.0), "n_neighbors"), (dict(x_or_graph=torch.zeros(2000, 4), n_neighbors=1026), "n_neighbors"),
        (dict(x_or_graph=x, n_comps=0), "n_comps"), (dict(x_or_graph=x, n_comps=33), "n_comps"), (dict(x_or_graph=x, n_comps=True), "n_comps"),
        (dict(x_or_graph=torch.zeros(20, 4), n_neighbors=5, n_comps=21), "n_comps"),
        (dict(x_or_graph=x, tol=0.0), "tol"), (dict(x_or_graph=x, tol="1e-9"), "tol"),
        (dict(x_or_graph=x, max_outer=0), "max_outer"), (dict(x_or_graph=x, max_outer=2.5), "max_outer"),
        (dict(x_or_graph=x, generator=0), "generator"),
        (dict(x_or_graph=KNNGraph(torch.zeros(10, 12, dtype=torch.int64), torch.zeros(10, 12))), "against itself"),
        (dict(x_or_graph=KNNGraph(torch.zeros(10, 3, dtype=torch.int32), torch.zeros(10, 3))), "int64"),
        (dict(x_or_graph=diffusion.SymGraph(sg.indptr.int(), sg.indices, sg.weights)), "SymGraph"),
        (dict(x_or_graph=diffusion.SymGraph(sg.indptr, sg.indices, torch.zeros(3, dtype=F64))), "SymGraph"),
        (dict(x_or_graph=x), "device"), (dict(x_or_graph=g), "device"), (dict(x_or_graph=sg), "device"),   # no CPU fallback
    ]
    for kw, word in bad:
        with pytest.raises((ValueError, TypeError), match=word):
            diffusion.diffusion_map(**kw)
    for graph, word in ((x, "KNNGraph"), (KNNGraph(torch.zeros(5, 5, dtype=torch.int64), torch.zeros(5, 5)), "against itself"),
                        (KNNGraph(torch.zeros(5, 2, dtype=torch.int64), torch.zeros(5, 3)), "int64 indices")):
        with pytest.raises(ValueError, match=word):
            diffusion.connectivities(graph)
    dm = diffusion.DiffusionMap(torch.ones(3, dtype=F64), torch.zeros(10, 3, dtype=F64), torch.zeros(3, dtype=F64), 1, 1, True, 1, sg)
    for kw, word in ((dict(dm=dm, roots=[]), "roots"), (dict(dm=dm, roots=[10]), "roots must lie"), (dict(dm=dm, roots=-1), "roots must lie"),
                     (dict(dm=dm, roots=[0.5]), "roots"), (dict(dm=dm, roots=torch.zeros(2)), "roots"), (dict(dm=dm, roots=True), "roots"),
                     (dict(dm=dm, roots=torch.tensor([0, 11])), "roots must lie"),
                     (dict(dm=dm, roots=0, n_dcs=0), "n_dcs"), (dict(dm=dm, roots=0, n_dcs=2.0), "n_dcs"), (dict(dm="dm", roots=0), "DiffusionMap")):
        with pytest.raises(ValueError, match=word):
            diffusion.pseudotime(**kw)
    with pytest.raises(ValueError, match="root must"):
        diffusion.dpt(dm, [0])
    with pytest.raises(ValueError, match="device"):
        diffusion.pseudotime_preservation(x, x, 0)


def test_ops_argument_errors(monkeypatch):
    from clip_dplm_amd import _ffi, ops

    def boom():
        raise AssertionError("the device library was touched")
    monkeypatch.setattr(ops, "_lib", boom)
    ip, ix, w = torch.zeros(11, dtype=torch.int64), torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=F64)
    x = torch.zeros(10, 4, dtype=F64)
    good = dict(indptr=ip, indices=ix, w=w, x=x)
    bad = [
        (dict(indptr=ip.int()), "indptr"), (dict(indptr=ip[:10]), "indptr must have shape"), (dict(indices=ix.long()), "indices"),
        (dict(w=w.float()), "w must"), (dict(w=w[:4]), "one length"), (dict(x=x.float()), "x must"),
        (dict(x=torch.zeros(10, 65, dtype=F64)), "1 <= m <= 64"), (dict(x=torch.zeros(10, dtype=F64), indptr=ip), "x must be"),
        (dict(x=x.T.contiguous().T), "contiguous"), (dict(s=torch.zeros(9, dtype=F64)), "s must"), (dict(s=torch.zeros(10)), "s must"),
        (dict(b=torch.zeros(10, 3, dtype=F64)), "b must"), (dict(c=x.float()), "c must"), (dict(out=torch.zeros(9, 4, dtype=F64)), "out must"),
        (dict(out=x), "never x"),
    ]
    for kw, word in bad:
        with pytest.raises(ValueError, match=word):
            ops.csr_spmm(**{**good, **kw})
    with pytest.raises(_ffi.ClipkError, match="device"):                  # host tensors: there is no CPU fallback
        ops.csr_spmm(**good)


def test_c_entry_point_refuses_before_any_launch():
    """Null pointers, bad sizes, a short workspace and Y overlapping X return a status without touching a device."""
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    buf = np.zeros(4096, np.float64)
    p = buf.ctypes.data
    ok = [p, p, p, None, 10, 20, 4, p, 1.0, None, 0.0, None, 0.0, p + 8 * 1024, None, 0, None]

    def call(**kw):
        names = ["indptr", "indices", "w", "s", "N", "nnz", "m", "X", "alpha", "B", "beta", "C", "gamma", "Y", "ws", "wsb", "stream"]
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.clipk_csr_spmm_f64(*a)
    assert call(indptr=None) == -1 and call(X=None) == -1 and call(Y=None) == -1 and call(indices=None) == -1 and call(w=None) == -1
    assert call(N=0) == -1 and call(nnz=-1) == -1 and call(m=0) == -1
    assert call(m=65) == -2
    assert call(Y=p) == -1                                               # Y is X
    assert call(Y=p + 8 * 39) == -1 and call(Y=p - 8 * 39) == -1         # Y overlaps X's last / first element (N m = 40)
    chunk = ref.SPMM_CHUNK
    assert call(nnz=chunk + 1, ws=None) == -1 and call(nnz=chunk + 1, ws=p, wsb=8 * 4 * 2 - 1) == -1   # two slots of m doubles
    assert lib.clipk_csr_spmm_workspace(chunk, 4) == 0 and lib.clipk_csr_spmm_workspace(chunk + 1, 4) == 2 * 4 * 8
    assert lib.clipk_csr_spmm_workspace(2 ** 33, 64) == 2 ** 33 // chunk * 64 * 8 and lib.clipk_csr_spmm_workspace(10, 65) == 0


# ------------------------------------------------------------------------------------------------ the restatements themselves
def test_spmm_restatements_agree_with_a_dense_product():
    rng = np.random.default_rng(3)
    N, m = 40, 5
    lens = rng.integers(0, 7, N)
    lens[7] = 9 * ref.SPMM_CHUNK + 24                                      # ten chunks
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = rng.integers(0, N, indptr[-1]).astype(np.int32)
    w, s = rng.standard_normal(indptr[-1]), rng.uniform(0.5, 2.0, N)
    X, B, C = rng.standard_normal((3, N, m))
    dense = np.zeros((N, N))
    np.add.at(dense, (np.repeat(np.arange(N), lens), indices), w)
    want = 0.7 * (s[:, None] * dense * s[None, :]) @ X - 0.3 * B + 2.0 * C
    got = ref.csr_spmm_ref(indptr, indices, w, X, s, 0.7, B, -0.3, C, 2.0)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    t = ref.csr_spmm_torch(*(torch.from_numpy(a) for a in (indptr, indices, w, X)), s=torch.from_numpy(s), alpha=0.7,
                           b=torch.from_numpy(B), beta=-0.3, c=torch.from_numpy(C), gamma=2.0)
    assert np.abs(t.numpy() - want).max() <= 1e-12 * np.abs(want).max()
    # the chunk order is visible: one sum over the hub row's entries differs from the chunked one in the last bits
    assert np.abs(ref.csr_spmm_ref(indptr, indices, w, X) - dense @ X).max() <= 1e-12 * np.abs(dense @ X).max()


# ------------------------------------------------------------------------------------------------ connectivities on host graphs
@pytest.mark.parametrize("case", ["branch_k14", "k1", "duplicates"])
def test_connectivities_on_host_graphs(case):
    from clip_dplm_amd import diffusion
    if case == "branch_k14":
        x, k = ref.branch_cloud(300, 4, 1)[0], 14
    elif case == "k1":
        x, k = ref.branch_cloud(50, 4, 5)[0], 1
    else:
        x, k = ref.branch_cloud(120, 4, 7)[0], 6
        x[40:60] = x[0:20]                                                 # distance-0 neighbours: rho from the first positive one
        x[60:64] = x[0]                                                    # five equal rows
    g = _host_graph(x, k)
    d = g.distances.double()
    rho, sigma = diffusion._smooth_knn(d)
    a_ref, rho_ref, sigma_ref = ref.membership_ref(d.numpy())
    assert np.array_equal(rho.numpy(), rho_ref)
    assert np.array_equal(sigma.numpy(), sigma_ref)                        # the same bisection path, step for step
    if case == "duplicates":
        assert (d[:20, 0] == 0).all() and (rho[:20] > 0).all() and (a_ref[:20, 0] == 1).all()
    sg = diffusion.connectivities(g)
    indptr, cols, wts, _ = ref.connectivities_ref(g.indices.numpy(), d.numpy())
    N = x.shape[0]
    assert sg.n == N and sg.nnz == 2 * N * k and sg.indices.dtype == torch.int32
    assert np.array_equal(sg.indptr.numpy(), indptr) and np.array_equal(sg.indices.numpy(), cols)
    # the glue's exp against libm's: both within an ulp of exp, a and b each off by <= 2 eps relative; fl(a + b) and
    # fl(a b) add half an eps each and w >= (a + b) / 2 >= a b: |dw| <= (2 w + w) 2.5 eps + eps w / 2 = 8 eps w
    assert (np.abs(sg.weights.numpy() - wts) <= 8 * ref.EPS * wts + 8 * 2.0 ** -1074).all()
    W = sg.to_dense()
    assert torch.equal(W, W.T)
    assert np.array_equal(sg.row_sums().numpy() > 0, np.ones(N, bool))
    assert np.abs(sg.row_sums().numpy() - W.numpy().sum(1)).max() <= 1e-13 * k
    assert sg.max_row_length == int(np.diff(indptr).max())
    rows = sg.rows().numpy()
    key = rows * N + sg.indices.numpy()
    assert (np.diff(key) >= 0).all()                                       # rows ascending, columns ascending inside a row
    dup = np.diff(key) == 0
    assert (sg.weights.numpy()[1:][dup] == 0).all() and dup.sum() > 0      # the second of a mutual pair carries 0


def test_symmetrisation_of_a_handmade_graph():
    """Three points: 0 <-> 1 mutual, 2 -> 0 one-sided.  Fixed nnz = 2 N k = 6."""
    from clip_dplm_amd import diffusion
    from clip_dplm_amd.neighbors import KNNGraph
    g = KNNGraph(torch.tensor([[1], [0], [0]]), torch.tensor([[1.0], [1.0], [4.0]]))
    sg = diffusion.connectivities(g)                                       # k = 1: every a = 1
    assert sg.indptr.tolist() == [0, 3, 5, 6] and sg.indices.tolist() == [1, 1, 2, 0, 0, 0]
    assert sg.weights.tolist() == [1.0, 0.0, 1.0, 1.0, 0.0, 1.0]
    assert sg.to_dense().tolist() == [[0, 1, 1], [1, 0, 0], [1, 0, 0]]


# ------------------------------------------------------------------------------------------------ dense-reference identities
def test_transition_matrix_identities(branch300):
    _, _, _, _, W, T, s, lam, vec = branch300
    assert np.array_equal(W, W.T)
    assert np.abs(T - T.T).max() <= 4 * ref.EPS * np.abs(T).max()
    assert np.abs(T - s[:, None] * W * s[None, :]).max() <= 8 * ref.EPS * np.abs(T).max()
    assert abs(lam[0] - 1) <= 1e-13 and lam[-1] >= -1 - 1e-13 and lam[1] < 1 - 1e-8
    # the stationary vector: T z = S W S z = S W (1 / q) = S q z^2 = z with z = sqrt(K 1) = 1 / (s q)  (not 1 / s: T (1 / s) =
    # S q = 1 / z)
    top = 1 / (s * W.sum(1))
    top /= np.linalg.norm(top)
    assert 1 - abs(top @ vec[:, 0]) <= 1e-13
    assert np.abs(T @ top - top).max() <= 1e-14


def test_transition_scaling_through_the_restated_operator(branch300, monkeypatch):
    from clip_dplm_amd import diffusion, ops
    monkeypatch.setattr(ops, "csr_spmm", ref.csr_spmm_torch)
    sg, s = branch300[3], branch300[6]
    assert np.abs(diffusion.transition_scaling(sg).numpy() - s).max() <= 1e-14 * s.max()


# ------------------------------------------------------------------------------------------------ the solver's torch logic
@pytest.mark.parametrize("n_comps", [1, 5, 15])
def test_solver_logic_on_the_host(branch300, monkeypatch, n_comps):
    from clip_dplm_amd import diffusion, ops
    calls = []

    def spy(*a, **kw):
        calls.append(kw.get("out") is not None and kw["out"] is kw.get("c"))
        assert kw.get("out") is None or kw["out"] is not a[3]            # never written over the block that is gathered
        return ref.csr_spmm_torch(*a, **kw)
    monkeypatch.setattr(ops, "csr_spmm", spy)
    _, _, _, sg, _, T, s, lam, vec = branch300
    tol = 1e-9
    theta, v, res, n_outer, n_spmm, converged = diffusion._solve(sg, torch.from_numpy(s), n_comps, tol, 50,
                                                                 torch.Generator().manual_seed(5))
    assert converged and n_spmm == len(calls) == 1 + (n_outer - 1) * diffusion.CHEB_DEGREE and 2 <= n_outer <= 12
    assert sum(calls) == (n_outer - 1) * (diffusion.CHEB_DEGREE - 1)      # every recurrence step writes over the block two back
    assert v.shape == (300, n_comps) and diffusion.block_size(n_comps, 300) == min(64, max(2 * n_comps, n_comps + 8))
    th, vn = theta.numpy(), v.numpy()
    assert (np.diff(th) <= 0).all() and np.abs(th - lam[:n_comps]).max() <= tol
    assert np.linalg.norm(T @ vn - vn * th, axis=0).max() <= tol + 1e-12 and res.max() <= tol
    assert np.abs(vn.T @ vn - np.eye(n_comps)).max() <= 1e-12
    signed = diffusion._fix_signs(v).numpy()
    top = np.abs(signed).argmax(0)
    assert (signed[top, np.arange(n_comps)] > 0).all() and np.array_equal(np.abs(signed), np.abs(vn))
    # one outer iteration is not enough and says so
    *_, n_outer1, _, converged1 = diffusion._solve(sg, torch.from_numpy(s), n_comps, tol, 1, torch.Generator().manual_seed(5))
    assert n_outer1 == 1 and not converged1


def test_sign_rule_takes_the_lowest_index_on_ties():
    from clip_dplm_amd import diffusion
    v = torch.tensor([[0.5, -0.5, 0.0], [-0.5, 0.5, 0.0], [0.5, 0.5, -1.0], [-0.5, -0.5, 0.0]], dtype=F64)
    got = diffusion._fix_signs(v)
    assert got[:, 0].tolist() == [0.5, -0.5, 0.5, -0.5] and got[:, 1].tolist() == [0.5, -0.5, -0.5, 0.5]
    assert got[:, 2].tolist() == [0.0, 0.0, 1.0, 0.0]


# ------------------------------------------------------------------------------------------------ pseudotime
@pytest.mark.parametrize("n_dcs", [3, 10, 15, 40])
def test_pseudotime_on_host_eigenpairs(branch300, n_dcs):
    from clip_dplm_amd import diffusion
    x, t, _, sg, _, _, _, lam, vec = branch300
    lam15, vec15 = lam[:15].copy(), vec[:, :15].copy()
    lam15[1] = 1.0                                                         # a second component's stationary vector is left out too
    dm = diffusion.DiffusionMap(torch.from_numpy(lam15), torch.from_numpy(vec15), torch.zeros(15, dtype=F64), 1, 1, True, 2, sg)
    roots = [int(np.argmin(t)), 0, 299]
    want = ref.pseudotime_ref(lam15, vec15, roots, n_dcs)
    got = diffusion.pseudotime(dm, roots, n_dcs)
    assert got.dtype == F64 and got.shape == (3, 300)
    assert np.abs(got.numpy() - want).max() <= 1e-12
    assert (got.max(1).values == 1).all() and all(got[r, roots[r]] == 0 for r in range(3))
    for r, root in enumerate(roots):                                       # multi-root rows are the single-root calls
        assert torch.equal(diffusion.dpt(dm, root, n_dcs), got[r])
    assert torch.equal(diffusion.pseudotime(dm, torch.tensor(roots), n_dcs), got)
    assert torch.isnan(diffusion.pseudotime(dm, roots, 2)).all()          # no component counts: 0 / 0


def test_reference_pseudotime_follows_the_branch_parameter(branch300):
    _, t, _, _, _, _, _, lam, vec = branch300
    root = int(np.argmin(t))
    for n_dcs in (10, 15):
        assert ref.spearman_ref(ref.pseudotime_ref(lam[:15], vec[:, :15], [root], n_dcs)[0], t) > 0.95


def test_spearman_with_ties():
    from clip_dplm_amd import diffusion
    rng = np.random.default_rng(11)
    a = rng.integers(0, 6, (3, 40)).astype(np.float64)                     # many ties
    b = a + rng.standard_normal((3, 40))
    got = diffusion.spearman(torch.from_numpy(a), torch.from_numpy(b))
    for r in range(3):
        assert abs(float(got[r]) - ref.spearman_ref(a[r], b[r])) <= 1e-13
    from scipy import stats
    assert abs(ref.spearman_ref(a[0], b[0]) - stats.spearmanr(a[0], b[0])[0]) <= 1e-12
