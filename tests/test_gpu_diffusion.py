"""GPU: the sparse operator (include/clipk.h: clipk_csr_spmm_f64) bit for bit against its numpy restatement, and the
diffusion map / pseudotime built on it (clip_dplm_amd/diffusion.py) against the dense f64 references of
tests/diffusion_ref.py: numpy.linalg.eigh of the dense T made from SymGraph.to_dense().

Where a bound is not an equality it is derived where it is used: from the roundings of the glue, from the residuals the
solver reports and the gaps of the reference spectrum (Davis-Kahan), and from the reference's own backward error."""
import math

import numpy as np
import pytest
import torch

import diffusion_ref as ref
from clip_dplm_amd import _ffi, diffusion, neighbors, ops

pytestmark = pytest.mark.gpu
F64 = torch.float64
CHUNK = ref.SPMM_CHUNK


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _same_bits(got, want):
    return torch.equal(_bits(got), torch.from_numpy(np.ascontiguousarray(want)).view(torch.int64))


# ------------------------------------------------------------------------------------------------ 1: SpMM, bit for bit
def _csr(N, rng, hub=None):
    """Rows of 0 .. 6 entries (empty rows and rows of one entry among them), repeated columns, a tenth of the weights
    exactly zero; N >= 3: one hub row longer than twice the chunk and one exactly one chunk long."""
    lens = rng.integers(0, 7, N)
    if N >= 3:
        lens[0], lens[1] = 0, 1
        lens[N // 2], lens[N - 1] = 2 * CHUNK + 37, CHUNK
    if hub is not None:
        lens[0] = hub
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(indptr[-1])
    indices = rng.integers(0, N, nnz).astype(np.int32)
    w = rng.standard_normal(nnz)
    w[rng.random(nnz) < 0.1] = 0.0
    return indptr, indices, w


SCALARS = [(1.0, 0.0, 0.0), (-0.75, 1.5, -2.0), (0.0, -0.3, 0.7), (2.0, 0.0, -1.0), (-1.25, 0.3, 0.0), (0.5, -1.0, 1.0),
           (3.0, 1.0, 1.0), (-1.0, -1.0, 0.0)]


def _spmm_cases(N, m, indptr, indices, w, rng, dev):
    s = rng.uniform(0.5, 2.0, N)
    X, B, C = rng.standard_normal((3, N, m))
    d = {k: torch.from_numpy(v).to(dev) for k, v in dict(indptr=indptr, indices=indices, w=w, s=s, X=X, B=B, C=C).items()}
    combo = 0
    for use_s in (False, True):
        for use_b in (False, True):
            for use_c in (False, True):
                alpha, beta, gamma = SCALARS[combo % len(SCALARS)]
                combo += 1
                want = ref.csr_spmm_ref(indptr, indices, w, X, s if use_s else None, alpha, B if use_b else None, beta,
                                        C if use_c else None, gamma)
                kw = dict(s=d["s"] if use_s else None, alpha=alpha, b=d["B"] if use_b else None, beta=beta,
                          c=d["C"] if use_c else None, gamma=gamma)
                got = ops.csr_spmm(d["indptr"], d["indices"], d["w"], d["X"], **kw)
                assert _same_bits(got, want), (N, m, use_s, use_b, use_c)
                if use_b:                                                  # Y is B
                    bb = d["B"].clone()
                    out = ops.csr_spmm(d["indptr"], d["indices"], d["w"], d["X"], **{**kw, "b": bb, "out": bb})
                    assert out is bb and _same_bits(bb, want), (N, m, use_s, use_c, "Y = B")
                if use_c and not use_b:                                    # Y is C
                    cc = d["C"].clone()
                    ops.csr_spmm(d["indptr"], d["indices"], d["w"], d["X"], **{**kw, "c": cc, "out": cc})
                    assert _same_bits(cc, want), (N, m, use_s, "Y = C")
                out = torch.full((N, m), math.nan, dtype=F64, device=dev)   # a given out that is neither
                ops.csr_spmm(d["indptr"], d["indices"], d["w"], d["X"], **{**kw, "out": out})
                assert _same_bits(out, want)


@pytest.mark.parametrize("m", [1, 3, 15, 32, 33, 64])
@pytest.mark.parametrize("N", [1, 63, 65, 1000])
def test_spmm_bit_for_bit(dev, N, m):
    rng = np.random.default_rng(1000 * N + m)
    if N == 1:                                                             # the one row: empty, one entry, at the chunk, a hub
        for hub in (0, 1, CHUNK, 2 * CHUNK + 37):
            _spmm_cases(N, m, *_csr(N, rng, hub), rng, dev)
    else:
        _spmm_cases(N, m, *_csr(N, rng), rng, dev)


def test_spmm_chunk_edges_and_alignment(dev):
    """Row lengths around every multiple of the chunk, starts that are and are not multiples of it, and operands whose
    8-byte (not 16-byte) alignment sends an even m down the one-column path: the same bits."""
    rng = np.random.default_rng(77)
    N, m = 40, 6
    lens = np.array([CHUNK - 1, CHUNK, CHUNK + 1, 0, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, 3, CHUNK, CHUNK, 3 * CHUNK, 5 * CHUNK + 9]
                    + [2] * 28)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = rng.integers(0, N, indptr[-1]).astype(np.int32)
    w, s = rng.standard_normal(indptr[-1]), rng.uniform(0.5, 2.0, N)
    X, B = rng.standard_normal((2, N, m))
    want = ref.csr_spmm_ref(indptr, indices, w, X, s, 1.5, B, -0.5)
    t = [torch.from_numpy(a).to(dev) for a in (indptr, indices, w)]
    sd = torch.from_numpy(s).to(dev)
    got = ops.csr_spmm(*t, torch.from_numpy(X).to(dev), s=sd, alpha=1.5, b=torch.from_numpy(B).to(dev), beta=-0.5)
    assert _same_bits(got, want)
    odd = torch.zeros(N * m + 1, dtype=F64, device=dev)[1:].view(N, m)      # 8 bytes past a 16-byte boundary
    assert odd.data_ptr() % 16 == 8
    odd.copy_(torch.from_numpy(X))
    got = ops.csr_spmm(*t, odd, s=sd, alpha=1.5, b=torch.from_numpy(B).to(dev), beta=-0.5)
    assert _same_bits(got, want)
    # a column outside [0, N) is skipped
    bad = indices.copy()
    bad[[5, CHUNK + 3, 700]] = [-1, N, 2 ** 31 - 1]
    got = ops.csr_spmm(t[0], torch.from_numpy(bad).to(dev), t[2], torch.from_numpy(X).to(dev), s=sd)
    assert _same_bits(got, ref.csr_spmm_ref(indptr, bad, w, X, s))


def test_spmm_refuses_y_aliasing_x(dev):
    ip = torch.tensor([0, 1, 2], device=dev)
    ix, w = torch.tensor([1, 0], dtype=torch.int32, device=dev), torch.ones(2, dtype=F64, device=dev)
    x = torch.ones(2, 4, dtype=F64, device=dev)
    with pytest.raises(ValueError, match="never x"):
        ops.csr_spmm(ip, ix, w, x, out=x)
    big = torch.ones(3, 4, dtype=F64, device=dev)                          # overlapping views of one buffer
    args = [ip.data_ptr(), ix.data_ptr(), w.data_ptr(), None, 2, 2, 4, big[:2].data_ptr(), 1.0, None, 0.0, None, 0.0,
            big[1:].data_ptr(), None, 0, ops._stream()]
    assert _ffi.load().clipk_csr_spmm_f64(*args) == -1
    torch.cuda.synchronize()
    assert (big == 1).all()                                                # nothing was launched


# ------------------------------------------------------------------------------------------------ 2: connectivities
def _cloud(case):
    if case == "branch_k14":
        return ref.branch_cloud(300, 4, 1)[0], 14
    if case == "k1":
        return ref.branch_cloud(50, 4, 5)[0], 1
    x = ref.branch_cloud(120, 4, 7)[0]
    x[40:60] = x[0:20]                                                     # distance-0 neighbours
    x[60:64] = x[0]
    return x, 6


@pytest.mark.parametrize("case", ["branch_k14", "k1", "duplicates"])
def test_connectivities_on_the_device(dev, case):
    x, k = _cloud(case)
    N = x.shape[0]
    g = neighbors.knn_graph(torch.from_numpy(x).to(dev), k)
    d = g.distances.double().cpu().numpy()
    a_ref, rho_ref, sigma_ref = ref.membership_ref(d)
    if case == "duplicates":
        assert (d[:20, 0] == 0).all() and (rho_ref[:20] > 0).all()         # rho from the first positive distance
    # sigma is a bisection midpoint - a dyadic number that the glue reaches by the same decisions - or its floor, 1e-3 x the
    # row's distances added in neighbour order: the same bits on both sides.  (rho = 0, every neighbour at distance 0: the
    # floor is the global mean, whose summation order is not stated, and no weight depends on sigma.)
    rho, sigma = diffusion._smooth_knn(g.distances.double())
    some = rho_ref > 0
    assert np.array_equal(rho.cpu().numpy(), rho_ref)
    differ = np.flatnonzero(some & (sigma.cpu().numpy() != sigma_ref))
    assert differ.size == 0, (differ, sigma.cpu().numpy()[differ], sigma_ref[differ])
    assert np.abs(sigma.cpu().numpy() - sigma_ref).max() <= N * k * ref.EPS * sigma_ref.max()
    if case == "duplicates":                                               # the floor is active in some rows with positive distances
        floored = sigma_ref == 1e-3 * np.array([sum(row.tolist()) / k for row in d])
        assert ((d - rho_ref[:, None] > 0).any(1) & floored).sum() >= 4
    sg = diffusion.connectivities(g)
    indptr, cols, wts = ref.symmetrise_ref(g.indices.cpu().numpy(), a_ref)
    assert sg.nnz == 2 * N * k and sg.weights.dtype == F64 and sg.indices.dtype == torch.int32
    assert np.array_equal(sg.indptr.cpu().numpy(), indptr) and np.array_equal(sg.indices.cpu().numpy(), cols)
    rows = sg.rows().cpu().numpy()
    assert (np.diff(rows * N + cols) >= 0).all()                           # rows ascending, columns ascending inside a row
    # t = (d - rho) / sigma is the same f64 on both sides; the device's exp and libm's are each within an ulp of exp(-t), so a
    # and b differ by <= 2 eps relative; fl(a + b) <= 2 w and fl(a b) <= w carry that plus half an eps of their own rounding,
    # and the difference rounds once more: |dw| <= (2 w + w) (2 + 1/2) eps + eps w / 2 = 8 eps w; a subnormal exp(-t) (t > 708
    # under a floored sigma) is within an ulp in the subnormal spacing 2^-1074 instead
    got = sg.weights.cpu().numpy()
    err = np.abs(got - wts)
    print(f"connectivities {case}: max |dw| / w = {(err / np.where(wts > 0, wts, 1)).max() / ref.EPS:.2f} eps")
    assert (err <= 8 * ref.EPS * wts + 8 * 2.0 ** -1074).all()
    W = sg.to_dense()
    assert torch.equal(W, W.T)
    assert sg.max_row_length == int(np.diff(indptr).max())
    q = ref.csr_spmm_ref(indptr, cols, got, np.ones((N, 1)))[:, 0]
    assert _same_bits(sg.row_sums(), q)


# ------------------------------------------------------------------------------------------------ 3: eigenpairs
N_COMPS = 15
TOL = 1e-9
CLOUDS = {"branch300": lambda: ref.branch_cloud(300, 4, 1), "branch1500": lambda: ref.branch_cloud(1500, 8, 1),
          "blobs1200": lambda: ref.blob_cloud(1200, 16, 0)}
_solved = {}


def _solve(name, dev):
    """Computed once per cloud and shared, never changed: the device map and the dense f64 reference of the SAME graph."""
    if name not in _solved:
        x, par = CLOUDS[name]()[:2]
        g = neighbors.knn_graph(torch.from_numpy(x).to(dev), 14)
        dm = diffusion.diffusion_map(g, n_comps=N_COMPS, tol=TOL)
        T, s = ref.transition_ref(dm.graph.to_dense().cpu().numpy())
        lam, vec = ref.eigh_desc(T)
        _solved[name] = dict(x=x, par=par, g=g, dm=dm, T=T, s=s, lam=lam, vec=vec)
    return _solved[name]


def _gaps(lam, n):
    """gap[l] for l < n: the distance of reference eigenvalue l to the nearest one outside its cluster (eigenvalues within
    1e-6 of a neighbour form a cluster: the unit eigenvalues of a disconnected graph)."""
    gap = np.zeros(n)
    cl = ref.clusters(lam, n, 1e-6)
    for lo, hi, g in cl:
        gap[lo:hi] = g
    return gap, cl


@pytest.mark.parametrize("name", list(CLOUDS))
def test_eigenpairs_against_dense_eigh(dev, name):
    c = _solve(name, dev)
    dm, T, lam, vec = c["dm"], c["T"], c["lam"], c["vec"]
    N = T.shape[0]
    assert lam[N_COMPS - 1] - lam[N_COMPS] > 1e-3                         # on the reference alone: the cut is well separated
    assert lam[0] <= 1 + 1e-12 and lam[-1] >= -1 - 1e-12 and np.abs(T - T.T).max() <= 4 * ref.EPS * np.abs(T).max()
    theta, v = dm.eigenvalues.cpu().numpy(), dm.eigenvectors.cpu().numpy()
    assert dm.converged and dm.eigenvectors is dm.X_diffmap and v.shape == (N, N_COMPS) and theta.shape == (N_COMPS,)
    assert dm.n_spmm == 1 + (dm.n_outer - 1) * diffusion.CHEB_DEGREE
    res = np.linalg.norm(T @ v - v * theta, axis=0)
    print(f"{name}: n_outer {dm.n_outer} n_spmm {dm.n_spmm} max residual {res.max():.2e} (reported {float(dm.residuals.max()):.2e}) "
          f"max |theta - lambda| {np.abs(theta - lam[:N_COMPS]).max():.2e} n_unit {dm.n_unit} max row {dm.graph.max_row_length}")
    assert (np.diff(theta) <= 0).all() and np.abs(theta - lam[:N_COMPS]).max() <= TOL
    assert res.max() <= TOL + 1e-12 and float(dm.residuals.max()) <= TOL
    assert np.abs(v.T @ v - np.eye(N_COMPS)).max() <= 1e-12
    top = np.abs(v).argmax(0)                                              # argmax: the lowest index on ties
    assert (v[top, np.arange(N_COMPS)] > 0).all()
    n_unit = int((lam > 1 - 1e-8).sum())
    assert dm.n_unit == n_unit and n_unit == (3 if name == "blobs1200" else 1)
    # subspaces (Davis-Kahan): the computed vectors of a cluster of reference eigenvalues leave the reference eigenspace by at
    # most 2 |R_cluster|_F / gap; the reference's own eigenvectors carry its backward error N eps |T| over the same gap
    gap, cl = _gaps(lam, N_COMPS)
    share = 0.0
    for lo, hi, g in cl:
        u = vec[:, lo:hi]
        outside = np.linalg.norm(v[:, lo:hi] - u @ (u.T @ v[:, lo:hi]), 2)
        bound = 2 * np.linalg.norm(res[lo:hi]) / g + N * ref.EPS / g
        share = max(share, outside / bound)
        assert outside <= bound, (lo, hi, g, outside, bound)
    print(f"{name}: clusters {[(lo, hi) for lo, hi, _ in cl]} min gap {gap.min():.2e} largest share of the subspace bound {share:.3f}")


# ------------------------------------------------------------------------------------------------ 4: pseudotime
@pytest.mark.parametrize("n_dcs", [10, 15])
@pytest.mark.parametrize("name", list(CLOUDS))
def test_pseudotime_against_the_dense_reference(dev, name, n_dcs):
    c = _solve(name, dev)
    dm, lam, vec, T = c["dm"], c["lam"], c["vec"], c["T"]
    N = T.shape[0]
    roots = [int(np.argmin(c["par"])) if name != "blobs1200" else 0, N // 2, N - 1]
    got = diffusion.pseudotime(dm, roots, n_dcs)
    theta, v = dm.eigenvalues.cpu().numpy(), dm.eigenvectors.cpu().numpy()
    same = ref.pseudotime_ref(theta, v, roots, n_dcs)                     # the glue on its own eigenpairs
    assert got.shape == (3, N) and np.abs(got.cpu().numpy() - same).max() <= 1e-12
    for r, root in enumerate(roots):                                       # multi-root rows are the single-root calls
        assert torch.equal(diffusion.dpt(dm, root, n_dcs), got[r])
    # against dense eigh: component l moves by at most 2 res_l / g_l (item 3), weighted by w_l = lambda_l / (1 - lambda_l), over
    # the normalising maximum of the unnormalised reference distances
    wl = ref.pseudotime_weights(lam[:N_COMPS], n_dcs)
    res = np.linalg.norm(T @ v - v * theta, axis=0)
    gap, _ = _gaps(lam, N_COMPS)
    want = ref.pseudotime_ref(lam[:N_COMPS], vec[:, :N_COMPS], roots, n_dcs)
    for r, root in enumerate(roots):
        dmax = np.sqrt((((vec[:, :N_COMPS] - vec[root, :N_COMPS]) * wl) ** 2).sum(1)).max()
        bound = float((wl * 2 * res / gap).sum()) / dmax
        err = np.abs(got[r].cpu().numpy() - want[r]).max()
        print(f"{name} n_dcs {n_dcs} root {root}: |pseudotime - dense| {err:.2e} bound {bound:.2e} share {err / bound:.3f}")
        assert err <= bound
    if name != "blobs1200":                                                # the root at the smallest generating parameter
        rho_ref = ref.spearman_ref(want[0], c["par"])
        rho = float(diffusion.spearman(got[:1], torch.from_numpy(c["par"]).to(dev)[None])[0])
        print(f"{name} n_dcs {n_dcs}: Spearman(pseudotime, parameter) {rho:.4f}, dense reference {rho_ref:.4f}")
        assert rho_ref > 0.95 and rho >= rho_ref - 0.01
        assert abs(rho - ref.spearman_ref(got[0].cpu().numpy(), c["par"])) <= 1e-12


# ------------------------------------------------------------------------------------------------ 5: end to end
def test_end_to_end_from_a_raw_cloud(dev):
    c = _solve("branch300", dev)
    x = torch.from_numpy(c["x"]).to(dev)
    dm = diffusion.diffusion_map(x)                                        # n_neighbors = 15 counts the point: k = 14
    want = c["dm"]
    assert torch.equal(dm.graph.indptr, want.graph.indptr) and torch.equal(dm.graph.indices, want.graph.indices)
    assert torch.equal(dm.graph.weights, want.graph.weights)
    assert torch.equal(dm.eigenvalues, want.eigenvalues) and torch.equal(dm.eigenvectors, want.eigenvectors)
    assert (dm.n_outer, dm.n_spmm, dm.n_unit, dm.converged) == (want.n_outer, want.n_spmm, want.n_unit, True)
    again = diffusion.diffusion_map(want.graph, generator=torch.Generator(device=dev).manual_seed(9))   # another start
    assert again.converged and (again.eigenvalues - want.eigenvalues).abs().max() <= 2 * TOL


def test_cosine_metric_and_preservation(dev):
    c = _solve("branch300", dev)
    x = torch.from_numpy(c["x"]).to(dev)
    shifted = x + 2.0                                                      # away from the origin: angles are a proper metric
    dm = diffusion.diffusion_map(shifted, n_comps=5, metric="cosine")
    assert dm.converged and abs(float(dm.eigenvalues[0]) - 1) <= 1e-9 and torch.isfinite(dm.eigenvectors).all()
    assert dm.graph.nnz == 2 * 300 * 14
    root = int(np.argmin(c["par"]))
    rot = torch.linalg.qr(torch.randn(4, 4, generator=torch.Generator().manual_seed(2))).Q.to(dev)
    rho = diffusion.pseudotime_preservation(x, 3.0 * (x @ rot), [root, 7])   # a similarity keeps every neighbourhood
    assert rho.shape == (2,) and rho.dtype == F64 and (rho > 0.99).all()
