"""Diffusion maps and diffusion pseudotime on the exact kNN graph - the representation the reference trains on.

The reference's DiffMapProteinCLIP trains on adata.obsm['X_diffmap'] and its tri-modal cell tower reads dpt_pseudotime
and connectivities; all three come from scanpy (sc.pp.neighbors -> sc.tl.diffmap -> sc.tl.dpt) on the host.  This module
builds them on the device from neighbors.knn_graph:

    connectivities           UMAP's fuzzy simplicial set of a KNNGraph (scanpy's default method='umap'): SymGraph, a CSR
                             matrix of fixed size 2 N k that is bitwise symmetric.
    diffusion_map            the n_comps algebraically largest eigenpairs of scanpy's density-normalised, symmetrised
                             transition matrix T = S W S (compute_transitions(density_normalize=True) + compute_eigen).
    pseudotime / dpt         scanpy's DPT distance from one or many roots, each row divided by its maximum.
    pseudotime_preservation  Spearman correlation of two clouds' pseudotimes, per root.

Neither umap-learn nor scanpy is a dependency, and neither was available to compare against: the definitions below follow
UMAP's published smooth_knn_dist / compute_membership_strengths and scanpy's compute_transitions / DPT as written in
their papers and documentation, and the docstrings here (restated in f64 numpy by tests/diffusion_ref.py) are the contract.

T is never materialised: ops.csr_spmm (include/clipk.h: clipk_csr_spmm_f64) applies diag(s) W diag(s) to a block of f64
vectors with a two-term epilogue, so one launch is one step of the Chebyshev recurrence.  The eigen-solver is
Chebyshev-filtered subspace iteration: its QR and its small eigh are torch.linalg calls, and it reads the residual norms
back once per outer iteration (it is not capturable).  There is no CPU fallback for the operator; connectivities,
pseudotime and SymGraph's own methods are torch glue that also takes host tensors.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional

import torch

from . import _args, neighbors, ops
from .neighbors import KNNGraph

__all__ = ["SymGraph", "DiffusionMap", "connectivities", "diffusion_map", "pseudotime", "dpt",
           "pseudotime_preservation", "MAX_COMPS", "CHEB_DEGREE"]

MAX_COMPS = 32
CHEB_DEGREE = 20
SIGMA_STEPS = 64             # bisection steps of smooth_knn_dist
SIGMA_TOL = 1e-5
MIN_K_DIST_SCALE = 1e-3
UNIT_EPS = 1e-8              # an eigenvalue above 1 - UNIT_EPS counts as 1: one per connected component


@dataclasses.dataclass
class SymGraph:
    """A symmetric weighted graph in CSR: indptr int64 [N + 1], indices int32 [nnz], weights f64 [nnz], rows in ascending
    column order.  From connectivities nnz = 2 N k whatever the graph: a mutual pair (i, j) appears twice in row i, the
    first entry with the combined weight and the second with weight 0, so nothing is read back to size the arrays."""
    indptr: torch.Tensor
    indices: torch.Tensor
    weights: torch.Tensor

    @property
    def n(self) -> int:
        return self.indptr.shape[0] - 1

    @property
    def nnz(self) -> int:
        return self.indices.shape[0]

    def rows(self) -> torch.Tensor:
        """int64 [nnz]: the row of every entry."""
        e = torch.arange(self.nnz, device=self.indptr.device)
        return torch.searchsorted(self.indptr[1:].contiguous(), e, right=True)

    def to_dense(self) -> torch.Tensor:
        """f64 [N, N] (tests and small graphs): entries of one (row, column) are added, and the second of a mutual pair is
        an exact 0, so the matrix equals its transpose bitwise."""
        out = torch.zeros((self.n, self.n), dtype=torch.float64, device=self.weights.device)
        return out.index_put_((self.rows(), self.indices.long()), self.weights, accumulate=True)

    def row_sums(self) -> torch.Tensor:
        """f64 [N]: W 1.  On the device through ops.csr_spmm (its fixed summation order); on the host each row's entries
        are added in ascending order."""
        if self.weights.is_cuda:
            one = torch.ones((self.n, 1), dtype=torch.float64, device=self.weights.device)
            return ops.csr_spmm(self.indptr, self.indices, self.weights, one).reshape(-1)
        out = torch.zeros(self.n, dtype=torch.float64)
        return out.index_add_(0, self.rows(), self.weights)

    @property
    def max_row_length(self) -> int:
        """The longest row (k + in-degree of the hub).  Reads the host."""
        return int((self.indptr[1:] - self.indptr[:-1]).max())


@dataclasses.dataclass
class DiffusionMap:
    """eigenvalues f64 [n_comps], descending; eigenvectors f64 [N, n_comps]: orthonormal eigenvectors of the SYMMETRIC
    T = S W S as scanpy stores them, component 0 (eigenvalue 1, proportional to z = 1 / (s q)) included, each with its entry of
    largest magnitude positive (the lowest index on ties); residuals f64 [n_comps]: |T v - theta v|_2; n_outer / n_spmm:
    outer iterations and operator applications the solver spent; converged: every residual <= tol; n_unit: eigenvalues above
    1 - 1e-8, the number of connected components among the computed ones; graph: the SymGraph."""
    eigenvalues: torch.Tensor
    eigenvectors: torch.Tensor
    residuals: torch.Tensor
    n_outer: int
    n_spmm: int
    converged: bool
    n_unit: int
    graph: SymGraph

    @property
    def X_diffmap(self) -> torch.Tensor:
        return self.eigenvectors


# --------------------------------------------------------------------------------------------------
def _smooth_knn(d: torch.Tensor):
    """(rho f64 [N], sigma f64 [N]) of UMAP's smooth_knn_dist on the distances d f64 [N, k] of k OTHER neighbours."""
    N, k = d.shape
    target = math.log2(k + 1)
    inf = torch.full((), math.inf, dtype=torch.float64, device=d.device)
    rho = torch.where(d > 0, d, inf).min(1).values
    rho = torch.where(torch.isinf(rho), torch.zeros_like(rho), rho)
    diff = d - rho[:, None]
    lo = torch.zeros(N, dtype=torch.float64, device=d.device)
    hi = torch.full((N,), math.inf, dtype=torch.float64, device=d.device)
    mid = torch.ones(N, dtype=torch.float64, device=d.device)
    done = torch.zeros(N, dtype=torch.bool, device=d.device)
    for _ in range(SIGMA_STEPS):                                        # masked: a finished row is frozen, no host read
        psum = torch.where(diff > 0, torch.exp(-(diff / mid[:, None])), torch.ones_like(diff)).sum(1)
        done = done | ((psum - target).abs() < SIGMA_TOL)
        above = psum > target
        hi_n = torch.where(above, mid, hi)
        lo_n = torch.where(above, lo, mid)
        mid_n = torch.where(above | ~torch.isinf(hi_n), (lo_n + hi_n) / 2, mid * 2)
        lo, hi, mid = torch.where(done, lo, lo_n), torch.where(done, hi, hi_n), torch.where(done, mid, mid_n)
    total = d[:, 0]
    for j in range(1, k):                                               # the row's distances added in neighbour order: a stated
        total = total + d[:, j]                                         # order, because a floored sigma enters exp(-x / sigma)
    mean = total / torch.full_like(total, k)                            # a true division (by a scalar torch multiplies by 1 / k)
    floor = MIN_K_DIST_SCALE * torch.where(rho > 0, mean, d.mean())
    return rho, torch.maximum(mid, floor)


def _check_self_graph(graph):
    neighbors.check_graph(graph)
    N, k = graph.indices.shape
    if N < 2 or k > N - 1:
        raise ValueError(f"graph must be a cloud's graph against itself (neighbors.knn_graph(x, k)): {N} rows with {k} "
                         "neighbours each")
    if N >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 rows (int32 columns)")


@torch.no_grad()
def connectivities(graph: KNNGraph) -> SymGraph:
    """UMAP's fuzzy simplicial set (scanpy's method='umap' connectivities) of a cloud's KNNGraph against itself: SymGraph.

    d_ij = graph.distances in f64 (unsquared) of the k OTHER neighbours; scanpy's n_neighbors counts the point itself, so
    its n_neighbors = 15 is k = 14.  Per row: rho_i = the smallest positive d_ij (0 if there is none); sigma_i by 64 steps
    of bisection from lo = 0, hi = inf, mid = 1 on psum = sum_j (d_ij - rho_i > 0 ? exp(-(d_ij - rho_i) / mid) : 1)
    against log2(k + 1): stop (freeze the row) once |psum - target| < 1e-5; psum > target: hi = mid, mid = (lo + hi) / 2;
    else lo = mid and mid doubles while hi is inf, else mid = (lo + hi) / 2.  sigma_i is floored at 1e-3 x the row's mean
    distance, summed in neighbour order (rho_i = 0, where no weight depends on sigma: x the global mean).  a_ij = 1 where d_ij - rho_i <= 0, else exp(-(d_ij - rho_i) / sigma_i).
    W = A + A^T - A o A^T entry by entry as fl(fl(a + b) - fl(a b)) with b = a_ji or 0: bitwise symmetric.

    The 2 N k entries (i, j, a_ij) and (j, i, a_ij) are sorted by (row, column); of two adjacent equal keys (a mutual
    pair) the first takes the combined weight and the second keeps its column with weight 0.  f64 torch glue without a
    host read; takes host graphs too.  These are UMAP's published definitions, not a comparison against umap-learn."""
    _check_self_graph(graph)
    idx = graph.indices
    N, k = idx.shape
    rho, sigma = _smooth_knn(graph.distances.double())
    diff = graph.distances.double() - rho[:, None]
    a = torch.where(diff > 0, torch.exp(-(diff / sigma[:, None])), torch.ones_like(diff)).reshape(-1)
    i = torch.arange(N, device=idx.device)[:, None].expand(N, k).reshape(-1)
    j = idx.reshape(-1)
    key, order = torch.cat([i * N + j, j * N + i]).sort(stable=True)
    v = torch.cat([a, a])[order]
    same = key[1:] == key[:-1]
    false = torch.zeros(1, dtype=torch.bool, device=idx.device)
    first, second = torch.cat([same, false]), torch.cat([false, same])
    b = torch.cat([v[1:], v[:1]])                                       # the partner of a first entry is the next one
    w = torch.where(second, torch.zeros_like(v), torch.where(first, (v + b) - (v * b), v))
    indptr = torch.searchsorted(key, torch.arange(N + 1, device=idx.device) * N)
    return SymGraph(indptr, (key % N).int(), w)


# --------------------------------------------------------------------------------------------------
def _check_map_args(x_or_graph, n_comps, n_neighbors, metric, tol, max_outer, generator):
    """Every argument error of diffusion_map, before any device work.  Returns the number of rows."""
    if isinstance(x_or_graph, SymGraph):
        g = x_or_graph
        ok = all(isinstance(t, torch.Tensor) for t in (g.indptr, g.indices, g.weights))
        if not ok or g.indptr.dtype != torch.int64 or g.indices.dtype != torch.int32 or g.weights.dtype != torch.float64 \
                or g.indptr.dim() != 1 or g.indptr.shape[0] < 2 or g.indices.dim() != 1 or g.weights.shape != g.indices.shape:
            raise ValueError("a SymGraph must hold indptr int64 [N + 1], indices int32 [nnz] and weights f64 [nnz]")
        N = g.n
    elif isinstance(x_or_graph, KNNGraph):
        _check_self_graph(x_or_graph)
        N = x_or_graph.indices.shape[0]
    else:
        _args.check_cloud(x_or_graph)
        N = x_or_graph.shape[0]
        _args.check_metric(metric, neighbors.METRICS)
        kmax = min(neighbors.MAX_K + 1, N)
        _args.int_in("n_neighbors (the point itself included)", n_neighbors, 2, kmax,
                     what=f"an int in [2, min(1025, N)] = [2, {kmax}]")
    _args.int_in("n_comps", n_comps, 1, min(MAX_COMPS, N),
                 what=f"an int in [1, min({MAX_COMPS}, N)] = [1, {min(MAX_COMPS, N)}]")
    if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not tol > 0:
        raise ValueError(f"tol must be a positive number, got {tol!r}")
    _args.int_in("max_outer", max_outer, 1)
    if generator is not None and not isinstance(generator, torch.Generator):
        raise ValueError("generator must be None or a torch.Generator")
    dev = x_or_graph.weights if isinstance(x_or_graph, SymGraph) else \
        x_or_graph.indices if isinstance(x_or_graph, KNNGraph) else x_or_graph
    if not dev.is_cuda:
        raise ValueError("diffusion_map needs device tensors (there is no CPU fallback for the operator)")
    return N


def block_size(n_comps: int, N: int) -> int:
    """Vectors the subspace iteration carries: min(64, max(2 n_comps, n_comps + 8)), at most N."""
    return min(64, max(2 * n_comps, n_comps + 8), N)


def transition_scaling(graph: SymGraph) -> torch.Tensor:
    """s f64 [N] with T = diag(s) W diag(s): q = W 1, K_ij = W_ij / (q_i q_j), z_i = sqrt(sum_j K_ij), s_i = 1 / (q_i z_i)
    (scanpy's compute_transitions with density_normalize=True, then its symmetrisation)."""
    q = graph.row_sums()
    one = torch.ones((graph.n, 1), dtype=torch.float64, device=q.device)
    z = ops.csr_spmm(graph.indptr, graph.indices, graph.weights, one, s=1.0 / q).reshape(-1).sqrt()
    return 1.0 / (q * z)


def _fix_signs(v: torch.Tensor) -> torch.Tensor:
    """Each column's entry of largest magnitude made positive (argmax returns the lowest index on ties)."""
    top = v.abs().argmax(0)
    sign = torch.sign(v.gather(0, top[None, :]))
    return v * torch.where(sign == 0, torch.ones_like(sign), sign)


def _solve(graph: SymGraph, s: torch.Tensor, n_comps: int, tol: float, max_outer: int, generator):
    """Chebyshev-filtered subspace iteration for the n_comps largest eigenpairs of T = diag(s) W diag(s).

    The spectrum lies in [-1, 1].  Per outer iteration: Rayleigh-Ritz on the orthonormal block V [N, m] (one operator
    application, an m x m eigh), the residuals of the leading n_comps Ritz pairs (the one host read), then the degree-20
    Chebyshev polynomial of the map of [-1, b] onto [-1, 1], b = the block's smallest Ritz value, applied to V by the
    three-term recurrence (19 further applications, each ONE csr_spmm launch with its epilogue; the first step reuses T V)
    and a QR."""
    N = graph.n
    m = block_size(n_comps, N)
    ip, ix, w = graph.indptr, graph.indices, graph.weights
    if generator is None:
        generator = torch.Generator(device=w.device).manual_seed(0)
    v = torch.randn((N, m), dtype=torch.float64, device=generator.device, generator=generator).to(w.device)
    v = torch.linalg.qr(v).Q.contiguous()                                # (the device QR returns column-major)
    n_spmm = 0
    for outer in range(1, max_outer + 1):
        tv = ops.csr_spmm(ip, ix, w, v, s=s)
        n_spmm += 1
        h = v.T @ tv
        theta, qm = torch.linalg.eigh((h + h.T) / 2)
        theta, qm = theta.flip(0), qm.flip(1)                           # descending
        v, tv = v @ qm, tv @ qm
        res = (tv - v * theta).norm(dim=0)
        *res_host, b = torch.cat([res[:n_comps], theta[-1:]]).tolist()  # the convergence check: one host read
        if max(res_host) <= tol or outer == max_outer:
            break
        c, e = (b - 1.0) / 2, (b + 1.0) / 2                             # centre and half-width of [-1, b]
        prev, cur = v, (tv - c * v) / e
        for _ in range(CHEB_DEGREE - 1):                                # y_{t+1} = (2 / e) (T y_t - c y_t) - y_{t-1}
            nxt = ops.csr_spmm(ip, ix, w, cur, s=s, alpha=2 / e, b=cur, beta=-2 * c / e, c=prev, gamma=-1.0, out=prev)
            n_spmm += 1
            prev, cur = cur, nxt
        v = torch.linalg.qr(cur).Q.contiguous()
    return theta[:n_comps].clone(), v[:, :n_comps], res[:n_comps].clone(), outer, n_spmm, max(res_host) <= tol


@torch.no_grad()
def diffusion_map(x_or_graph, n_comps: int = 15, n_neighbors: int = 15, metric: str = "euclidean", tol: float = 1e-9,
                  max_outer: int = 50, generator: Optional[torch.Generator] = None) -> DiffusionMap:
    """The n_comps algebraically largest eigenpairs of the diffusion-map transition matrix of a cloud, in f64: DiffusionMap.

    x_or_graph: a device cloud f32 [N, P] (P % 4 == 0; its exact graph of n_neighbors - 1 other rows under `metric` is
    built: scanpy's n_neighbors counts the point itself), a KNNGraph of a cloud against itself, or a SymGraph.
    With W = connectivities: q = W 1, K_ij = W_ij / (q_i q_j), z_i = sqrt(sum_j K_ij), T_ij = K_ij / (z_i z_j)
    = (S W S)_ij with s_i = 1 / (q_i z_i) - scanpy's compute_transitions(density_normalize=True) and compute_eigen.
    1 <= n_comps <= 32.  tol bounds every returned residual |T v - theta v|_2 when `converged`; the vectors are orthonormal
    to rounding and signed as DiffusionMap says.  generator seeds the starting block (None: a fixed seed - two calls give
    the same bits).  Eigenvalues that agree to within tol (one per connected component at 1, `n_unit` of them) have
    eigenvectors that are only defined as a subspace.  Reads the host once per outer iteration; not capturable."""
    N = _check_map_args(x_or_graph, n_comps, n_neighbors, metric, tol, max_outer, generator)
    if isinstance(x_or_graph, SymGraph):
        graph = x_or_graph
    elif isinstance(x_or_graph, KNNGraph):
        graph = connectivities(x_or_graph)
    else:
        graph = connectivities(neighbors.knn_graph(x_or_graph, n_neighbors - 1, metric=metric))
    s = transition_scaling(graph)
    theta, v, res, n_outer, n_spmm, converged = _solve(graph, s, n_comps, float(tol), max_outer, generator)
    n_unit = int((theta > 1 - UNIT_EPS).sum())
    return DiffusionMap(theta, _fix_signs(v), res, n_outer, n_spmm, converged, n_unit, graph)


# --------------------------------------------------------------------------------------------------
def _check_roots(roots, N):
    if isinstance(roots, torch.Tensor):
        if roots.is_floating_point() or roots.dtype == torch.bool or roots.dim() > 1:
            raise ValueError("roots must be an int, a sequence of ints or a 1-D integer tensor")
        roots = roots.reshape(-1).tolist()
    elif isinstance(roots, int) and not isinstance(roots, bool):
        roots = [roots]
    if not isinstance(roots, (list, tuple)) or not roots \
            or any(isinstance(r, bool) or not isinstance(r, int) for r in roots):
        raise ValueError("roots must be an int, a non-empty sequence of ints or a 1-D integer tensor")
    if any(not 0 <= r < N for r in roots):
        raise ValueError(f"roots must lie in [0, {N}), got {list(roots)}")
    return list(roots)


def _check_dm(dm, n_dcs):
    if not isinstance(dm, DiffusionMap) or not isinstance(dm.eigenvalues, torch.Tensor) \
            or not isinstance(dm.eigenvectors, torch.Tensor) or dm.eigenvectors.dim() != 2 \
            or dm.eigenvalues.shape != dm.eigenvectors.shape[1:]:
        raise ValueError("dm must be a DiffusionMap (diffusion.diffusion_map)")
    _args.int_in("n_dcs", n_dcs, 1)


@torch.no_grad()
def pseudotime(dm: DiffusionMap, roots, n_dcs: int = 10) -> torch.Tensor:
    """f64 [R, N]: scanpy's diffusion pseudotime from each root.  Of the components l < n_dcs those with lambda_l <=
    1 - 1e-8 count (the stationary vector of every connected component is left out, as scanpy leaves out component 0):
        D_r(i) = sqrt(sum_l (lambda_l / (1 - lambda_l))^2 (psi_l(i) - psi_l(root_r))^2),   row r divided by its maximum.
    roots: an int, a sequence of ints or a 1-D integer tensor (read on the host to check its range).  With dm.n_unit > 1
    the graph is disconnected and the values of rows in another component than the root are not meaningful (scanpy sets
    them to inf; per-component pseudotime is not done here).  Torch glue: takes host tensors too."""
    _check_dm(dm, n_dcs)
    roots = _check_roots(roots, dm.eigenvectors.shape[0])
    lam, psi = dm.eigenvalues.double(), dm.eigenvectors.double()
    use = (torch.arange(lam.shape[0], device=lam.device) < n_dcs) & (lam <= 1 - UNIT_EPS)
    wl = torch.where(use, lam / (1 - torch.where(use, lam, torch.zeros_like(lam))), torch.zeros_like(lam))
    r = torch.tensor(roots, dtype=torch.int64, device=psi.device)
    delta = (psi[None, :, :] - psi[r][:, None, :]) * wl                # [R, N, L]
    d = (delta * delta).sum(2).sqrt()
    return d / d.max(1, keepdim=True).values


def dpt(dm: DiffusionMap, root: int, n_dcs: int = 10) -> torch.Tensor:
    """f64 [N]: pseudotime from one root."""
    if isinstance(root, bool) or not isinstance(root, int):
        raise ValueError(f"root must be an int, got {root!r}")
    return pseudotime(dm, [root], n_dcs)[0]


def _average_ranks(v: torch.Tensor) -> torch.Tensor:
    """f64 [R, N]: ranks 0 .. N - 1 along the rows, equal values sharing the mean of their ranks."""
    srt = v.sort(1).values.contiguous()
    v = v.contiguous()
    return (torch.searchsorted(srt, v, right=False) + torch.searchsorted(srt, v, right=True) - 1).double() / 2


def spearman(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """f64 [R]: Spearman's rank correlation of the rows of a and b [R, N] (Pearson's of the average ranks)."""
    ra, rb = _average_ranks(a.double()), _average_ranks(b.double())
    ra, rb = ra - ra.mean(1, keepdim=True), rb - rb.mean(1, keepdim=True)
    return (ra * rb).sum(1) / ((ra * ra).sum(1) * (rb * rb).sum(1)).sqrt()


@torch.no_grad()
def pseudotime_preservation(x_a, x_b, roots, n_dcs: int = 10, **map_args) -> torch.Tensor:
    """f64 [R]: is pseudotime preserved between two spaces?  Spearman's correlation, per root, of the diffusion pseudotimes
    of the clouds (or graphs) x_a and x_b over the same N rows; map_args go to diffusion_map."""
    dm_a, dm_b = diffusion_map(x_a, **map_args), diffusion_map(x_b, **map_args)
    if dm_a.eigenvectors.shape[0] != dm_b.eigenvectors.shape[0]:
        raise ValueError(f"x_a has {dm_a.eigenvectors.shape[0]} rows, x_b {dm_b.eigenvectors.shape[0]}")
    return spearman(pseudotime(dm_a, roots, n_dcs), pseudotime(dm_b, roots, n_dcs))
