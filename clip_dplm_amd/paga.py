"""PAGA: the graph of a cloud's clusters, abstracted from its exact kNN graph - the coarse topology beside the diffusion map.

The reference's cell-tower data preparation runs sc.tl.paga on the neighbour graph before sc.tl.diffmap and sc.tl.dpt
(tong/utils/data.py:43-49, compute_paga_dpt of the tri-modal notebook).  neighbors and diffusion put the other two
steps on the device; this module is the first one, for any labelling of the rows (cluster.kmeans or annotations):

    group_edge_counts     the G x G count of graph edges by (label of the row, label of the neighbour) - everything in
                          PAGA derives from this one table; with key_labels over an atlas it is the kNN label-transfer
                          confusion matrix of a query cloud.
    paga                  PAGA v1.2 (scanpy's default model): expected edge counts under random wiring, connectivities
                          = observed / expected capped at 1, and their maximum spanning forest: PAGAResult.
    connectivities_tree   the forest step on its own.
    modularity            Newman's Q of a labelling on diffusion.connectivities - the quantity Leiden maximises, so any
                          labelling of a cloud can be scored against the graph.
    paga_preservation     is the coarse topology preserved between two spaces?  Spearman's correlation of the
                          connectivities and the Jaccard index of the tree edges.

Neither scanpy nor igraph is a dependency, and neither was available to compare against: the definitions below follow
PAGA v1.2 as published (Wolf et al., Genome Biology 2019, and the model as scanpy's documentation states it), and the
docstrings here (restated in numpy loops by tests/paga_ref.py) are the contract.  A comparison with scanpy has not been
made.  Out of scope: Leiden / Louvain clustering itself, PAGA v1.0, transitions_confidence (RNA velocity),
PAGA-initialised layouts and more than one GPU.

The table comes from ONE pass over the [N, k] indices (ops.knn_label_pairs; include/clipk.h: clipk_knn_label_pairs) with
no intermediate that grows with N x G; the rest is f64 torch glue on G x G tensors.  There is no CPU fallback for the
search; everything after it also takes host graphs.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Optional

import torch

from . import _args, diffusion, neighbors, ops
from .diffusion import SymGraph
from .neighbors import KNNGraph

__all__ = ["PAGAResult", "PAGAPreservation", "group_edge_counts", "paga", "connectivities_tree", "modularity",
           "paga_preservation", "MAX_GROUPS"]

MAX_GROUPS = ops.LABEL_PAIRS_MAX_G


@dataclasses.dataclass
class PAGAResult:
    """counts int64 [G, G]: graph edges by (label of the row, label of the neighbour); sizes int64 [G]: rows per label;
    expected f64 [G, G]: the edges between two clusters under random wiring (diagonal 0); connectivities f64 [G, G]:
    symmetric, diagonal 0, in [0, 1]; tree f64 [G, G] or None: the connectivities on the edges of their maximum spanning
    forest, symmetric; num_groups: G; k: neighbours per row of the graph (scanpy's n_neighbors - 1)."""
    counts: torch.Tensor
    sizes: torch.Tensor
    expected: torch.Tensor
    connectivities: torch.Tensor
    tree: Optional[torch.Tensor]
    num_groups: int
    k: int


@dataclasses.dataclass
class PAGAPreservation:
    """spearman: f64 scalar tensor, Spearman's correlation of the G (G - 1) / 2 upper-triangle connectivities of the two
    spaces; tree_jaccard: f64 scalar tensor, tree edges in both / tree edges in either (1 when neither has an edge)."""
    spearman: torch.Tensor
    tree_jaccard: torch.Tensor


# --------------------------------------------------------------------------------------------------
def _positions(labels: torch.Tensor, G: int, device) -> torch.Tensor:
    """int64 [n] on `device`: the label where it lies in [0, G), else G (the slot that is dropped)."""
    labels = labels.to(device)
    return torch.where((labels >= 0) & (labels < G), labels, torch.full_like(labels, G))


def _int32_labels(labels: torch.Tensor, G: int, device) -> torch.Tensor:
    """int32 [n]: the kernel's labels; a value outside [0, G) - one outside int32 included - becomes -1."""
    pos = _positions(labels, G, device)
    return torch.where(pos < G, pos, torch.full_like(pos, -1)).int().contiguous()


def _check_counts_args(graph, labels, num_groups, key_labels):
    neighbors.check_graph(graph)
    _args.int_in("num_groups", num_groups, 1, MAX_GROUPS)
    labels = _args.labels_arg("labels", labels, graph.indices.shape[0])
    if key_labels is not None:
        key_labels = _args.labels_arg("key_labels", key_labels)
        if key_labels.shape[0] == 0:
            raise ValueError("key_labels is empty")
    if graph.indices.is_cuda and graph.indices.shape[1] > ops.LABEL_PAIRS_MAX_K:
        raise ValueError(f"at most {ops.LABEL_PAIRS_MAX_K} neighbours per row on the device, got {graph.indices.shape[1]}")
    return labels, key_labels


def _counts(graph, labels, G, key_labels):
    idx = graph.indices
    if idx.is_cuda:
        rl = _int32_labels(labels, G, idx.device)
        kl = None if key_labels is None else _int32_labels(key_labels, G, idx.device)
        return ops.knn_label_pairs(idx.contiguous(), rl, G, kl)
    a = _positions(labels, G, idx.device)
    kl = a if key_labels is None else _positions(key_labels, G, idx.device)
    Ny = kl.shape[0]
    b = kl[idx.clamp(0, Ny - 1)]
    a = a[:, None].expand_as(idx)
    ok = (idx >= 0) & (idx < Ny) & (a < G) & (b < G)
    return torch.bincount((a * G + b)[ok], minlength=G * G).reshape(G, G)


@torch.no_grad()
def group_edge_counts(graph: KNNGraph, labels, num_groups: int, key_labels=None) -> torch.Tensor:
    """int64 [G, G]: counts[a, b] = #{(i, t) : labels[i] = a and key_labels[graph.indices[i, t]] = b}.

    graph: any KNNGraph - of a cloud against itself, or of x against y with key_labels over y's rows (then the table is
    the kNN label-transfer confusion matrix of x's annotation against the atlas's).  labels: integer tensor [M] over the
    graph's rows; key_labels: integer tensor [Ny] over the searched rows, None: the row labels.  Only values in
    [0, num_groups) count, 1 <= num_groups <= 1024: a row label outside, a neighbour label outside, and an index outside
    [0, Ny) - the -1 of a missing result - each count nowhere.
    A device graph goes through ops.knn_label_pairs: one pass over the indices, no [M, G] intermediate, no host read
    (capturable), k <= 1024.  A host graph: one flat torch.bincount of a G + b over the valid entries.  Exact."""
    labels, key_labels = _check_counts_args(graph, labels, num_groups, key_labels)
    return _counts(graph, labels, num_groups, key_labels)


# --------------------------------------------------------------------------------------------------
def _check_conn(conn):
    if not isinstance(conn, torch.Tensor) or conn.dtype != torch.float64 or conn.dim() != 2 \
            or conn.shape[0] != conn.shape[1] or conn.shape[0] == 0:
        raise ValueError("conn must be a float64 tensor of shape (G, G)")


@torch.no_grad()
def connectivities_tree(conn: torch.Tensor) -> torch.Tensor:
    """f64 [G, G], symmetric: conn on the edges of the maximum spanning forest of the symmetric f64 [G, G] matrix conn,
    0 elsewhere.  This is scanpy's minimum spanning tree of 1 / connectivities, carrying the connectivities.

    Kruskal over the pairs a < b with conn[a, b] > 0 (the upper triangle is read), sorted by conn descending and, among
    equal values, by (a, b) ascending; a pair joins the forest when its ends are not yet connected.  Connectivities
    saturate at 1, so ties are common and THE TIE RULE IS PART OF THE CONTRACT: scipy's minimum_spanning_tree may pick
    other edges among tied ones (the total weight agrees).  Reads the matrix on the host; the result is on conn's device."""
    _check_conn(conn)
    G = conn.shape[0]
    host = conn.detach().cpu()
    a, b = torch.triu_indices(G, G, 1)                                  # row-major: (a, b) ascending
    v = host[a, b]
    keep = v > 0
    a, b, v = a[keep], b[keep], v[keep]
    order = torch.sort(v, descending=True, stable=True).indices        # stable: ties stay in (a, b) order
    parent = list(range(G))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    tree = torch.zeros((G, G), dtype=torch.float64)
    left = G - 1
    for ea, eb, ev in zip(a[order].tolist(), b[order].tolist(), v[order].tolist()):
        ra, rb = find(ea), find(eb)
        if ra == rb:
            continue
        parent[max(ra, rb)] = min(ra, rb)
        tree[ea, eb] = tree[eb, ea] = ev
        left -= 1
        if left == 0:
            break
    return tree.to(conn.device)


def _check_paga_args(x_or_graph, groups, n_neighbors, metric, num_groups, tree):
    """Every argument error of paga, before any device work.  Returns (the labels as int64, the number of rows)."""
    if isinstance(x_or_graph, KNNGraph):
        diffusion._check_self_graph(x_or_graph)
        N = x_or_graph.indices.shape[0]
        if x_or_graph.indices.is_cuda and x_or_graph.indices.shape[1] > ops.LABEL_PAIRS_MAX_K:
            raise ValueError(f"at most {ops.LABEL_PAIRS_MAX_K} neighbours per row, got {x_or_graph.indices.shape[1]}")
    else:
        _args.check_cloud(x_or_graph)
        N = x_or_graph.shape[0]
        _args.check_metric(metric, neighbors.METRICS)
        kmax = min(neighbors.MAX_K + 1, N)
        _args.int_in("n_neighbors (the point itself included)", n_neighbors, 2, kmax,
                     what=f"an int in [2, min(1025, N)] = [2, {kmax}]")
        k = n_neighbors - 1
    if isinstance(x_or_graph, KNNGraph):
        k = x_or_graph.indices.shape[1]
    if 2 * N * N * k >= 2 ** 63:
        raise ValueError(f"{N} rows with {k} neighbours: the numerator of `expected` (up to 2 N^2 k) would not fit int64")
    labels = _args.labels_arg("groups", groups, N)
    _args.int_in("num_groups", num_groups, 1, MAX_GROUPS, optional=True)
    if not isinstance(tree, bool):
        raise ValueError(f"tree must be a bool, got {tree!r}")
    if not isinstance(x_or_graph, KNNGraph):
        _args.need_device("paga builds a cloud's graph from", x_or_graph)
    return labels, N


def _relabel(labels, num_groups):
    """(positions, G): the labels as they came with num_groups, else their ranks among torch.unique's values."""
    if num_groups is not None:
        return labels, num_groups
    values, inv = torch.unique(labels, return_inverse=True)
    if values.shape[0] > MAX_GROUPS:
        raise ValueError(f"at most {MAX_GROUPS} distinct groups, got {values.shape[0]}")
    return inv, values.shape[0]


def _paga(graph, labels, G, tree):
    dev = graph.indices.device
    C = _counts(graph, labels, G, None)
    pos = _positions(labels, G, dev)
    ns = torch.zeros(G + 1, dtype=torch.int64, device=dev).scatter_add_(0, pos, torch.ones_like(pos))[:G]
    n = ns.sum()
    es = C.sum(1)
    off = ~torch.eye(G, dtype=torch.bool, device=dev)
    inter = C * off
    sym = inter + inter.T
    num = (es[:, None] * ns[None, :] + es[None, :] * ns[:, None]) * off
    expected = num.double() / (n - 1).clamp(min=1).double()
    one, zero = torch.ones_like(expected), torch.zeros_like(expected)
    conn = torch.where(sym == 0, zero, torch.where(expected == 0, one, torch.minimum(one, sym.double() / expected)))
    return PAGAResult(C, ns, expected, conn, connectivities_tree(conn) if tree else None, G, graph.indices.shape[1])


@torch.no_grad()
def paga(x_or_graph, groups, n_neighbors: int = 15, metric: str = "euclidean", num_groups: Optional[int] = None,
         tree: bool = True) -> PAGAResult:
    """PAGA v1.2 (scanpy's default model) of a labelled cloud on its exact kNN graph: PAGAResult.

    x_or_graph: a device cloud f32 [N, P] (P % 4 == 0; its exact graph of n_neighbors - 1 OTHER rows under `metric` is
    built: scanpy's n_neighbors counts the point itself, 2 <= n_neighbors <= min(1025, N)), or a KNNGraph of a cloud
    against itself (device or host).  groups: integer tensor [N].  num_groups=None relabels with torch.unique (any
    integer values; the one host read: G is a shape; at most 1024 distinct values) and group g is the g-th smallest value.
    num_groups=G: the labels are already 0..G-1; a value outside counts nowhere - its row is no part of n or of any
    cluster, and edges from or to it are dropped.

    With C = counts = group_edge_counts(graph, groups, G) (the DIRECTED kNN edges: scanpy's `ones` matrix), ns[a] = rows
    labelled a, n = sum ns, es[a] = sum_b C[a, b] (inner plus outgoing edges of a: scanpy's es), inter = C with a zero
    diagonal and sym = inter + inter^T, all int64, for a != b:
        expected[a, b]       = fl( f64(es[a] ns[b] + es[b] ns[a]) / f64(n - 1) )     the integer exact (2 N^2 k < 2^63 is
                               checked), then ONE conversion and ONE division (n <= 1: divided by 1; the numerator is 0)
        connectivities[a, b] = 0 where sym[a, b] = 0, else 1 where expected[a, b] = 0, else min(1, fl(f64(sym[a, b]) /
                               expected[a, b]))
    and both diagonals are 0.  scanpy stores `expected` only where sym > 0; here EVERY off-diagonal pair has it.
    tree: connectivities_tree(connectivities), which reads the [G, G] matrix on the host; tree=False leaves it None, and
    with num_groups given the call then reads nothing back and can be captured in a graph.
    A correctly rounded f64 division gives on the device the bits a numpy restatement gives on the host."""
    labels, _ = _check_paga_args(x_or_graph, groups, n_neighbors, metric, num_groups, tree)
    graph = x_or_graph if isinstance(x_or_graph, KNNGraph) else \
        neighbors.knn_graph(x_or_graph, n_neighbors - 1, metric=metric)
    labels, G = _relabel(labels.to(graph.indices.device), num_groups)
    return _paga(graph, labels, G, tree)


# --------------------------------------------------------------------------------------------------
def _check_sym_graph(g):
    ok = isinstance(g, SymGraph) and all(isinstance(t, torch.Tensor) for t in (g.indptr, g.indices, g.weights))
    if not ok or g.indptr.dtype != torch.int64 or g.indices.dtype != torch.int32 or g.weights.dtype != torch.float64 \
            or g.indptr.dim() != 1 or g.indptr.shape[0] < 2 or g.indices.dim() != 1 or g.weights.shape != g.indices.shape:
        raise ValueError("graph must be a SymGraph (diffusion.connectivities): indptr int64 [N + 1], indices int32 [nnz] "
                         "and weights f64 [nnz]")


@torch.no_grad()
def modularity(graph: SymGraph, labels, num_groups: int, resolution: float = 1.0) -> torch.Tensor:
    """f64 scalar tensor: Newman's modularity of a labelling on a weighted symmetric graph, the quantity Leiden maximises
    on diffusion.connectivities - any labelling of a cloud (k-means, annotations) can be scored against the graph:
        Q = sum_c [ in_c / W - resolution (tot_c / W)^2 ]
    over the CSR entries whose row AND column are labelled in [0, num_groups): in_c = the weight sum of the entries with
    both ends in c, tot_c = the weight sum of the entries whose row is in c, W = sum_c tot_c.  resolution = 0 gives the
    fraction of in-cluster weight.  labels: integer tensor [N]; 1 <= num_groups <= 1024; resolution >= 0.
    f64 torch glue (torch.bincount with weights over the nnz entries, whose order of summation is not fixed on the
    device); host or device; no [N, G] intermediate.  W = 0 gives nan."""
    _check_sym_graph(graph)
    labels = _args.labels_arg("labels", labels, graph.n)
    _args.int_in("num_groups", num_groups, 1, MAX_GROUPS)
    if isinstance(resolution, bool) or not isinstance(resolution, (int, float)) or not resolution >= 0 \
            or math.isinf(resolution):
        raise ValueError(f"resolution must be a non-negative finite number, got {resolution!r}")
    G, dev = num_groups, graph.weights.device
    pos = _positions(labels, G, dev)
    a = pos[graph.rows()]
    b = pos[graph.indices.long().clamp(0, graph.n - 1)]
    ok = (a < G) & (b < G)
    w = torch.where(ok, graph.weights, torch.zeros_like(graph.weights))
    tot = torch.bincount(torch.where(ok, a, torch.full_like(a, G)), weights=w, minlength=G + 1)[:G]
    inn = torch.bincount(torch.where(ok & (a == b), a, torch.full_like(a, G)), weights=w, minlength=G + 1)[:G]
    W = tot.sum()
    return (inn / W - float(resolution) * (tot / W) ** 2).sum()


@torch.no_grad()
def paga_preservation(x_a, x_b, groups, **paga_args) -> PAGAPreservation:
    """Is the coarse topology preserved between two spaces?  x_a and x_b are two clouds (or KNNGraphs) over the same N rows
    and groups one labelling of them; paga_args (n_neighbors, metric, num_groups) go to paga.  PAGAPreservation(spearman of
    the two spaces' upper-triangle connectivities (diffusion.spearman; nan when one side is constant), tree_jaccard of
    their tree edges).  Needs G >= 3 (ValueError otherwise): one pair has no rank correlation.  The counterpart of
    diffusion.pseudotime_preservation for the cluster graph."""
    args = {k: paga_args.pop(k) for k in ("n_neighbors", "metric", "num_groups") if k in paga_args}
    if paga_args:
        raise TypeError(f"unexpected arguments {sorted(paga_args)}")
    args = {"n_neighbors": 15, "metric": "euclidean", "num_groups": None, **args}
    labels, _ = _check_paga_args(x_a, groups, tree=True, **args)
    _check_paga_args(x_b, groups, tree=True, **args)                   # (groups has one entry per row of either)
    labels, G = _relabel(labels, args["num_groups"])
    if G < 3:
        raise ValueError(f"paga_preservation needs at least 3 groups, got {G}")
    args["num_groups"] = G
    ra, rb = paga(x_a, labels, **args), paga(x_b, labels, **args)
    iu = torch.triu_indices(G, G, 1, device=ra.connectivities.device)
    ca, cb = ra.connectivities[iu[0], iu[1]], rb.connectivities.to(ra.connectivities.device)[iu[0], iu[1]]
    ta, tb = ra.tree[iu[0], iu[1]] > 0, rb.tree.to(ra.tree.device)[iu[0], iu[1]] > 0
    both, either = (ta & tb).sum().double(), (ta | tb).sum().double()
    jac = torch.where(either > 0, both / either.clamp(min=1), torch.ones_like(both))
    return PAGAPreservation(diffusion.spearman(ca[None], cb[None])[0], jac)
