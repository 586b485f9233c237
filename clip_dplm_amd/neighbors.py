"""Exact k-nearest-neighbour graphs of embedding clouds on the device, without the N x N matrix.

The other embedding-space tools of this package use every pair; this one gives a cloud's NEIGHBOURS - what kBET, the
published (kNN-truncated) LISI, label transfer from an atlas and kNN-preservation scores start from.

    knn_graph     the k nearest rows of y (or the k nearest OTHER rows of x) of every row of x, nearest first, with their
                  squared distances: KNNGraph.

How.  argmin_j |x_i - y_j|^2 = argmax_j z_ij with z_ij = <x_i, y_j> - |y_j|^2 / 2, so the search is the tile walk of
retrieval.topk with a key-side bias (ops.sim_knn; include/clipk.h: clipk_sim_knn).  The walk keeps at most 64 results per
row in registers; beyond that it RESUMES: round r asks for the next min(64, k - 64 r) keys after a cursor, the (score,
index) of the previous round's last result.  The cursor is a position in the walk's total order (z descending, equal z by
the lower index), so duplicate rows that straddle a round boundary come out once each.  The cursors are device tensors:
nothing is read back and a call can be captured in a graph.  k neighbours cost ceil(k / 64) walks.

The order is that of z in f32.  The returned squared distances are recomputed from the differences of the listed pairs
(ops.pair_sqdist) - |x|^2 - 2 z would cancel exactly where neighbours are closest - so they are accurate values of those
pairs, and may be out of order by rounding-sized amounts where two neighbours are nearly equally far.

Row exclusion (y=None) is by index, not by distance: another row equal to row i is a neighbour at distance 0.
There is no CPU fallback; KNNGraph's own methods are torch glue that also takes host tensors.
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import torch

from . import _args, ops

__all__ = ["KNNGraph", "knn_graph", "MAX_K", "ROUND_K"]

METRICS = ("euclidean", "cosine")
MAX_K = 1024                 # 16 walks
ROUND_K = 64                 # results of one walk: the register lists of clipk_sim_knn


@dataclasses.dataclass
class KNNGraph:
    """indices int64 [M, k]: row i's k neighbours, nearest first (equal z: the lower index first); sqdist f32 [M, k]: their
    squared distances (metric "cosine": 1 - cos)."""
    indices: torch.Tensor
    sqdist: torch.Tensor

    @property
    def k(self) -> int:
        return self.indices.shape[1]

    @property
    def distances(self) -> torch.Tensor:
        """f32 [M, k]: sqdist.sqrt()."""
        return self.sqdist.sqrt()

    def label_counts(self, labels, num_labels: int) -> torch.Tensor:
        """int64 [M, G]: how many of each row's neighbours carry each label.  labels: integer tensor over the searched rows
        (the rows of y, or of x for a self graph) with values in 0..G-1, on the graph's device; a value outside [0, G), and
        an index -1, count for no label."""
        if not isinstance(labels, torch.Tensor) or labels.is_floating_point() or labels.dtype == torch.bool \
                or labels.dim() != 1:
            raise TypeError("labels must be a 1-D integer tensor")
        _args.int_in("num_labels", num_labels, 1)
        idx = self.indices
        lab = labels.long().to(idx.device)[idx.clamp(min=0)]
        ok = (idx >= 0) & (lab >= 0) & (lab < num_labels)
        out = torch.zeros((idx.shape[0], num_labels), dtype=torch.int64, device=idx.device)
        return out.scatter_add_(1, lab.clamp(0, num_labels - 1), ok.long())


def check_graph(graph):
    if not isinstance(graph, KNNGraph) or not isinstance(graph.indices, torch.Tensor) \
            or not isinstance(graph.sqdist, torch.Tensor):
        raise ValueError("graph must be a KNNGraph (neighbors.knn_graph)")
    i, d = graph.indices, graph.sqdist
    if i.dtype != torch.int64 or i.dim() != 2 or i.shape[1] == 0 or d.shape != i.shape or not d.is_floating_point() \
            or d.device != i.device:
        raise ValueError("graph must hold int64 indices [M, k] and floating sqdist [M, k] on one device")


def _check_args(x, k, y, metric, row_block):
    """Every argument error, before any device work."""
    _args.check_cloud(x)
    if y is not None:
        _args.check_cloud(y, "y")
    if y is not None and y.shape[1] != x.shape[1]:
        raise ValueError(f"x has {x.shape[1]} columns, y {y.shape[1]}")
    _args.check_metric(metric, METRICS)
    Ny = x.shape[0] if y is None else y.shape[0]
    kmax = min(MAX_K, Ny - 1 if y is None else Ny)
    _args.int_in("k", k, 1, kmax, what=f"an int in [1, min(1024, {'N - 1' if y is None else 'Ny'})] = [1, {kmax}]")
    _args.int_in("row_block", row_block, 1)
    _args.need_device("knn_graph needs", x, y)
    if y is not None and y.device != x.device:
        raise ValueError(f"x is on {x.device}, y on {y.device}")


@torch.no_grad()
def knn_graph(x, k: int, y=None, metric: str = "euclidean", row_block: int = 65536) -> KNNGraph:
    """The k nearest rows of y [Ny, P] of every row of x [M, P] (f32, device, P % 4 == 0), nearest first: KNNGraph(indices
    int64 [M, k], sqdist f32 [M, k]).

    y=None searches x against itself with each row excluded BY INDEX (an equal other row is a neighbour at distance 0);
    then 1 <= k <= min(1024, M - 1), with y 1 <= k <= min(1024, Ny).
    metric "euclidean": sqdist = |x_i - y_j|^2; "cosine": the rows are L2-normalised first and sqdist = 1 - cos.
    Equally near keys (equal z = <x_i, y_j> - |y_j|^2 / 2 in f32) come in ascending index.  Rows go through in blocks of
    row_block against all of y; the result does not depend on it.  ceil(k / 64) walks; no host read - capturable."""
    _check_args(x, k, y, metric, row_block)
    xs = _args.prepare(x, metric)
    ys = xs if y is None else _args.prepare(y, metric)
    idx = _rounds(xs, ys, k, y is None, row_block)
    return KNNGraph(idx, ops.pair_sqdist(xs, ys, idx))


def _rounds(xs, ys, k, skip_self, row_block):
    """int64 [M, k]: the round loop over ops.sim_knn on prepared clouds - per row block ceil(k / 64) walks, each resuming
    after the previous one's last (score, index)."""
    bias = -0.5 * (ys * ys).sum(1)
    M = xs.shape[0]
    idx = torch.empty((M, k), dtype=torch.int64, device=xs.device)
    for r0 in range(0, M, row_block):
        xb = xs[r0:r0 + row_block]
        after = None
        for c0 in range(0, k, ROUND_K):
            kk = min(ROUND_K, k - c0)
            s, i = ops.sim_knn(xb, ys, kk, bias=bias, diag_offset=r0 if skip_self else -1, after=after)
            idx[r0:r0 + row_block, c0:c0 + kk] = i
            if c0 + kk < k:
                after = (s[:, kk - 1].contiguous(), i[:, kk - 1].contiguous())
    return idx
