"""The label-pair count of clip_dplm_amd.paga (ops.knn_label_pairs: clipk_knn_label_pairs) against the two torch routes to the
same G x G table that exist without it, on the same device and the same graph, one JSON line per (shape, labels, G); then
paga.paga end to end beside neighbors.knn_graph alone, one line per shape.

  python3 tools/bench_paga.py [--shapes m,l] [--groups 8,64,128,129,1024] [--iters 3] [--warmup 1]
                              [--out profiles/paga/bench_paga.jsonl]

Shapes (rows x neighbours):  m  65536 x 15      l  1048576 x 30
The graph is the exact kNN graph (neighbors.knn_graph) of a cloud of G_c = 64 Gaussian blobs in 16 dimensions (centres
~ 4 N(0, I), unit noise), generated on the device from a seed.  Labels, for every G:
  blob     the generating blob of each row mod G: most neighbours of a row carry its label (the contended diagonal)
  random   uniform over [0, G), independent of the cloud: M k entries spread over G^2 words
Measured, in the same process, the paths alternating within every iteration:
  kernel   ops.knn_label_pairs(idx, labels int32, G): one launch (the table's zeroing included)
  slab     route (a): graph.label_counts(labels, G), an [M, G] int64 slab, then index_add_ over the row labels
  flat     route (b): torch.bincount(labels[:, None] * G + labels[idx], minlength=G * G)
Time: device events around `inner` back-to-back calls after warm-up, divided by inner; the median of --iters, every timed
value in the record.  The three tables are compared for equality once per line.
idx_gb_s: the index stream's 8 M k bytes over the kernel's time - what the algorithm must read, the labels (4 M bytes,
cache-resident) left out; idx_hbm_frac: that against the 8.0 TB/s HBM3E peak.  At shape m the 7.9 MB of indices stay in
the caches between the back-to-back calls, so that figure is not a share of HBM bandwidth there; at shape l (252 MB)
they are about the size of the Infinity Cache.
End to end: paga.paga(x, labels, num_groups=64, tree=True) with the blob labels against neighbors.knn_graph(x, k) alone."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_dplm_amd import neighbors, ops, paga  # noqa: E402

HBM_PEAK = 8.0e12
BLOBS, P = 64, 16

SHAPES = {
    "m": dict(N=65536, k=15, inner=50, inner_torch=5),
    "l": dict(N=1 << 20, k=30, inner=10, inner_torch=1),
}


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner


def inputs(N, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    centres = 4.0 * torch.randn(BLOBS, P, device=dev, generator=g)
    blob = torch.randint(BLOBS, (N,), device=dev, generator=g)
    x = torch.randn(N, P, device=dev, generator=g) + centres[blob]
    return x, blob, g


def slab_route(graph, lab, G):
    rows = graph.label_counts(lab, G)
    return torch.zeros((G, G), dtype=torch.int64, device=lab.device).index_add_(0, lab, rows)


def flat_route(idx, lab, G):
    return torch.bincount((lab[:, None] * G + lab[idx]).reshape(-1), minlength=G * G).reshape(G, G)


def medians(calls, iters, warmup):
    for _ in range(warmup):
        for fn, inner in calls.values():
            fn()
    t = {n: [] for n in calls}
    for _ in range(iters):                                                # alternating
        for n, (fn, inner) in calls.items():
            t[n].append(timed(fn, inner))
    return {n: statistics.median(v) for n, v in t.items()}, t


def run_counts(name, cfg, graph, lab, kind, G, iters, warmup):
    N, k = cfg["N"], cfg["k"]
    idx, lab32 = graph.indices, lab.int()
    calls = {
        "kernel": (lambda: ops.knn_label_pairs(idx, lab32, G), cfg["inner"]),
        "slab": (lambda: slab_route(graph, lab, G), cfg["inner_torch"]),
        "flat": (lambda: flat_route(idx, lab, G), cfg["inner_torch"]),
    }
    med, t = medians(calls, iters, warmup)
    out = {"what": "counts", "shape": name, "N": N, "k": k, "labels": kind, "G": G,
           "path": "lds" if G <= 128 else "wave", "inner": cfg["inner"], "inner_torch": cfg["inner_torch"]}
    out.update({n + "_ms": round(v, 4) for n, v in med.items()})
    out.update({n + "_ms_all": [round(v, 4) for v in vals] for n, vals in t.items()})
    out["slab_vs_kernel"] = round(med["slab"] / med["kernel"], 2)
    out["flat_vs_kernel"] = round(med["flat"] / med["kernel"], 2)
    out["idx_gb_s"] = round(8.0 * N * k / (med["kernel"] * 1e-3) / 1e9, 1)
    out["idx_hbm_frac"] = round(8.0 * N * k / (med["kernel"] * 1e-3) / HBM_PEAK, 3)
    table = ops.knn_label_pairs(idx, lab32, G)
    out["equal_tables"] = bool(torch.equal(table, slab_route(graph, lab, G)) and torch.equal(table, flat_route(idx, lab, G)))
    out["diagonal_share"] = round(float(table.diagonal().sum()) / float(table.sum()), 4)
    return out


def run_end_to_end(name, cfg, x, blob, iters, warmup):
    N, k = cfg["N"], cfg["k"]
    calls = {
        "paga": (lambda: paga.paga(x, blob, n_neighbors=k + 1, num_groups=BLOBS), 1),
        "knn_graph": (lambda: neighbors.knn_graph(x, k), 1),
    }
    med, t = medians(calls, iters, warmup)
    out = {"what": "end_to_end", "shape": name, "N": N, "P": P, "k": k, "G": BLOBS}
    out.update({n + "_ms": round(v, 3) for n, v in med.items()})
    out.update({n + "_ms_all": [round(v, 3) for v in vals] for n, vals in t.items()})
    out["paga_minus_graph_ms"] = round(med["paga"] - med["knn_graph"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="m,l")
    ap.add_argument("--groups", default="8,64,128,129,1024")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_paga.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")

    def emit(record):
        line = json.dumps(record)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    for name in a.shapes.split(","):
        cfg = SHAPES[name]
        x, blob, g = inputs(cfg["N"], dev)
        graph = neighbors.knn_graph(x, cfg["k"])
        for G in (int(v) for v in a.groups.split(",")):
            labels = {"blob": blob % G, "random": torch.randint(G, (cfg["N"],), device=dev, generator=g)}
            for kind, lab in labels.items():
                emit(run_counts(name, cfg, graph, lab, kind, G, a.iters, a.warmup))
                torch.cuda.empty_cache()
        emit(run_end_to_end(name, cfg, x, blob, a.iters, a.warmup))
        del x, blob, graph
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
