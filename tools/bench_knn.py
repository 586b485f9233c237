"""The exact k-nearest-neighbour graph of clip_dplm_amd.neighbors (clipk_sim_knn + clipk_pair_sqdist) against chunked torch
on the same device and against the route manifold._knn takes, one JSON line per (shape, k).

  python3 tools/bench_knn.py [--shapes s,m,l] [--ks 15,64,89,256] [--iters 3] [--warmup 1] [--out profiles/knn/bench_knn.jsonl]

Shapes (N x P):  s  1024 x 128 (launch-bound)      m  65536 x 128      l  131072 x 512
Inputs: Gaussian blobs (10 centres ~ N(0, I), unit noise) generated on the device from a seed; the cloud against itself.
Measured, in the same process, the paths alternating within every iteration:
  knn      neighbors.knn_graph(x, k): the norms, ceil(k / 64) walks of clipk_sim_knn, clipk_pair_sqdist
  walks    the walks alone (neighbors._rounds): knn minus the distances
  topk64   ops.sim_topk(x, x, 64) at the same shape: the cost of ONE plain walk - knn per round is held against it
  old      manifold._knn(x, k), k <= 63 only: two widened copies of the cloud, retrieval.topk for k + 1, the row removed
  torch    row chunks of at most 1 GiB of distances: torch.cdist, the chunk's own diagonal set to +inf, torch.topk(k,
           largest=False)
Time: device events around `inner` back-to-back calls after warm-up, divided by inner; the median of --iters, every timed
value in the record.  FLOPs of one walk: 2 N^2 P against the 157.3 TFLOP/s f32 matrix peak."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_dplm_amd import manifold, neighbors, ops  # noqa: E402

F32_PEAK = 157.3e12

SHAPES = {
    "s": dict(N=1024, P=128, inner=50),
    "m": dict(N=65536, P=128, inner=1),
    "l": dict(N=131072, P=512, inner=1),
}


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner


def inputs(N, P, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    centres = torch.randn(10, P, device=dev, generator=g)
    x = torch.randn(N, P, device=dev, generator=g)
    x += centres[torch.randint(10, (N,), device=dev, generator=g)]
    return x


def torch_knn(x, k, chunk):
    idx, dist = [], []
    for i in range(0, len(x), chunk):
        d = torch.cdist(x[i:i + chunk], x)
        r = torch.arange(d.shape[0], device=x.device)
        d[r, i + r] = float("inf")
        v, j = torch.topk(d, k, dim=1, largest=False)
        idx.append(j)
        dist.append(v)
    return torch.cat(idx), torch.cat(dist)


def run(name, cfg, k, iters, warmup, dev):
    N, P, inner = cfg["N"], cfg["P"], cfg["inner"]
    x = inputs(N, P, dev)
    chunk = max(64, min(N, (1 << 28) // N))                               # <= 1 GiB of f32 distances per temporary
    calls = {
        "knn": lambda: neighbors.knn_graph(x, k),
        "walks": lambda: neighbors._rounds(x, x, k, True, 65536),
        "topk64": lambda: ops.sim_topk(x, x, 64),
        "torch": lambda: torch_knn(x, k, chunk),
    }
    if k <= 63:
        calls["old"] = lambda: manifold._knn(x, k)
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    t = {n: [] for n in calls}
    for _ in range(iters):                                                # alternating
        for n, fn in calls.items():
            t[n].append(timed(fn, inner))
    med = {n: statistics.median(v) for n, v in t.items()}
    rounds = (k + 63) // 64
    out = {"shape": name, "N": N, "P": P, "k": k, "rounds": rounds, "inner": inner, "torch_chunk_rows": chunk}
    out.update({n + "_ms": round(v, 4) for n, v in med.items()})
    out.update({n + "_ms_all": [round(v, 4) for v in vals] for n, vals in t.items()})
    out["torch_vs_knn"] = round(med["torch"] / med["knn"], 3)
    if "old" in med:
        out["old_vs_knn"] = round(med["old"] / med["knn"], 3)
    out["walks_per_round_vs_topk64"] = round(med["walks"] / rounds / med["topk64"], 3)
    out["sqdist_ms"] = round(med["knn"] - med["walks"], 4)
    out["walk_f32_pipe_frac"] = round(2.0 * N * N * P / F32_PEAK * 1e3 / (med["walks"] / rounds), 3)
    graph = neighbors.knn_graph(x, k)
    ti, td = torch_knn(x, k, chunk)
    out["rows_with_torch_index_set"] = float((graph.indices.sort(1).values == ti.sort(1).values).all(1).float().mean())
    out["max_dist_diff_vs_torch"] = float((graph.distances.sort(1).values - td.sort(1).values).abs().max())
    del x, graph, ti, td
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="s,m,l")
    ap.add_argument("--ks", default="15,64,89,256")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_knn.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    for name in a.shapes.split(","):
        for k in (int(v) for v in a.ks.split(",")):
            line = json.dumps(run(name, SHAPES[name], k, a.iters, a.warmup, dev))
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
