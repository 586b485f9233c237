"""One Lloyd iteration of clip_dplm_amd.cluster (clipk_kmeans_step) against the torch path on the same device, one JSON
line per shape.

  python3 tools/bench_kmeans.py [--shapes xl10,xl64,m,s,w] [--iters 7] [--warmup 2] [--out profiles/kmeans/bench_kmeans.jsonl]

Shapes (N x P x K):  xl10  2^20 x 512 x 10       xl64  2^20 x 512 x 64
                     m     65536 x 128 x 10      s     1024 x 128 x 10 (launch-bound)
                     w     131072 x 512 x 1024 (the two-launch path: ops.sim_top2_bias assigns, ops.kmeans_step sums)
Inputs: Gaussian blobs (K centres ~ N(0, I), unit noise), centroids = K rows of x, generated on the device from a seed.
Measured, in the same process, the two paths alternating within every iteration:
  fused_iter    cluster._lloyd: the centroid norms, the step (one launch for K <= 64, two beyond), the division by the
                counts and the centroid shift - what kmeans() runs per iteration
  torch_iter    torch.cdist (row chunks of at most 2 GiB of distances) + argmin, index_add_, bincount, the same division
  fused_update / torch_update (shape w)   the update launch alone - ops.kmeans_step(labels=...) - against index_add_ +
                bincount under the same labels
Time: device events around `inner` back-to-back calls after warm-up, divided by inner; the median of --iters.  Every
timed value is in the record, with the agreement of the two paths on these inputs."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_dplm_amd import cluster, ops  # noqa: E402

SHAPES = {
    "xl10": dict(N=1 << 20, P=512, K=10, inner=3),
    "xl64": dict(N=1 << 20, P=512, K=64, inner=3),
    "m": dict(N=65536, P=128, K=10, inner=50),
    "s": dict(N=1024, P=128, K=10, inner=200),
    "w": dict(N=131072, P=512, K=1024, inner=3),
}


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner


def inputs(N, P, K, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    centres = torch.randn(K, P, device=dev, generator=g)
    x = torch.randn(N, P, device=dev, generator=g)
    x += centres[torch.randint(K, (N,), device=dev, generator=g)]
    return x, x[torch.randperm(N, device=dev, generator=g)[:K]].clone()


def torch_assign(x, c, chunk):
    return torch.cat([torch.cdist(x[i:i + chunk], c).argmin(1) for i in range(0, len(x), chunk)])


def torch_update(x, c, labels):
    sums = torch.zeros_like(c).index_add_(0, labels, x)
    counts = torch.bincount(labels, minlength=len(c))
    return sums, counts


def torch_iter(x, c, chunk):
    labels = torch_assign(x, c, chunk)
    sums, counts = torch_update(x, c, labels)
    new = torch.where(counts[:, None] > 0, sums / counts.clamp_min(1)[:, None], c)
    return new, labels, (new - c).square().sum()


def run(name, cfg, iters, warmup, dev):
    N, P, K, inner = cfg["N"], cfg["P"], cfg["K"], cfg["inner"]
    x, c = inputs(N, P, K, dev)
    chunk = max(64, min(N, (1 << 29) // K))                              # <= 2 GiB of f32 distances per temporary
    calls = {"fused_iter": lambda: cluster._lloyd(x, c, "euclidean", None), "torch_iter": lambda: torch_iter(x, c, chunk)}
    if K > ops.KMEANS_MAX_K_FUSED:
        lab32 = cluster._lloyd(x, c, "euclidean", None)[1]
        lab64 = lab32.long()
        calls["fused_update"] = lambda: ops.kmeans_step(x, c, labels=lab32)
        calls["torch_update"] = lambda: torch_update(x, c, lab64)
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    t = {k: [] for k in calls}
    for _ in range(iters):                                                # alternating
        for k, fn in calls.items():
            t[k].append(timed(fn, inner))
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {"shape": name, "N": N, "P": P, "K": K, "inner": inner, "torch_chunk_rows": chunk,
           "grid": list(ops.kmeans_step_plan(N, K))}
    out.update({k + "_ms": round(v, 4) for k, v in med.items()})
    out.update({k + "_ms_all": [round(v, 4) for v in vals] for k, vals in t.items()})
    out["iter_speedup_vs_torch"] = round(med["torch_iter"] / med["fused_iter"], 3)
    if "fused_update" in med:
        out["update_speedup_vs_torch"] = round(med["torch_update"] / med["fused_update"], 3)
    # the work of the launch: two 64-centroid-wide products per 64-centroid block (the update alone for K > 64) against
    # the 157.3 TFLOP/s f32 matrix peak, and x read once against 8 TB/s
    kb = 64 * ((K + 63) // 64)
    out["fused_iter_flop"] = 2.0 * N * kb * P * 2
    out["x_bytes"] = 4.0 * N * P
    # agreement of the two paths on these inputs
    new_f, lab_f, _, _ = cluster._lloyd(x, c, "euclidean", None)
    new_t, lab_t, _ = torch_iter(x, c, chunk)
    out["labels_differ"] = int((lab_f.long() != lab_t).sum())
    out["max_centroid_diff"] = float((new_f - new_t).abs().max())
    del x, c
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="xl10,xl64,m,s,w")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_kmeans.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    for name in a.shapes.split(","):
        line = json.dumps(run(name, SHAPES[name], a.iters, a.warmup, dev))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
