"""Silhouette widths of clip_dplm_amd.cluster (clipk_label_dist_sums) against chunked torch on the same device, one JSON
line per shape.

  python3 tools/bench_silhouette.py [--shapes s,m,l64,l512] [--iters 7] [--warmup 2] [--out profiles/silhouette/bench_silhouette.jsonl]

Shapes (N x P x G):  s     1024 x 128 x 10 (launch-bound)     m     65536 x 128 x 10
                     l64   131072 x 512 x 64                  l512  131072 x 512 x 512
Inputs: Gaussian blobs (min(G, 10) centres ~ N(0, I), unit noise) and uniformly random labels, generated on the device
from a seed.  Measured, in the same process, the paths alternating within every iteration:
  fused          cluster.silhouette_samples: the norms, the walk(s), the O(N G) glue
  torch          row chunks of at most 1 GiB of distances: torch.cdist, the chunk's own diagonal zeroed, a matmul with
                 the N x G one-hot, the same glue
  sums           ops.label_dist_sums alone (norms given): the walk and its finalize launch
  sums_rowsplit  (G <= 64) the same labels with n_labels = 65: the first product is the same and the second takes the
                 form for many labels, four 16-key blocks with waves owning 32 label rows each - against `sums`, where the
                 four waves split the keys, this is the cost of leaving waves idle at few labels
  ksum_kbary     ops.kernel_sums with kbary at the same Mx, Ny, P, one bandwidth: the nearest existing kernel
  ksum           ops.kernel_sums without kbary: the first product and the element function alone, no second product
  sklearn        (shape s, if importable) sklearn.metrics.silhouette_samples on the host, the copies included; host clock
Time: device events around `inner` back-to-back calls after warm-up, divided by inner; the median of --iters, every timed
value in the record.  FLOPs of the walk: 2 N^2 P for the first product, 2 N^2 G for the second, against the 157.3 TFLOP/s
f32 matrix peak."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_dplm_amd import cluster, ops  # noqa: E402

F32_PEAK = 157.3e12

SHAPES = {
    "s": dict(N=1024, P=128, G=10, inner=100),
    "m": dict(N=65536, P=128, G=10, inner=2),
    "l64": dict(N=131072, P=512, G=64, inner=1),
    "l512": dict(N=131072, P=512, G=512, inner=1),
}


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner


def inputs(N, P, G, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    K = min(G, 10)
    centres = torch.randn(K, P, device=dev, generator=g)
    x = torch.randn(N, P, device=dev, generator=g)
    x += centres[torch.randint(K, (N,), device=dev, generator=g)]
    labels = torch.randint(G, (N,), device=dev, generator=g)
    labels[:G] = torch.arange(G, device=dev)                               # every label present
    return x, labels


def glue(d, own, n):
    n_own = n[own]
    a = d.gather(1, own[:, None])[:, 0] / (n_own - 1).clamp_min(1.0)
    b = (d / n[None, :]).scatter_(1, own[:, None], float("inf")).min(1).values
    s = torch.nan_to_num((b - a) / torch.maximum(a, b))
    return torch.where(n_own > 1, s, torch.zeros_like(s))


def torch_silhouette(x, labels, onehot, n, chunk):
    out = []
    for i in range(0, len(x), chunk):
        d = torch.cdist(x[i:i + chunk], x)
        r = torch.arange(d.shape[0], device=x.device)
        d[r, i + r] = 0
        out.append(glue(d @ onehot, labels[i:i + chunk], n))
    return torch.cat(out)


def run(name, cfg, iters, warmup, dev):
    N, P, G, inner = cfg["N"], cfg["P"], cfg["G"], cfg["inner"]
    x, labels = inputs(N, P, G, dev)
    lab32 = labels.int()
    nx = (x * x).sum(1)
    onehot = torch.nn.functional.one_hot(labels, G).float()
    n = onehot.sum(0)
    chunk = max(64, min(N, (1 << 28) // N))                               # <= 1 GiB of f32 distances per temporary
    one = torch.ones(1, device=dev)
    calls = {
        "fused": lambda: cluster.silhouette_samples(x, labels),
        "torch": lambda: torch_silhouette(x, labels, onehot, n, chunk),
        "sums": lambda: ops.label_dist_sums(x, x, lab32, G, nx=nx, ny=nx, diag_offset=0),
        "ksum_kbary": lambda: ops.kernel_sums(x, x, one, one, nx, nx, diag_offset=0, want_bary=True),
        "ksum": lambda: ops.kernel_sums(x, x, one, one, nx, nx, diag_offset=0),
    }
    if G <= 64:
        calls["sums_rowsplit"] = lambda: ops.label_dist_sums(x, x, lab32, 65, nx=nx, ny=nx, diag_offset=0)
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    t = {k: [] for k in calls}
    for _ in range(iters):                                                # alternating
        for k, fn in calls.items():
            t[k].append(timed(fn, inner))
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {"shape": name, "N": N, "P": P, "G": G, "inner": inner, "torch_chunk_rows": chunk,
           "grid": list(ops.label_dist_sums_plan(N, N))}
    out.update({k + "_ms": round(v, 4) for k, v in med.items()})
    out.update({k + "_ms_all": [round(v, 4) for v in vals] for k, vals in t.items()})
    out["speedup_vs_torch"] = round(med["torch"] / med["fused"], 3)
    out["sums_vs_ksum_kbary"] = round(med["sums"] / med["ksum_kbary"], 3)
    if "sums_rowsplit" in med:
        out["keysplit_vs_rowsplit"] = round(med["sums_rowsplit"] / med["sums"], 3)
    first, second = 2.0 * N * N * P, 2.0 * N * N * G
    out["sums_f32_pipe_frac_first_product"] = round(first / F32_PEAK * 1e3 / med["sums"], 3)
    out["sums_f32_pipe_frac_both_products"] = round((first + second) / F32_PEAK * 1e3 / med["sums"], 3)
    out["ksum_f32_pipe_frac_first_product"] = round(first / F32_PEAK * 1e3 / med["ksum"], 3)
    out["max_diff_vs_torch"] = float((cluster.silhouette_samples(x, labels) - torch_silhouette(x, labels, onehot, n, chunk))
                                     .abs().max())
    if name == "s":
        try:
            from sklearn.metrics import silhouette_samples
        except ImportError:
            out["sklearn_ms"] = None
        else:
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s = torch.from_numpy(silhouette_samples(x.cpu().numpy(), labels.cpu().numpy())).to(dev)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            out["sklearn_ms"] = round(statistics.median(ts), 3)
            out["max_diff_vs_sklearn"] = float((cluster.silhouette_samples(x, labels) - s.float()).abs().max())
    del x, onehot
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="s,m,l64,l512")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_silhouette.py measures on the GPU: no device found")
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
