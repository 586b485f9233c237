"""LISI label masses of clip_dplm_amd.mixing (clipk_label_kernel_sums) against chunked torch on the same device, one JSON
line per shape.

  python3 tools/bench_lisi.py [--shapes s,m,m2,l2,l64,l512] [--iters 5] [--warmup 1] [--out profiles/lisi/bench_lisi.jsonl]

Shapes (N x P x G):  s     1024 x 128 x 10 (launch-bound)     m     65536 x 128 x 10       m2   65536 x 128 x 2
                     l2    131072 x 512 x 2                   l64   131072 x 512 x 64      l512 131072 x 512 x 512
(those of tools/bench_silhouette.py plus the two-modality case G = 2).
Inputs: Gaussian blobs (min(G, 10) centres ~ N(0, I), unit noise) and uniformly random labels, generated on the device
from a seed; beta and dmin from manifold.perplexity_bandwidths at perplexity 30, once, outside the timed region.
Measured, in the same process, the paths alternating within every iteration:
  stats       ops.label_kernel_sums, the row statistics only (want_out=False): the walk and its finalize launch
  out         the same with the [N, G] result written too
  dist        ops.label_dist_sums in sqeuclidean mode at the same shape: the same walk minus the exponential - the number
              to explain any gap against
  torch       row chunks of at most 1 GiB of distances: torch.cdist squared, exp(-beta (d - dmin)), the chunk's own
              diagonal zeroed, a matmul with the N x G one-hot, then mass and sumsq
  lisi        the whole mixing.lisi call, calibration (ten walks of clipk_cond_entropy_sums) included
  lisi_reuse  mixing.lisi with bandwidths= given: the norms, one walk, the glue
Time: device events around `inner` back-to-back calls after warm-up, divided by inner; the median of --iters, every timed
value in the record.  FLOPs of the walk: 2 N^2 P for the first product, 2 N^2 G for the second, against the 157.3 TFLOP/s
f32 matrix peak."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_dplm_amd import manifold, mixing, ops  # noqa: E402

F32_PEAK = 157.3e12
PERPLEXITY = 30.0

SHAPES = {
    "s": dict(N=1024, P=128, G=10, inner=100),
    "m": dict(N=65536, P=128, G=10, inner=2),
    "m2": dict(N=65536, P=128, G=2, inner=2),
    "l2": dict(N=131072, P=512, G=2, inner=1),
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


def torch_lisi(x, onehot, beta, dmin, chunk):
    out = []
    for i in range(0, len(x), chunk):
        d = torch.cdist(x[i:i + chunk], x).square_()
        w = d.sub_(dmin[i:i + chunk, None]).mul_(-beta[i:i + chunk, None]).exp_()
        r = torch.arange(w.shape[0], device=x.device)
        w[r, i + r] = 0
        m = w @ onehot
        out.append(m.sum(1).square() / (m * m).sum(1))
    return torch.cat(out)


def run(name, cfg, iters, warmup, dev):
    N, P, G, inner = cfg["N"], cfg["P"], cfg["G"], cfg["inner"]
    x, labels = inputs(N, P, G, dev)
    lab32 = labels.int()
    nx = (x * x).sum(1)
    onehot = torch.nn.functional.one_hot(labels, G).float()
    bw = manifold.perplexity_bandwidths(x, PERPLEXITY)
    beta, dmin = bw[0], bw[1]
    chunk = max(64, min(N, (1 << 28) // N))                               # <= 1 GiB of f32 distances per temporary
    calls = {
        "stats": lambda: ops.label_kernel_sums(x, x, lab32, G, beta, dmin, nx, nx, diag_offset=0, want_out=False),
        "out": lambda: ops.label_kernel_sums(x, x, lab32, G, beta, dmin, nx, nx, diag_offset=0),
        "dist": lambda: ops.label_dist_sums(x, x, lab32, G, "sqeuclidean", nx=nx, ny=nx, diag_offset=0),
        "torch": lambda: torch_lisi(x, onehot, beta, dmin, chunk),
        "lisi": lambda: mixing.lisi(x, labels, perplexity=PERPLEXITY, num_labels=G),
        "lisi_reuse": lambda: mixing.lisi(x, labels, perplexity=PERPLEXITY, num_labels=G, bandwidths=bw),
    }
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    t = {k: [] for k in calls}
    for _ in range(iters):                                                # alternating
        for k, fn in calls.items():
            t[k].append(timed(fn, inner))
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {"shape": name, "N": N, "P": P, "G": G, "inner": inner, "perplexity": PERPLEXITY, "torch_chunk_rows": chunk,
           "grid": list(ops.cond_entropy_sums_plan(N))}
    out.update({k + "_ms": round(v, 4) for k, v in med.items()})
    out.update({k + "_ms_all": [round(v, 4) for v in vals] for k, vals in t.items()})
    out["stats_vs_dist"] = round(med["stats"] / med["dist"], 3)
    out["out_vs_stats"] = round(med["out"] / med["stats"], 3)
    out["torch_vs_stats"] = round(med["torch"] / med["stats"], 3)
    out["torch_vs_lisi_reuse"] = round(med["torch"] / med["lisi_reuse"], 3)
    out["lisi_vs_stats"] = round(med["lisi"] / med["stats"], 3)
    first, second = 2.0 * N * N * P, 2.0 * N * N * G
    out["stats_f32_pipe_frac_first_product"] = round(first / F32_PEAK * 1e3 / med["stats"], 3)
    out["stats_f32_pipe_frac_both_products"] = round((first + second) / F32_PEAK * 1e3 / med["stats"], 3)
    out["dist_f32_pipe_frac_first_product"] = round(first / F32_PEAK * 1e3 / med["dist"], 3)
    fused, plain = mixing.lisi(x, labels, perplexity=PERPLEXITY, num_labels=G, bandwidths=bw), torch_lisi(x, onehot, beta, dmin,
                                                                                                       chunk)
    out["max_diff_vs_torch"] = float((fused - plain).abs().max())
    out["median_lisi"] = mixing.median_score(fused)
    del x, onehot
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="s,m,m2,l2,l64,l512")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_lisi.py measures on the GPU: no device found")
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
