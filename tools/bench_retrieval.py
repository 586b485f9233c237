"""Fused retrieval kernels (clipk_sim_topk / clipk_sim_rank) against the materialising baseline, one JSON line per shape.

  python3 tools/bench_retrieval.py [--shapes a,b,c,d] [--iters 5] [--warmup 2] [--out profiles/retrieval/bench.jsonl]
                                   [--prefilter none,bf16,bf16x3] [--candidates KC]

Shapes:  a  Mx = 8192, Ny = 2^20, P = 512, k = 10
         b  Mx = 64,   Ny = 2^22, P = 512, k = 10
         c  P = 120 at the sizes of a (the notebook's RNA width)
         d  a with k = 64 and an ascending gallery: every score beats the current k-th and inserts
Baseline (same process): ops.sim_logits over gallery chunks, torch.topk per chunk, torch.topk over the chunk winners.
Time: device events around the call after warm-up, the median of --iters.  FLOPs = 2 Mx Ny P against the 157.3 TFLOP/s
f32 matrix peak; gallery bytes against 8 TB/s; the larger of the two floors names the bound.
--prefilter bf16 / bf16x3 (one line per shape and mode): searches on a prefiltered EmbeddingIndex (its planes built
before timing) against the exact fused top-k of the same process, the certified fraction, and the functional
retrieval.topk (which also splits the gallery each call).  Shape d runs at k = 63 there (a prefilter takes k <= 63)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_dplm_amd import ops, retrieval  # noqa: E402

F32_PEAK = 157.3e12
HBM = 8e12
SHAPES = {
    "a": dict(Mx=8192, Ny=1 << 20, P=512, k=10, adversarial=False),
    "b": dict(Mx=64, Ny=1 << 22, P=512, k=10, adversarial=False),
    "c": dict(Mx=8192, Ny=1 << 20, P=120, k=10, adversarial=False),
    "d": dict(Mx=8192, Ny=1 << 20, P=512, k=64, adversarial=True),
}


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms)


def inputs(Mx, Ny, P, adversarial, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    if adversarial:
        y = 0.01 * torch.randn(Ny, P, device=dev, generator=g)
        y[:, 0] = torch.arange(1, Ny + 1, device=dev, dtype=torch.float32) / Ny       # ascending, distinct
        x = torch.zeros(Mx, P, device=dev)
        x[:, 0] = 1.0
        return x, y
    x = torch.randn(Mx, P, device=dev, generator=g)
    y = torch.randn(Ny, P, device=dev, generator=g)
    return x / x.norm(dim=1, keepdim=True), y / y.norm(dim=1, keepdim=True)


def baseline_topk(x, y, k, scale_dev, chunk):
    vals, idxs = [], []
    for j0 in range(0, y.shape[0], chunk):
        S = ops.sim_logits(x, y[j0:j0 + chunk], scale_dev)
        v, i = torch.topk(S, k, dim=1)
        vals.append(v)
        idxs.append(i + j0)
        del S
    v, pos = torch.topk(torch.cat(vals, 1), k, dim=1)
    return v, torch.cat(idxs, 1).gather(1, pos)


def run(name, cfg, iters, warmup, dev):
    Mx, Ny, P, k = cfg["Mx"], cfg["Ny"], cfg["P"], cfg["k"]
    x, y = inputs(Mx, Ny, P, cfg["adversarial"], dev)
    scale_dev = torch.ones(1, device=dev)
    flops = 2.0 * Mx * Ny * P
    gbytes = 4.0 * Ny * P
    t_fused = timed(lambda: ops.sim_topk(x, y, k), iters, warmup)
    s, i = ops.sim_topk(x, y, k)
    chunk = max(4096, min(Ny, (1 << 29) // Mx))                       # <= 2 GiB of logits per chunk
    t_base = timed(lambda: baseline_topk(x, y, k, scale_dev, chunk), max(1, iters // 2), 1)
    bs, bi = baseline_topk(x, y, k, scale_dev, chunk)
    labels = i[:, 0].contiguous()
    t_rank = timed(lambda: ops.sim_rank(x, y, labels=labels), iters, warmup)
    r, _ = ops.sim_rank(x, y, labels=labels)
    floor_c, floor_m = flops / F32_PEAK * 1e3, gbytes / HBM * 1e3
    out = {
        "shape": name, "Mx": Mx, "Ny": Ny, "P": P, "k": k, "adversarial": cfg["adversarial"],
        "topk_ms": round(t_fused, 4), "rank_ms": round(t_rank, 4), "baseline_ms": round(t_base, 4),
        "speedup_vs_baseline": round(t_base / t_fused, 3),
        "flops": flops, "topk_tflops": round(flops / t_fused / 1e9, 2),
        "topk_f32_pipe_frac": round(floor_c / t_fused, 3), "rank_f32_pipe_frac": round(floor_c / t_rank, 3),
        "gallery_bytes": gbytes, "hbm_floor_ms": round(floor_m, 4), "compute_floor_ms": round(floor_c, 4),
        "bound": "f32 matrix pipe" if floor_c >= floor_m else "HBM",
        "top1_agrees_with_baseline": round(float((bi[:, 0] == i[:, 0]).float().mean()), 5),
        "max_score_diff_vs_baseline": float((bs - s).abs().max()),
        "rank_of_own_top1_is_zero": bool((r == 0).all()),
    }
    del x, y, s, i, bs, bi
    torch.cuda.empty_cache()
    return out


def run_prefilter(name, cfg, mode, candidates, iters, warmup, dev):
    Mx, Ny, P = cfg["Mx"], cfg["Ny"], cfg["P"]
    k = min(cfg["k"], 63)
    x, y = inputs(Mx, Ny, P, cfg["adversarial"], dev)
    t_exact = timed(lambda: ops.sim_topk(x, y, k), iters, warmup)
    s0, i0 = ops.sim_topk(x, y, k)
    idx = retrieval.EmbeddingIndex(P, dev, prefilter=mode)
    idx.add(y)
    t_index = timed(lambda: idx.search(x, k, candidates=candidates), iters, warmup)
    s1, i1, st = idx.search(x, k, candidates=candidates, return_stats=True)
    t_func = timed(lambda: retrieval.topk(x, y, k, prefilter=mode, candidates=candidates), max(1, iters // 2), 1)
    out = {
        "shape": name, "Mx": Mx, "Ny": Ny, "P": P, "k": k, "adversarial": cfg["adversarial"], "prefilter": mode,
        "candidates": st["candidates"], "index_search_ms": round(t_index, 4), "exact_topk_ms": round(t_exact, 4),
        "speedup_vs_exact": round(t_exact / t_index, 3), "certified_frac": round(st["certified"] / st["queries"], 5),
        "functional_topk_ms": round(t_func, 4), "equal_to_exact": bool(torch.equal(s0, s1) and torch.equal(i0, i1)),
    }
    del x, y, idx, s0, i0, s1, i1
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,d")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--prefilter", default="none", help="comma list of none, bf16, bf16x3")
    ap.add_argument("--candidates", type=int, default=None, help="prefilter candidates per query (default: the API's)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in a.shapes.split(","):
        for mode in a.prefilter.split(","):
            if mode == "none":
                res = run(name, SHAPES[name], a.iters, a.warmup, dev)
            else:
                res = run_prefilter(name, SHAPES[name], mode, a.candidates, a.iters, a.warmup, dev)
            line = json.dumps(res)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
