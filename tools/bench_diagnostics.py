"""Fused similarity statistics (clipk_sim_stats) against what it replaces, one JSON line per shape.

  python3 tools/bench_diagnostics.py [--shapes a,s,t] [--iters 5] [--warmup 2] [--out profiles/diagnostics/bench.jsonl]

Shapes:  a  Mx = 8192,  Ny = 2^20,  P = 512      (the retrieval gallery size)
         s  Mx = 16384, Ny = 16384, P = 512      (a validation set against itself)
         t  Mx = 16384, Ny = 16384, P = 128
Compared, in the same process and alternating within every iteration:
  stats     one ops.sim_stats pass (64 bins)
  three     the three fused passes it subsumes, back to back: ops.sim_topk (k = 1), ops.sim_rank, ops.simce_lse (tiled)
  rank      ops.sim_rank alone: the same tile walk with the cheapest epilogue, so stats / rank is the epilogue's price
  chunked   ops.sim_logits over gallery chunks (<= 2 GiB of logits) plus the torch reductions that give the same
            outputs (max / argmax, masked max, logsumexp, f64 sums, histc); --baseline-iters of it (it is slow)
Time: device events around each call after warm-up, the median of --iters.  FLOPs = 2 Mx Ny P against the 157.3 TFLOP/s
f32 matrix peak."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_dplm_amd import ops  # noqa: E402

F32_PEAK = 157.3e12
SHAPES = {
    "a": dict(Mx=8192, Ny=1 << 20, P=512),
    "s": dict(Mx=16384, Ny=16384, P=512),
    "t": dict(Mx=16384, Ny=16384, P=128),
}
SCALE, BINS = 14.2857, 64


def once(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def inputs(Mx, Ny, P, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(Mx, P, device=dev, generator=g)
    y = torch.randn(Ny, P, device=dev, generator=g)
    return x / x.norm(dim=1, keepdim=True), y / y.norm(dim=1, keepdim=True)


def chunked(x, y, scale_dev, chunk):
    """The outputs of sim_stats from materialised chunks (labels i -> i)."""
    Mx, dev = x.shape[0], x.device
    rows = torch.arange(Mx, device=dev)
    best = torch.full((Mx,), float("-inf"), device=dev)
    hard = best.clone()
    best_i = torch.full((Mx,), -1, dtype=torch.int64, device=dev)
    hard_i = best_i.clone()
    lse = best.clone()
    s1 = torch.zeros(Mx, dtype=torch.float64, device=dev)
    s2 = s1.clone()
    pos = torch.empty(Mx, device=dev)
    hist = torch.zeros(BINS, device=dev)
    for j0 in range(0, y.shape[0], chunk):
        S = ops.sim_logits(x, y[j0:j0 + chunk], scale_dev)
        c = S.shape[1]
        v, i = S.max(1)
        up = v > best
        best, best_i = torch.where(up, v, best), torch.where(up, i + j0, best_i)
        lse = torch.logaddexp(lse, torch.logsumexp(S, 1))
        inside = (rows >= j0) & (rows < j0 + c)
        r_in = rows[inside]
        if r_in.numel():
            pos[r_in] = S[r_in, r_in - j0]
        s1 += S.sum(1, dtype=torch.float64)
        s2 += (S * S).sum(1, dtype=torch.float64)
        hist += torch.histc(S, BINS, -SCALE, SCALE)
        if r_in.numel():
            S[r_in, r_in - j0] = float("-inf")
        v, i = S.max(1)
        up = v > hard
        hard, hard_i = torch.where(up, v, hard), torch.where(up, i + j0, hard_i)
        del S
    s1 -= pos.double()
    s2 -= pos.double() ** 2
    hist -= torch.histc(pos, BINS, -SCALE, SCALE)
    return pos, best, best_i, hard, hard_i, lse, s1, s2, hist


def run(name, cfg, iters, warmup, base_iters, dev):
    Mx, Ny, P = cfg["Mx"], cfg["Ny"], cfg["P"]
    x, y = inputs(Mx, Ny, P, dev)
    scale_dev = torch.full((1,), SCALE, device=dev)
    chunk = max(4096, min(Ny, (1 << 29) // Mx))

    def stats():
        return ops.sim_stats(x, y, scale=SCALE, nbins=BINS)

    def three():
        ops.sim_topk(x, y, 1, scale=SCALE)
        ops.sim_rank(x, y, scale=SCALE)
        ops.simce_lse(x, y, scale_dev)

    def rank():
        ops.sim_rank(x, y, scale=SCALE)

    for _ in range(warmup):
        stats(), three(), rank()
    t = {"stats": [], "three": [], "rank": []}
    for _ in range(iters):                                          # alternating
        t["stats"].append(once(stats))
        t["three"].append(once(three))
        t["rank"].append(once(rank))
    t_base = [once(lambda: chunked(x, y, scale_dev, chunk)) for _ in range(base_iters + 1)][1:]
    med = {k: statistics.median(v) for k, v in t.items()}
    st = stats()
    ref = chunked(x, y, scale_dev, chunk)
    flops = 2.0 * Mx * Ny * P
    out = {
        "shape": name, "Mx": Mx, "Ny": Ny, "P": P, "bins": BINS,
        "stats_ms": round(med["stats"], 4), "three_fused_ms": round(med["three"], 4), "rank_ms": round(med["rank"], 4),
        "chunked_ms": round(statistics.median(t_base), 4) if t_base else None,
        "stats_ms_all": [round(v, 4) for v in t["stats"]], "three_fused_ms_all": [round(v, 4) for v in t["three"]],
        "speedup_vs_three_fused": round(med["three"] / med["stats"], 3),
        "speedup_vs_chunked": round(statistics.median(t_base) / med["stats"], 3) if t_base else None,
        "stats_over_rank": round(med["stats"] / med["rank"], 3),
        "stats_f32_pipe_frac": round(flops / F32_PEAK * 1e3 / med["stats"], 3),
        "rank_f32_pipe_frac": round(flops / F32_PEAK * 1e3 / med["rank"], 3),
        "best_idx_agrees_with_chunked": round(float((st.best_idx == ref[2]).float().mean()), 5),
        "max_lse_diff_vs_chunked": float((st.lse - ref[5]).abs().max()),
        "max_rel_neg_sum_diff_vs_chunked": float(((st.neg_sum - ref[6]).abs() / ref[6].abs()).max()),
        "hist_total": int(st.hist_neg.sum()), "hist_outer": int(st.hist_neg[0] + st.hist_neg[-1]),
        "hist_max_slot_share": round(float(st.hist_neg.max()) / float(st.hist_neg.sum()), 4),
    }
    del x, y
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,s,t")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-iters", type=int, default=1)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in a.shapes.split(","):
        line = json.dumps(run(name, SHAPES[name], a.iters, a.warmup, a.baseline_iters, dev))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
