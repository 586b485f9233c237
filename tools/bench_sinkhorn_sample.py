"""Drawing from the entropic plan without the matrix (clipk_sim_sample; ops.sim_sample) against the Sinkhorn
half-iteration at the same shape and against torch on materialised logits, one JSON line per shape.

  python3 tools/bench_sinkhorn_sample.py [--shapes s,m,l] [--iters 7] [--warmup 2] [--baseline-iters 2]
                                         [--out profiles/sinkhorn_sample/bench_sinkhorn_sample.jsonl]

Shapes (those of tools/bench_sinkhorn.py):  s  M = N = 1024,  P = 128
                                            m  M = N = 8192,  P = 512
                                            l  M = N = 65536, P = 512      (the matrix alone is 16 GiB in f32)
Measured, in the same process, the two fused calls alternating within every iteration:
  sample      one ops.sim_sample call: one draw per row with the key-side bias, the seed in device memory
  half        one ops.sim_lse_bias call at the same shape with the same bias: the same tile walk with the (max, sum)
              epilogue; sample / half is the figure that matters
  torch       the same draw in torch, the logits materialised in row chunks of at most 2 GiB: scale * x y^T + bias,
              softmax, torch.multinomial(., 1); --baseline-iters of it
Time: device events around each call after warm-up, the median of --iters.  FLOPs of a pass = 2 M N P against the
157.3 TFLOP/s f32 matrix peak."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_dplm_amd import ops  # noqa: E402

F32_PEAK = 157.3e12
SHAPES = {
    "s": dict(M=1024, N=1024, P=128),
    "m": dict(M=8192, N=8192, P=512),
    "l": dict(M=65536, N=65536, P=512),
}
EPS = 0.5


def once(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def inputs(M, N, P, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(M, P, device=dev, generator=g)
    y = torch.randn(N, P, device=dev, generator=g)
    y[:, 0] += 0.3 * math.sqrt(P)
    return x / x.norm(dim=1, keepdim=True), y / y.norm(dim=1, keepdim=True)


def torch_sample(x, y, scale, bias, chunk):
    out = []
    for i in range(0, x.shape[0], chunk):
        s = scale * (x[i:i + chunk] @ y.T) + bias[None, :]
        out.append(torch.multinomial(torch.softmax(s, dim=1), 1)[:, 0])
    return torch.cat(out)


def run(name, cfg, iters, warmup, base_iters, dev):
    M, N, P = cfg["M"], cfg["N"], cfg["P"]
    x, y = inputs(M, N, P, dev)
    scale = torch.full((1,), 2.0 / EPS, device=dev)
    loga = torch.full((M,), -math.log(M), device=dev)
    logb = torch.full((N,), -math.log(N), device=dev)
    u = torch.empty_like(loga)
    v = logb.clone()
    for _ in range(3):                                              # a few iterations: a bias of the solver's kind
        ops.sim_lse_bias(x, y, scale, bias=v, logw=loga, out=u)
        ops.sim_lse_bias(y, x, scale, bias=u, logw=logb, out=v)
    seed = torch.tensor([1, 0], dtype=torch.int64, device=dev)
    chunk = max(64, min(M, (1 << 29) // N))                         # <= 2 GiB of f32 per temporary

    def sample():
        return ops.sim_sample(x, y, scale, bias=v, seed=seed)

    def half():
        ops.sim_lse_bias(x, y, scale, bias=v, logw=loga, out=u)

    for _ in range(warmup):
        sample(), half()
    t = {"sample": [], "half": []}
    for _ in range(iters):                                           # alternating
        t["sample"].append(once(sample))
        t["half"].append(once(half))
    med = {k: statistics.median(vals) for k, vals in t.items()}
    out = {"shape": name, "M": M, "N": N, "P": P, "eps": EPS}
    out.update({k + "_ms": round(val, 4) for k, val in med.items()})
    out.update({k + "_ms_all": [round(val, 4) for val in vals] for k, vals in t.items()})
    flops = 2.0 * M * N * P
    out["sample_over_half"] = round(med["sample"] / med["half"], 4)
    out["sample_f32_pipe_frac"] = round(flops / F32_PEAK * 1e3 / med["sample"], 3)
    out["half_f32_pipe_frac"] = round(flops / F32_PEAK * 1e3 / med["half"], 3)
    if base_iters > 0:
        sc = float(scale)
        torch_sample(x, y, sc, v, chunk)                              # warm-up
        t_t = [once(lambda: torch_sample(x, y, sc, v, chunk)) for _ in range(base_iters)]
        out["torch_ms"] = round(statistics.median(t_t), 4)
        out["torch_ms_all"] = [round(val, 4) for val in t_t]
        out["speedup_vs_torch"] = round(statistics.median(t_t) / med["sample"], 3)
        out["torch_chunk_rows"] = chunk
    del x, y
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="s,m,l")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-iters", type=int, default=2)
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
