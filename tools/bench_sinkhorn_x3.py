"""The bf16x3 Sinkhorn half-iteration (clipk_sim_lse_bias_x3) and ot.sinkhorn(..., precision="bf16x3") against the exact
f32 path of the same library, one JSON line per shape.

  python3 tools/bench_sinkhorn_x3.py [--shapes s,m,l] [--iters 7] [--warmup 2] [--solve-iters 3] [--solve-warmup 1]
                                     [--out profiles/sinkhorn_x3/bench_sinkhorn_x3.jsonl]

Shapes:  s  M = N = 1024,  P = 128
         m  M = N = 8192,  P = 512
         l  M = N = 65536, P = 512
Measured in one process, the two precisions alternating within every iteration (other work shares the machine: a
difference is judged against the spread of the alternating samples, which is recorded):
  half_f32 / half_x3    one ops.sim_lse_bias / ops.sim_lse_bias_x3 call (u update with the key-side bias, no error
                        scalar); the planes of half_x3 are split beforehand, as a solve splits them once
  split                 the two ops.split_bf16 launches of a solve (both clouds), on their own
  solve_f32 / solve_x3  ot.sinkhorn(n_iters=50, tol=None) in both precisions; the split launches, the exact last
                        iteration and the exact error pass are inside solve_x3's timed region
Time: device events around each call after warm-up; median, minimum and maximum of the samples.  The deviation of the
split half-iteration from the f32 one is recorded next to the logit error bound eta that covers it."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_dplm_amd import ops, ot, retrieval  # noqa: E402

F32_PEAK = 157.3e12
BF16_PEAK = 16 * F32_PEAK             # the f32 MFMA rate is 1/16 of the bf16 rate
SHAPES = {
    "s": dict(M=1024, N=1024, P=128),
    "m": dict(M=8192, N=8192, P=512),
    "l": dict(M=65536, N=65536, P=512),
}
EPS, ITERS = 0.5, 50


def once(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def stats(ts):
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts), samples=len(ts))


def inputs(M, N, P, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(M, P, device=dev, generator=g)
    y = torch.randn(N, P, device=dev, generator=g)
    y[:, 0] += 0.3 * math.sqrt(P)
    return x / x.norm(dim=1, keepdim=True), y / y.norm(dim=1, keepdim=True)


def planes(t):
    hi = torch.empty((t.shape[0], ops.plane_pitch(t.shape[1])), dtype=torch.bfloat16, device=t.device)
    return hi, torch.empty_like(hi)


def run(name, cfg, iters, warmup, solve_iters, solve_warmup, dev):
    M, N, P = cfg["M"], cfg["N"], cfg["P"]
    x, y = inputs(M, N, P, dev)
    scale = torch.full((1,), 2.0 / EPS, device=dev)
    loga = torch.full((M,), -math.log(M), device=dev)
    v = torch.full((N,), -math.log(N), device=dev)
    (xh, xl), (yh, yl) = planes(x), planes(y)
    norm = torch.zeros(1, device=dev)

    def split():
        ops.split_bf16(x, xh, xl, norm)
        ops.split_bf16(y, yh, yl, norm)

    split()
    u32, u3 = torch.empty_like(loga), torch.empty_like(loga)
    half_f32 = lambda: ops.sim_lse_bias(x, y, scale, bias=v, logw=loga, out=u32)                     # noqa: E731
    half_x3 = lambda: ops.sim_lse_bias_x3(xh, xl, yh, yl, P, scale, bias=v, logw=loga, out=u3)      # noqa: E731
    t = {"half_f32": [], "half_x3": [], "split": [], "solve_f32": [], "solve_x3": []}
    for i in range(warmup + iters):
        for key, fn in (("half_f32", half_f32), ("half_x3", half_x3), ("split", split)):
            ms = once(fn)
            if i >= warmup:
                t[key].append(ms)
    dev_max = float((u3.double() - u32.double()).abs().max())
    eta = 2.0 / EPS * retrieval.prefilter_eps_rel(P, "bf16x3")            # unit rows: |x| = |y| = 1
    res = {}
    for i in range(solve_warmup + solve_iters):
        for key, prec in (("solve_f32", "f32"), ("solve_x3", "bf16x3")):
            ms = once(lambda: res.__setitem__(key, ot.sinkhorn(x, y, eps=EPS, n_iters=ITERS, tol=None, precision=prec)))
            if i >= solve_warmup:
                t[key].append(ms)
    r32, r3 = res["solve_f32"], res["solve_x3"]
    out = {"shape": name, "M": M, "N": N, "P": P, "eps": EPS, "n_iters": ITERS,
           "grid_f32": ops.sim_lse_bias_plan(M, N), "grid_x3": ops.sim_lse_bias_x3_plan(M, N)}
    out.update({k: stats(ts) for k, ts in t.items()})
    hf, hx = out["half_f32"]["median_ms"], out["half_x3"]["median_ms"]
    sf, sx = out["solve_f32"]["median_ms"], out["solve_x3"]["median_ms"]
    out["half_speedup_x3_over_f32"] = hf / hx
    out["solve_speedup_x3_over_f32"] = sf / sx
    out["half_f32_share_of_f32_peak"] = 2.0 * M * N * P / (hf * 1e-3) / F32_PEAK
    out["half_x3_share_of_bf16_peak"] = 6.0 * M * N * ops.plane_pitch(P) / (hx * 1e-3) / BF16_PEAK
    out["half_deviation_max"] = dev_max
    out["logit_error_bound"] = float(r3.logit_error_bound)
    out["logit_error_bound_restated"] = eta
    out["solve_value_f32"], out["solve_value_x3"] = float(r32.value), float(r3.value)
    out["solve_marginal_error_f32"], out["solve_marginal_error_x3"] = float(r32.marginal_error), float(r3.marginal_error)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="s,m,l")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--solve-iters", type=int, default=3)
    ap.add_argument("--solve-warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sinkhorn_x3 needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    lines = []
    for name in a.shapes.split(","):
        rec = run(name, SHAPES[name], a.iters, a.warmup, a.solve_iters, a.solve_warmup, dev)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
