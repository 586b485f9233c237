"""Fused Sinkhorn optimal transport (clipk_sim_lse_bias, clipk_sinkhorn_apply; clip_dplm_amd.ot) against the same
algorithm on the materialised matrix, one JSON line per shape.

  python3 tools/bench_sinkhorn.py [--shapes s,m,l] [--iters 5] [--warmup 2] [--div-iters 3] [--div-warmup 1]
                                  [--baseline-iters 1] [--out profiles/sinkhorn/bench_sinkhorn.jsonl]

Shapes:  s  M = N = 1024,  P = 128
         m  M = N = 8192,  P = 512
         l  M = N = 65536, P = 512      (the matrix alone is 16 GiB in f32)
Measured, in the same process, the fused calls alternating within every iteration:
  half        one ops.sim_lse_bias call (u update with the key-side bias, no error scalar)
  simce_lse   ops.simce_lse at the same shape: the same matrix work without the bias, the yardstick for `half`
  iteration   one Sinkhorn iteration = the u and the v half-iterations, back to back
  divergence  ot.sinkhorn_divergence forward (50 iterations, tol=None) and backward, inputs of both clouds requiring grad
  torch_*     the same iteration / divergence in torch with S = (2 / eps) x y^T materialised once per problem (row
              chunks of at most 2 GiB where the logsumexp temporaries would not fit); --baseline-iters of it (it is slow)
Time: device events around each call after warm-up, the median of --iters.  FLOPs of a half-iteration = 2 M N P against
the 157.3 TFLOP/s f32 matrix peak."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_dplm_amd import ops, ot  # noqa: E402

F32_PEAK = 157.3e12
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


def inputs(M, N, P, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(M, P, device=dev, generator=g)
    y = torch.randn(N, P, device=dev, generator=g)
    y[:, 0] += 0.3 * math.sqrt(P)
    return x / x.norm(dim=1, keepdim=True), y / y.norm(dim=1, keepdim=True)


def lse_rows(S, bias, chunk):
    """logsumexp_j (S_ij + bias_j) per row, `chunk` rows at a time (the sum S + bias is a temporary of the chunk's size)."""
    return torch.cat([torch.logsumexp(S[i:i + chunk] + bias[None, :], dim=1) for i in range(0, S.shape[0], chunk)])


def lse_cols(S, bias, chunk):
    """logsumexp_i (S_ij + bias_i) per column, accumulated over row chunks."""
    out = torch.full((S.shape[1],), float("-inf"), device=S.device)
    for i in range(0, S.shape[0], chunk):
        out = torch.logaddexp(out, torch.logsumexp(S[i:i + chunk] + bias[i:i + chunk, None], dim=0))
    return out


def torch_solve(x, y, eps, n_iters, symmetric, chunk):
    """The iteration of ot.sinkhorn on the materialised matrix; returns (value, u, v, S)."""
    M, N = x.shape[0], y.shape[0]
    S = (2.0 / eps) * (x @ y.T)
    loga = torch.full((M,), -math.log(M), device=x.device)
    logb = torch.full((N,), -math.log(N), device=x.device)
    if symmetric:
        u = loga
        for _ in range(n_iters):
            u = 0.5 * (u + loga - lse_rows(S, u, chunk))
        v = u
    else:
        v = logb
        for _ in range(n_iters):
            u = loga - lse_rows(S, v, chunk)
            v = logb - lse_cols(S, u, chunk)
    f, g = eps * (u - loga) + (x * x).sum(1), eps * (v - logb) + (y * y).sum(1)
    return f.mean() + g.mean(), u, v, S


def torch_row_gradient(x, y, S, u, v, chunk, transpose=False):
    """2 (r_i x_i - sum_j P_ij y_j) from the materialised S (its transpose for the key side), in row chunks."""
    out = torch.empty_like(x)
    for i in range(0, x.shape[0], chunk):
        s = S[:, i:i + chunk].T if transpose else S[i:i + chunk]
        p = (s + u[i:i + chunk, None] + v[None, :]).exp()
        out[i:i + chunk] = 2.0 * (p.sum(1)[:, None] * x[i:i + chunk] - p @ y)
    return out


def torch_divergence(x, y, eps, n_iters, chunk):
    """Forward and both gradients of the debiased divergence, the three matrices materialised one after another."""
    v_xy, u, v, S = torch_solve(x, y, eps, n_iters, False, chunk)
    gx = torch_row_gradient(x, y, S, u, v, chunk)
    gy = torch_row_gradient(y, x, S, v, u, chunk, transpose=True)
    del S
    v_xx, uu, _, S = torch_solve(x, x, eps, n_iters, True, chunk)
    gx -= torch_row_gradient(x, x, S, uu, uu, chunk)
    del S
    v_yy, uu, _, S = torch_solve(y, y, eps, n_iters, True, chunk)
    gy -= torch_row_gradient(y, y, S, uu, uu, chunk)
    del S
    return v_xy - 0.5 * v_xx - 0.5 * v_yy, gx, gy


def run(name, cfg, iters, warmup, base_iters, div_iters, div_warmup, dev):
    M, N, P = cfg["M"], cfg["N"], cfg["P"]
    x, y = inputs(M, N, P, dev)
    scale = torch.full((1,), 2.0 / EPS, device=dev)
    loga = torch.full((M,), -math.log(M), device=dev)
    logb = torch.full((N,), -math.log(N), device=dev)
    u, v = torch.empty_like(loga), logb.clone()
    chunk = max(64, min(M, (1 << 29) // N))                        # <= 2 GiB of f32 per temporary
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)

    def half():
        ops.sim_lse_bias(x, y, scale, bias=v, logw=loga, out=u)

    def simce():
        ops.simce_lse(x, y, scale)

    def iteration():
        ops.sim_lse_bias(x, y, scale, bias=v, logw=loga, out=u)
        ops.sim_lse_bias(y, x, scale, bias=u, logw=logb, out=v)

    def divergence():
        xg.grad = yg.grad = None
        d = ot.sinkhorn_divergence(xg, yg, eps=EPS, n_iters=ITERS, tol=None)
        d.backward()
        return d

    S_holder = {}

    def torch_iteration():
        S = S_holder["S"]
        uu = loga - lse_rows(S, logb, chunk)
        return logb - lse_cols(S, uu, chunk)

    for _ in range(warmup):
        half(), simce(), iteration()
    for _ in range(div_warmup):
        divergence()
    t = {"half": [], "simce_lse": [], "iteration": [], "divergence": []}
    for _ in range(iters):                                          # alternating
        t["half"].append(once(half))
        t["simce_lse"].append(once(simce))
        t["iteration"].append(once(iteration))
    for _ in range(max(1, div_iters)):
        t["divergence"].append(once(lambda: S_holder.__setitem__("d", divergence())))
    med = {k: statistics.median(vals) for k, vals in t.items()}
    d = S_holder.pop("d")
    gx, gy = xg.grad.clone(), yg.grad.clone()
    out = {"shape": name, "M": M, "N": N, "P": P, "eps": EPS, "divergence_iters": ITERS}
    out.update({k + "_ms": round(val, 4) for k, val in med.items()})
    out.update({k + "_ms_all": [round(val, 4) for val in vals] for k, vals in t.items()})
    flops = 2.0 * M * N * P
    out["half_over_simce_lse"] = round(med["half"] / med["simce_lse"], 4)
    out["half_f32_pipe_frac"] = round(flops / F32_PEAK * 1e3 / med["half"], 3)
    out["simce_lse_f32_pipe_frac"] = round(flops / F32_PEAK * 1e3 / med["simce_lse"], 3)
    if base_iters > 0:
        S_holder["S"] = (2.0 / EPS) * (x @ y.T)
        t_it = [once(torch_iteration) for _ in range(base_iters + 1)][1:]
        S_holder.clear()
        torch.cuda.empty_cache()
        ref = torch_divergence(x, y, EPS, ITERS, chunk)               # warm-up, and the values to compare
        t_div = [once(lambda: torch_divergence(x, y, EPS, ITERS, chunk)) for _ in range(base_iters)]
        out["torch_iteration_ms"] = round(statistics.median(t_it), 4)
        out["torch_divergence_ms"] = round(statistics.median(t_div), 4)
        out["iteration_speedup_vs_torch"] = round(statistics.median(t_it) / med["iteration"], 3)
        out["divergence_speedup_vs_torch"] = round(statistics.median(t_div) / med["divergence"], 3)
        out["torch_chunk_rows"] = chunk
        out["divergence"] = float(d)
        out["divergence_diff_vs_torch"] = abs(float(d) - float(ref[0]))
        out["max_grad_diff_vs_torch"] = max(float((gx - ref[1]).abs().max()), float((gy - ref[2]).abs().max()))
        out["max_grad"] = float(gx.abs().max())
    del x, y, xg, yg
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="s,m,l")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-iters", type=int, default=1)
    ap.add_argument("--div-iters", type=int, default=3, help="timed runs of the fused divergence")
    ap.add_argument("--div-warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in a.shapes.split(","):
        line = json.dumps(run(name, SHAPES[name], a.iters, a.warmup, a.baseline_iters, a.div_iters, a.div_warmup, dev))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
