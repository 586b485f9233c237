"""Fused multi-bandwidth MMD (clipk_kernel_sums; clip_dplm_amd.distribution.mmd2) against the two ways to the same number
without it, one JSON line per shape.

  python3 tools/bench_mmd.py [--shapes s,m,l] [--iters 7] [--warmup 2] [--baseline-iters 3]
                             [--out profiles/mmd/bench_mmd.jsonl]

Shapes:  s  M = N = 1024,  P = 128
         m  M = N = 8192,  P = 512
         l  M = N = 16384, P = 128
B = 5 bandwidths (the default multipliers over the closed-form mean cost, computed once and handed over as a device
tensor), weights 1 / 5, the unbiased estimator.  Measured, in the same process, the fused call and baseline (a)
alternating within every iteration:
  fused_value        one distribution.mmd2 call without gradients: three clipk_kernel_sums launches
  fused_grad         the value and both gradients: forward + backward, seven launches
  apply_value/_grad  (a) the same quantities from B single-bandwidth ops.sinkhorn_apply calls per block (scale = 2 gamma,
                     u = -gamma |x|^2, v = -gamma |y|^2): the path that exists without the kernel, B tile walks per block;
                     the diagonal of a self block is taken off as M x the weight (its computed d2_ii is not exactly 0)
  torch_value/_grad  (b) torch on the materialised matrix: torch.cdist squared, the B exponentials, the means, autograd
                     for the gradients; row chunks of at most 2 GiB per temporary where the matrix would not fit
Time: device events around `inner` back-to-back calls after warm-up (so that a timed window is milliseconds, not one
launch), divided by inner; the median of --iters.  Every timed value is in the record."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_dplm_amd import distribution, ops, ot  # noqa: E402

SHAPES = {
    "s": dict(M=1024, N=1024, P=128, inner=20),
    "m": dict(M=8192, N=8192, P=512, inner=2),
    "l": dict(M=16384, N=16384, P=128, inner=2),
}
MULTIPLIERS = distribution.DEFAULT_MULTIPLIERS


def timed(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / inner


def inputs(M, N, P, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(M, P, device=dev, generator=g)
    y = torch.randn(N, P, device=dev, generator=g)
    y[:, 0] += 0.3 * math.sqrt(P)
    return x / x.norm(dim=1, keepdim=True), y / y.norm(dim=1, keepdim=True)


# ---------------------------------------------------------------------------------------- (a) B sinkhorn_apply calls per block
class ApplyMMD:
    """mmd2 and its gradients from single-bandwidth plan sums: exp(-gamma d2) = exp(2 gamma <x, y> - gamma nx - gamma ny)."""

    def __init__(self, x, y, gammas, weights):
        self.x, self.y, self.w = x, y, weights
        self.nx, self.ny = (x * x).sum(1), (y * y).sum(1)
        self.scales = [(2.0 * g).reshape(1) for g in gammas]
        self.u = [-g * self.nx for g in gammas]
        self.v = [-g * self.ny for g in gammas]
        self.wg = [w * g for w, g in zip(weights, gammas)]

    def _block(self, a, b, pa, pb, coef, bary):
        """sum_b coef[b] x (row sums, key-weighted sums) of one block, B launches."""
        mass = m = None
        for k, c in enumerate(coef):
            r, bb, _ = ops.sinkhorn_apply(a, b, self.scales[k], pa[k], pb[k], want_bary=bary, want_cost=False)
            mass = c * r if mass is None else mass + c * r
            if bary:
                m = c * bb if m is None else m + c * bb
        return mass, m

    def value(self):
        x, y = self.x, self.y
        M, N = len(x), len(y)
        wsum = sum(self.w)
        sxx = self._block(x, x, self.u, self.u, self.w, False)[0].sum(dtype=torch.float64) - M * wsum
        syy = self._block(y, y, self.v, self.v, self.w, False)[0].sum(dtype=torch.float64) - N * wsum
        sxy = self._block(x, y, self.u, self.v, self.w, False)[0].sum(dtype=torch.float64)
        return (sxx / (M * (M - 1)) + syy / (N * (N - 1)) - 2.0 * sxy / (M * N)).float()

    def _row_gradient(self, a, b, pa, pb):
        g, m = self._block(a, b, pa, pb, self.wg, True)
        return -2.0 * (g[:, None] * a - m)

    def value_and_grads(self):
        x, y = self.x, self.y
        M, N = len(x), len(y)
        gx = self._row_gradient(x, x, self.u, self.u) * (2.0 / (M * (M - 1))) - self._row_gradient(x, y, self.u, self.v) * (2.0 / (M * N))
        gy = self._row_gradient(y, y, self.v, self.v) * (2.0 / (N * (N - 1))) - self._row_gradient(y, x, self.v, self.u) * (2.0 / (M * N))
        return self.value(), gx, gy


# ---------------------------------------------------------------------------------------- (b) torch on the matrix
def torch_mmd2(x, y, gammas, weights, chunk, grad):
    """The unbiased estimator on materialised row chunks; with grad the chunks' backward passes accumulate into x.grad
    and y.grad.  Returns the value (0-d, detached)."""
    M, N = len(x), len(y)
    total = torch.zeros((), dtype=torch.float64, device=x.device)
    for a, b, norm, self_block in ((x, x, M * (M - 1), True), (y, y, N * (N - 1), True), (x, y, -0.5 * M * N, False)):
        for i in range(0, len(a), chunk):
            d2 = torch.cdist(a[i:i + chunk], b) ** 2
            k = sum(w * torch.exp(-g * d2) for g, w in zip(gammas, weights))
            part = k.sum(dtype=torch.float64)
            if self_block:
                part = part - k.diagonal(offset=i).sum(dtype=torch.float64)
            part = part / norm
            if grad:
                part.backward()
            total += part.detach()
    return total.float()


def run(name, cfg, iters, warmup, base_iters, dev):
    M, N, P, inner = cfg["M"], cfg["N"], cfg["P"], cfg["inner"]
    x, y = inputs(M, N, P, dev)
    B = len(MULTIPLIERS)
    gammas = (1.0 / (torch.tensor(MULTIPLIERS, device=dev) * ot.mean_cost(x, y))).contiguous()
    weights = torch.full((B,), 1.0 / B, device=dev)
    glist, wlist = list(gammas.unbind()), [1.0 / B] * B
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    apply_path = ApplyMMD(x, y, glist, wlist)
    chunk = max(64, min(max(M, N), (1 << 29) // max(M, N)))          # <= 2 GiB of f32 per temporary

    def fused_value():
        with torch.no_grad():
            return distribution.mmd2(x, y, gammas=gammas, weights=weights)

    def fused_grad():
        xg.grad = yg.grad = None
        v = distribution.mmd2(xg, yg, gammas=gammas, weights=weights)
        v.backward()
        return v

    def torch_value():
        with torch.no_grad():
            return torch_mmd2(x, y, glist, wlist, chunk, False)

    def torch_grad():
        xg.grad = yg.grad = None
        return torch_mmd2(xg, yg, glist, wlist, chunk, True)

    calls = {"fused_value": fused_value, "apply_value": apply_path.value, "fused_grad": fused_grad,
             "apply_grad": apply_path.value_and_grads}
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    t = {k: [] for k in calls}
    for _ in range(iters):                                            # alternating
        for k, fn in calls.items():
            t[k].append(timed(fn, inner))
    med = {k: statistics.median(v) for k, v in t.items()}
    out = {"shape": name, "M": M, "N": N, "P": P, "B": B, "inner": inner}
    out.update({k + "_ms": round(v, 4) for k, v in med.items()})
    out.update({k + "_ms_all": [round(v, 4) for v in vals] for k, vals in t.items()})
    out["value_speedup_vs_apply"] = round(med["apply_value"] / med["fused_value"], 3)
    out["grad_speedup_vs_apply"] = round(med["apply_grad"] / med["fused_grad"], 3)
    # the three block launches of the value: 2 M N P FLOPs each against the 157.3 TFLOP/s f32 matrix peak
    out["fused_value_f32_pipe_frac"] = round(2.0 * (M * M + N * N + M * N) * P / 157.3e12 * 1e3 / med["fused_value"], 3)
    # agreement of the three paths on these inputs
    v_f = fused_grad().detach()
    gx_f, gy_f = xg.grad.clone(), yg.grad.clone()
    v_a, gx_a, gy_a = apply_path.value_and_grads()
    out["value"] = float(v_f)
    out["value_diff_vs_apply"] = abs(float(v_f) - float(v_a))
    out["max_grad"] = float(gx_f.abs().max())
    out["max_grad_diff_vs_apply"] = max(float((gx_f - gx_a).abs().max()), float((gy_f - gy_a).abs().max()))
    if base_iters > 0:
        torch_value(), torch_grad()                                   # warm-up
        tv = [timed(torch_value, 1) for _ in range(base_iters)]
        tg = [timed(torch_grad, 1) for _ in range(base_iters)]
        v_t = torch_grad()
        out["torch_value_ms"], out["torch_grad_ms"] = round(statistics.median(tv), 4), round(statistics.median(tg), 4)
        out["torch_value_ms_all"], out["torch_grad_ms_all"] = [round(v, 4) for v in tv], [round(v, 4) for v in tg]
        out["value_speedup_vs_torch"] = round(statistics.median(tv) / med["fused_value"], 3)
        out["grad_speedup_vs_torch"] = round(statistics.median(tg) / med["fused_grad"], 3)
        out["torch_chunk_rows"] = chunk
        out["value_diff_vs_torch"] = abs(float(v_f) - float(v_t))
        out["max_grad_diff_vs_torch"] = max(float((gx_f - xg.grad).abs().max()), float((gy_f - yg.grad).abs().max()))
    del x, y, xg, yg
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="s,m,l")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-iters", type=int, default=3, help="timed runs of the torch baseline (0: skip it)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mmd.py measures on the GPU: no device found")
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
