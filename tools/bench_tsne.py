"""Exact t-SNE on the device (clipk_cond_entropy_sums, clipk_tsne_grad, clipk_tsne_update; clip_dplm_amd.manifold.tsne)
against the walk it is modelled on and against torch on the materialised matrix, one JSON line per shape.

  python3 tools/bench_tsne.py [--shapes s,m,l,xl] [--iters 7] [--warmup 2] [--baseline-iters 3] [--n-iter 1000]
                              [--sklearn] [--out profiles/tsne/bench_tsne.jsonl]

Shapes:  s  N = 1024,  P = 128        m  N = 8192,  P = 512
         l  N = 16384, P = 128        xl N = 65536, P = 512
The cloud: 16 Gaussian blobs (centres N(0, 1), points at 0.5 sigma), perplexity 30.  Measured, in the same process, the
walks alternating within every iteration:
  grad_walk          one ops.tsne_grad call (record packing, walk, split finalize) at a map of scale 1
  grad_walk_kl       the same with the KL row sum
  update             one ops.tsne_update call (the one-workgroup tail and the elementwise step)
  calib_walk         one ops.cond_entropy_sums call with B = 8 candidates per row
  lse_half           ops.sim_lse_bias of the cloud with itself: a Sinkhorn half-iteration, the walk of this structure
                     with the smallest epilogue - the floor
  full               manifold.tsne with --n-iter iterations from a random init, calibration included: host clock around
                     the call and a device synchronise, once, after a 2-iteration warm-up call
  torch_grad/_calib  the same gradient / the same eight candidate sums from the materialised N x N matrices (f32, matrix
                     products for the row sums), where they fit (N <= 16384)
  sklearn_*          with --sklearn and the library importable: TSNE(method="exact") at s and m, method="barnes_hut" at
                     every shape, on the host, once each
Time: device events around `inner` back-to-back calls after warm-up, divided by inner; the median of --iters.  Every
timed value is in the record."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_dplm_amd import manifold, ops  # noqa: E402

SHAPES = {
    "s": dict(N=1024, P=128, inner=20),
    "m": dict(N=8192, P=512, inner=4),
    "l": dict(N=16384, P=128, inner=4),
    "xl": dict(N=65536, P=512, inner=1),
}
PERPLEXITY = 30.0
TORCH_MAX_N = 16384


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
    centres = torch.randn(16, P, device=dev, generator=g)
    x = centres[torch.arange(N, device=dev) % 16] + 0.5 * torch.randn(N, P, device=dev, generator=g)
    return x.contiguous(), torch.randn(N, 2, device=dev, generator=g)


def torch_matrices(x, beta, dmin, log_s0):
    """(d, P) materialised in f32."""
    nx = (x * x).sum(1)
    d = (nx[:, None] + nx[None, :] - 2.0 * x @ x.T).clamp_min_(0)
    p = torch.exp(-beta[:, None] * (d - dmin[:, None]) - log_s0[:, None])
    p.fill_diagonal_(0)
    return d, (p + p.T) / (2.0 * len(x))


def torch_grad(Pm, y, alpha):
    """The gradient from the materialised P: the row sums as matrix products, sum_j A_ij (y_i - y_j) = rowsum(A) y - A y."""
    w = 1.0 / (1.0 + torch.cdist(y, y) ** 2)
    w.fill_diagonal_(0)
    pw, w2 = Pm * w, w * w
    attr = pw.sum(1, keepdim=True) * y - pw @ y
    rep = w2.sum(1, keepdim=True) * y - w2 @ y
    return 4.0 * (alpha * attr - rep / w.sum())


def torch_calib(d, betas, dmin):
    """s0, s1 [N, 8] from the materialised d, one candidate at a time."""
    t = d - dmin[:, None]
    s0, s1 = [], []
    for b in range(betas.shape[1]):
        e = torch.exp(-betas[:, b:b + 1] * t)
        e.fill_diagonal_(0)
        s0.append(e.sum(1))
        s1.append((t * e).sum(1))
    return torch.stack(s0, 1), torch.stack(s1, 1)


def sklearn_times(x, shape, n_iter):
    try:
        from sklearn.manifold import TSNE
    except ImportError:
        return {"sklearn": "not importable"}
    out, xh = {}, x.cpu().numpy()
    methods = (("exact", "barnes_hut") if shape in ("s", "m") else ("barnes_hut",))
    for method in methods:
        t0 = time.perf_counter()
        res = TSNE(n_components=2, perplexity=PERPLEXITY, method=method, max_iter=n_iter, init="random", random_state=0).fit(xh)
        out[f"sklearn_{method}_s"] = round(time.perf_counter() - t0, 3)
        out[f"sklearn_{method}_kl"] = float(res.kl_divergence_)
    return out


def run(name, cfg, a, dev):
    N, P, inner = cfg["N"], cfg["P"], cfg["inner"]
    x, y = inputs(N, P, dev)
    nx = (x * x).sum(1)
    beta, dmin, log_s0, entropy = manifold.perplexity_bandwidths(x, PERPLEXITY)
    betas = (beta[:, None] * torch.exp2(torch.linspace(-2.0, 2.0, 8, device=dev))[None, :]).contiguous()
    scale = torch.ones(1, device=dev)
    rows = ops.tsne_grad(x, y, beta, dmin, log_s0, nx=nx)
    ys, upd, gains = y.clone(), torch.zeros_like(y), torch.ones_like(y)
    calls = {
        "grad_walk": lambda: ops.tsne_grad(x, y, beta, dmin, log_s0, nx=nx),
        "lse_half": lambda: ops.sim_lse_bias(x, x, scale),
        "calib_walk": lambda: ops.cond_entropy_sums(x, betas, shift=dmin, nx=nx),
        "grad_walk_kl": lambda: ops.tsne_grad(x, y, beta, dmin, log_s0, nx=nx, want_kl=True),
        "update": lambda: ops.tsne_update(rows, ys, upd, gains, alpha=1.0, momentum=0.8, lr=1e-6),
    }
    for _ in range(a.warmup):
        for fn in calls.values():
            fn()
    t = {k: [] for k in calls}
    for _ in range(a.iters):                                          # alternating
        for k, fn in calls.items():
            t[k].append(timed(fn, inner))
    med = {k: statistics.median(v) for k, v in t.items()}
    nqb, ks = ops.tsne_grad_plan(N)
    out = {"shape": name, "N": N, "P": P, "perplexity": PERPLEXITY, "inner": inner, "grid": [nqb, ks],
           "entropy_err_max": float((entropy - torch.log(torch.tensor(PERPLEXITY))).abs().max())}
    out.update({k + "_ms": round(v, 4) for k, v in med.items()})
    out.update({k + "_ms_all": [round(v, 4) for v in vals] for k, vals in t.items()})
    out["grad_walk_over_lse_half"] = round(med["grad_walk"] / med["lse_half"], 3)
    out["calib_walk_over_lse_half"] = round(med["calib_walk"] / med["lse_half"], 3)
    # 2 N^2 P FLOPs of the product against the 157.3 TFLOP/s f32 matrix peak
    out["grad_walk_f32_pipe_frac"] = round(2.0 * N * N * P / 157.3e12 * 1e3 / med["grad_walk"], 3)
    if a.n_iter > 0:
        y0 = 1e-4 * y
        manifold.tsne(x, perplexity=PERPLEXITY, n_iter=2, init=y0)   # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = manifold.tsne(x, perplexity=PERPLEXITY, n_iter=a.n_iter, init=y0)
        torch.cuda.synchronize()
        out["full_s"], out["full_n_iter"] = round(time.perf_counter() - t0, 4), a.n_iter
        out["full_kl"] = float(res.kl_divergence)
        if N <= 8192:
            out["full_knn_preservation_10"] = round(float(manifold.knn_preservation(x, res.embedding, 10)), 4)
    if a.baseline_iters > 0 and N <= TORCH_MAX_N:
        d, Pm = torch_matrices(x, beta, dmin, log_s0)
        g_t = torch_grad(Pm, y, 1.0)
        z, _, _ = ops.tsne_update(rows)
        g_f = 4.0 * (rows[:, 0:2] - rows[:, 2:4] / z)
        out["max_grad"] = float(g_t.abs().max())
        out["max_grad_diff_vs_torch"] = float((g_f - g_t).abs().max())
        s0_t, _ = torch_calib(d, betas, dmin)
        _, s0_f, _ = ops.cond_entropy_sums(x, betas, shift=dmin, nx=nx)
        out["max_s0_rel_diff_vs_torch"] = float(((s0_f - s0_t).abs() / s0_t).max())
        tg = [timed(lambda: torch_grad(Pm, y, 1.0), 1) for _ in range(a.baseline_iters)]
        tc = [timed(lambda: torch_calib(d, betas, dmin), 1) for _ in range(a.baseline_iters)]
        out["torch_grad_ms"], out["torch_calib_ms"] = round(statistics.median(tg), 4), round(statistics.median(tc), 4)
        out["torch_grad_ms_all"], out["torch_calib_ms_all"] = [round(v, 4) for v in tg], [round(v, 4) for v in tc]
        out["grad_speedup_vs_torch"] = round(statistics.median(tg) / med["grad_walk"], 3)
        out["calib_speedup_vs_torch"] = round(statistics.median(tc) / med["calib_walk"], 3)
        del d, Pm
    if a.sklearn:
        out.update(sklearn_times(x, name, a.n_iter if a.n_iter > 0 else 1000))
    del x, y
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="s,m,l,xl")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-iters", type=int, default=3, help="timed runs of the torch baselines (0: skip them)")
    ap.add_argument("--n-iter", type=int, default=1000, help="iterations of the full call (0: skip it)")
    ap.add_argument("--sklearn", action="store_true", help="also time the host library (minutes to hours)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tsne.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    for name in a.shapes.split(","):
        line = json.dumps(run(name, SHAPES[name], a, dev))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
