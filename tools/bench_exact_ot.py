"""The exact coupling by auction rounds on the device (ot.exact_assignment; clipk_auction_rounds, clipk_sim_top2_bias)
against the path the reference's library takes and against the entropic coupling, one JSON line per shape.

  python3 tools/bench_exact_ot.py [--shapes xs,s,m,l] [--iters 3] [--warmup 1] [--scipy-limit 60]
                                  [--out profiles/exact_ot/bench_exact_ot.jsonl]

Shapes (unit clouds, the keys shifted as in tools/bench_sinkhorn.py):   xs N = 256,   P = 128
                                                                        s  N = 1024,  P = 128
                                                                        m  N = 4096,  P = 512
                                                                        l  N = 16384, P = 512
Measured per shape:
  solve       ot.exact_assignment with its defaults (eps = 1e-4 x mean cost, four phases, 32 rounds per host read):
              host clock around the call, which ends in host reads; median of --iters.  rounds = rounds enqueued.
  bids        a second, untimed solve that reads the unassigned count before every round: the bidders of each round,
              their sum, the rounds that had any, and the share of those with at most 64 bidders (one query block)
  one_block   one ops.sim_top2_bias call over an N-row list with a device count of 64 (a late round's bid), and `full`,
              the same call with the count at N (a phase's first round): device events, median of 20
  upstream    what the reference's library does per batch: torch.cdist(x, y)^2 on the device, copy to the host,
              scipy.optimize.linear_sum_assignment, copy the pairs back.  The assignment runs in a child process that
              never opens the device and is abandoned after --scipy-limit seconds (the shape then reports
              "upstream_skipped" and no ratio)
  sinkhorn    for context, the entropic coupling this project had before: ot.sinkhorn with 50 iterations, tol=None, at
              eps = 0.05 x mean cost, plus sample_pairs - device events around both
cost_minus_scipy is the solve's mean cost minus scipy's optimum (where scipy ran), next to the solve's own certificate."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_dplm_amd import ops, ot  # noqa: E402

SHAPES = {
    "xs": dict(N=256, P=128),
    "s": dict(N=1024, P=128),
    "m": dict(N=4096, P=512),
    "l": dict(N=16384, P=512),
}

CHILD = """
import sys, time, numpy as np
from scipy.optimize import linear_sum_assignment
c = np.load(sys.argv[1])
t = time.perf_counter()
r, cols = linear_sum_assignment(c)
dt = time.perf_counter() - t
np.save(sys.argv[2], cols)
print(dt, float(c[r, cols].astype(np.float64).mean()))
"""


def once(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def inputs(N, P, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(N, P, device=dev, generator=g)
    y = torch.randn(N, P, device=dev, generator=g)
    y[:, 0] += 0.3 * math.sqrt(P)
    return x / x.norm(dim=1, keepdim=True), y / y.norm(dim=1, keepdim=True)


def bidders_per_round(x, y):
    """The solve of ot.exact_assignment's defaults, one round per call, the count read before every round."""
    dev, N = x.device, x.shape[0]
    mc = float(ot.mean_cost(x, y))
    bias = -(y * y).sum(1)
    assigned = torch.empty(N, dtype=torch.int32, device=dev)
    owner = torch.empty(N, dtype=torch.int32, device=dev)
    state = torch.zeros(2, dtype=torch.int32, device=dev)
    eps_t = torch.empty(1, dtype=torch.float32, device=dev)
    counts = []
    for e in ot.eps_schedule(0.03 * mc, 1e-4 * mc, 8.0):
        eps_t.fill_(e)
        assigned.fill_(-1)
        owner.fill_(-1)
        left = N
        while left:
            counts.append(left)
            ops.auction_rounds(x, y, bias, eps_t, assigned, owner, state[0:1], state[1:2], 1)
            left, stalled = state.tolist()
            if stalled or len(counts) > 200000:
                return counts
    return counts


def upstream(x, y, limit):
    """(total ms or None, parts, scipy's mean cost or None)."""
    dev = x.device
    torch.cdist(x, y)                                                   # warm-up
    t_d, c = wall(lambda: (torch.cdist(x, y) ** 2).cpu())
    parts = {"cdist_and_copy_ms": round(t_d, 3)}
    with tempfile.TemporaryDirectory() as tmp:
        src, dst = os.path.join(tmp, "c.npy"), os.path.join(tmp, "cols.npy")
        np.save(src, c.numpy())
        try:
            p = subprocess.run([sys.executable, "-c", CHILD, src, dst], capture_output=True, text=True, timeout=limit + 30)
        except subprocess.TimeoutExpired:
            return None, parts, None
        if p.returncode != 0:
            raise RuntimeError(p.stderr)
        dt, opt = (float(v) for v in p.stdout.split())
        cols = np.load(dst)
    parts["assignment_ms"] = round(dt * 1e3, 3)
    if dt > limit:
        return None, parts, opt
    t_b, _ = wall(lambda: torch.from_numpy(cols).to(dev))
    parts["pairs_back_ms"] = round(t_b, 3)
    return t_d + dt * 1e3 + t_b, parts, opt


def run(name, cfg, iters, warmup, limit, dev):
    N, P = cfg["N"], cfg["P"]
    x, y = inputs(N, P, dev)
    out = {"shape": name, "N": N, "P": P}
    for _ in range(warmup):
        r = ot.exact_assignment(x, y)
    t = []
    for _ in range(iters):
        dt, r = wall(lambda: ot.exact_assignment(x, y))
        t.append(dt)
    out.update(solve_ms=round(statistics.median(t), 3), solve_ms_all=[round(v, 3) for v in t], rounds=r.n_rounds,
               phase_rounds=list(r.phase_rounds), converged=r.converged, eps=r.eps, cost=r.cost, gap=r.gap)
    counts = bidders_per_round(x, y)
    out.update(bid_rounds=len(counts), bids=int(sum(counts)),
               share_rounds_le_64_bidders=round(sum(c <= 64 for c in counts) / len(counts), 4),
               ms_per_enqueued_round=round(statistics.median(t) / max(r.n_rounds, 1), 5))
    # ---- one bid pass at one query block and at the full count
    rows = torch.arange(N, dtype=torch.int32, device=dev)
    two = torch.full((1,), 2.0, device=dev)
    nqb, ks = ops.sim_top2_bias_plan(N, N)
    for key, n in (("one_block", min(64, N)), ("full", N)):
        cnt = torch.tensor([n], dtype=torch.int32, device=dev)
        fn = lambda: ops.sim_top2_bias(x, y, two, bias=r.bias, rows=rows, n_active=cnt)     # noqa: E731
        fn()
        out[f"top2_{key}_ms"] = round(statistics.median([once(fn) for _ in range(20)]), 5)
    out.update(top2_query_blocks=nqb, top2_key_splits=ks)
    # ---- the reference library's path
    t_up, parts, opt = upstream(x, y, limit)
    out.update(upstream_parts=parts)
    if opt is not None:
        out["cost_minus_scipy"] = r.cost - opt
    if t_up is None:
        out["upstream_skipped"] = f"linear_sum_assignment alone took more than {limit} s"
    else:
        out.update(upstream_ms=round(t_up, 3), upstream_over_solve=round(t_up / statistics.median(t), 4))
    # ---- the entropic coupling, for context
    def entropic():
        s = ot.sinkhorn(x, y, eps_rel=0.05, n_iters=50, tol=None)
        return s.sample_pairs(seed=1)
    entropic()
    t_s = [once(entropic) for _ in range(max(iters, 3))]
    out.update(sinkhorn50_and_pairs_ms=round(statistics.median(t_s), 3),
               solve_over_sinkhorn=round(statistics.median(t) / statistics.median(t_s), 4))
    del x, y
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="xs,s,m,l")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scipy-limit", type=float, default=60.0)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in a.shapes.split(","):
        line = json.dumps(run(name, SHAPES[name], a.iters, a.warmup, a.scipy_limit, dev))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
