"""Plain vs class-aware vs hard-negative fused similarity passes, for a kernel-time comparison under a tracing profiler:

  rocprofv3 --kernel-trace --stats -d <dir> -o run -- python3 tools/bench_hard_negative.py [--iters 20] [--beta 0.5]
  python3 tools/bench_hard_negative.py --summarize <dir>/.../run_kernel_trace.csv > profiles/hard_negative/kernel_stats.txt

Shapes (those of tools/bench_class_aware.py): B = 1024 x 1024 (P = 512) and one rank's block of an 8-rank global batch,
512 x 4096 (P = 512, label_offset 1024); --p 128 runs them at P = 128, where the exponentials weigh more against the
matrix work.  Per shape the three variants' LSE and gradient passes are launched interleaved (plain, class-aware,
hard-negative, plain, ...), 3 warm-up rounds and then --iters rounds: clipk_simce_lse / clipk_simce_grad_scaled,
clipk_simce_lse_cls / clipk_simce_grad_cls (~B/4 random classes, "mask", eps = 0.1), clipk_simce_lse_hard /
clipk_simce_grad_hard (the same ids).  --summarize groups a rocprofv3 kernel trace by (kernel, grid) and prints the
median and minimum of the last --iters launches of each group.  Without a profiler the script prints device-event
medians per pass (one JSON line per shape)."""
from __future__ import annotations

import argparse
import csv
import json
import os
import re
import statistics
import sys

SHAPES = {"1024x1024": (1024, 1024, 0), "512x4096": (512, 4096, 1024)}
WARMUP = 3


def summarize(path, iters):
    groups = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            m = re.search(r"simce_\w+(<\w+>)?", row["Kernel_Name"])
            if not m:
                continue
            name = m.group(0)
            wg = [int(row[f"Workgroup_Size_{a}"]) for a in "XY"]
            grid = tuple(int(row[f"Grid_Size_{a}"]) // w for a, w in zip("XY", wg))
            groups.setdefault((name, grid), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for (name, grid), us in groups.items():
        us = us[-iters:]
        print(f"{name:<34} grid=({grid[0]},{grid[1]}) n={len(us):3d} median={statistics.median(us):8.2f} us  "
              f"min={min(us):8.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--beta", type=float, default=0.5)
    ap.add_argument("--p", type=int, default=512)
    ap.add_argument("--summarize", metavar="KERNEL_TRACE_CSV")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize, args.iters)

    import torch
    import torch.nn.functional as F

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from clip_dplm_amd import ops

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    P, beta = args.p, args.beta
    sc = torch.tensor([14.2849], device=dev)
    for name, (Mx, Ny, off) in SHAPES.items():
        y = F.normalize(torch.randn(Ny, P, generator=g), dim=-1).to(dev)
        a = F.normalize(torch.randn(Ny, P, generator=g), dim=-1).to(dev)
        x = a[off:off + Mx].contiguous()
        ids = torch.randint(0, Ny // 4, (Ny,), generator=g).to(dev)
        cx = ids[off:off + Mx].contiguous()
        lse_c, _ = ops.simce_lse(y, a, sc)
        lse_cc, _, cnt_c = ops.simce_lse_cls(y, a, sc, ids, ids, "mask", 0.1)
        _, _, coef_c = ops.simce_lse_hard(y, a, sc, beta, ids, ids)
        lse, _ = ops.simce_lse(x, y, sc, label_offset=off)
        lse_k, _, cnt = ops.simce_lse_cls(x, y, sc, cx, ids, "mask", 0.1, label_offset=off)
        _, _, coef = ops.simce_lse_hard(x, y, sc, beta, cx, ids, label_offset=off)
        runs = {
            "plain_lse": lambda: ops.simce_lse(x, y, sc, label_offset=off),
            "cls_lse": lambda: ops.simce_lse_cls(x, y, sc, cx, ids, "mask", 0.1, label_offset=off),
            "hard_lse": lambda: ops.simce_lse_hard(x, y, sc, beta, cx, ids, label_offset=off),
            "plain_grad": lambda: ops.simce_grad(x, y, sc, lse, lse_c, 0.5, 0.5, 1.0 / Ny, label_offset=off),
            "cls_grad": lambda: ops.simce_grad_cls(x, y, sc, lse_k, lse_cc, cnt, cnt_c, 0.5, 0.5, 1.0 / Ny, Ny, cls_x=cx,
                                                   cls_y=ids, same_class="mask", eps=0.1, label_offset=off),
            "hard_grad": lambda: ops.simce_grad_hard(x, y, sc, beta, coef, coef_c, 0.5, 0.5, 1.0 / Ny, cls_x=cx,
                                                     cls_y=ids, label_offset=off),
        }
        ms = {k: [] for k in runs}
        for it in range(WARMUP + args.iters):                     # interleaved: one launch of each variant per round
            for k, fn in runs.items():
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn()
                e.record()
                e.synchronize()
                if it >= WARMUP:
                    ms[k].append(s.elapsed_time(e))
        out = {"shape": name, "Mx": Mx, "Ny": Ny, "P": P, "beta": beta}
        out.update({k + "_ms": round(statistics.median(v), 4) for k, v in ms.items()})
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
