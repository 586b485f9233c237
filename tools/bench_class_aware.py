"""Plain vs class-aware fused similarity + CE passes, for a kernel-time comparison under a tracing profiler:

  rocprofv3 --kernel-trace --stats -d <dir> -o run -- python3 tools/bench_class_aware.py [--iters 20]

Shapes: B = 1024 x 1024 (P = 512) and one rank's block of an 8-rank global batch, 512 x 4096 (P = 512, label_offset
1024).  Each shape runs the plain LSE + gradient passes (clipk_simce_lse / clipk_simce_grad_scaled) and the
class-aware ones (clipk_simce_lse_cls / clipk_simce_grad_cls, ~B/4 random classes, "mask", eps = 0.1) --iters times;
the profiler's per-kernel statistics separate simce_lse_tiled_kernel<false|true> and simce_grad_tiled_kernel<false|true>.
Without a profiler the script prints device-event medians per pass (one JSON line per shape and variant)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from clip_dplm_amd import ops  # noqa: E402

SHAPES = {"1024x1024": (1024, 1024, 0), "512x4096": (512, 4096, 1024)}


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    P = 512
    sc = torch.tensor([14.2849], device=dev)
    for name, (Mx, Ny, off) in SHAPES.items():
        y = F.normalize(torch.randn(Ny, P, generator=g), dim=-1).to(dev)
        a = F.normalize(torch.randn(Ny, P, generator=g), dim=-1).to(dev)
        x = a[off:off + Mx].contiguous()
        ids = torch.randint(0, Ny // 4, (Ny,), generator=g).to(dev)
        cx = ids[off:off + Mx].contiguous()
        lse_c, _ = ops.simce_lse(y, a, sc)
        lse_cc, _, cnt_c = ops.simce_lse_cls(y, a, sc, ids, ids, "mask", 0.1)
        lse, _ = ops.simce_lse(x, y, sc, label_offset=off)
        lse_k, _, cnt = ops.simce_lse_cls(x, y, sc, cx, ids, "mask", 0.1, label_offset=off)
        runs = {
            "plain_lse": lambda: ops.simce_lse(x, y, sc, label_offset=off),
            "cls_lse": lambda: ops.simce_lse_cls(x, y, sc, cx, ids, "mask", 0.1, label_offset=off),
            "plain_grad": lambda: ops.simce_grad(x, y, sc, lse, lse_c, 0.5, 0.5, 1.0 / Ny, label_offset=off),
            "cls_grad": lambda: ops.simce_grad_cls(x, y, sc, lse_k, lse_cc, cnt, cnt_c, 0.5, 0.5, 1.0 / Ny, Ny, cls_x=cx,
                                                   cls_y=ids, same_class="mask", eps=0.1, label_offset=off),
        }
        out = {"shape": name, "Mx": Mx, "Ny": Ny, "P": P}
        for k, fn in runs.items():
            out[k + "_ms"] = round(timed(fn, args.iters), 4)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
