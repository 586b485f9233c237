#!/usr/bin/env python
"""Time one probe training step (forward, backward, Adam) of LinearClassifier on the fused Linear + cross-entropy kernels
against the path the library had before them: torch.cat of the two embedding tensors, linear_f32 (clipk_gemm_f32 +
clipk_gemm_wgrad_f32) and torch.nn.functional.cross_entropy on the device.  Both arms run in one process, alternating by
rounds; device events around `iters` steps; the median and the minimum over the rounds are reported.  The two fused
entries are also timed alone, with the X bytes and f32 MFMA operations they need computed from the shapes:

    forward   X bytes = 4 M K              MFMA flop = 2 M K 16 ceil(C / 16)
    backward  X bytes = 8 M K (two reads)  MFMA flop = 4 M K 16 ceil(C / 16)     (Z again, then G^T X; no dX: frozen inputs)

    python tools/bench_probe.py --out profiles/probe/bench_probe.jsonl
Needs the GPU; there is no CPU fallback."""
import argparse
import json
import statistics
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(131072, 1024, 16), (131072, 1024, 64), (131072, 256, 16), (131072, 256, 64),
          (32, 1024, 16), (32, 1024, 64), (32, 256, 16), (32, 256, 64)]


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e-3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default=None, help="M,K,C;M,K,C;... (default: the eight shapes of profiles/probe/README.md)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_probe.py needs the GPU")
    import clip_dplm_amd as K
    from clip_dplm_amd import functional as KF
    from clip_dplm_amd import ops
    dev = torch.device("cuda:0")
    shapes = SHAPES if args.shapes is None else [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";")]
    records = []
    for M, Kd, C in shapes:
        g = torch.Generator().manual_seed(M + Kd + C)
        xa = torch.randn(M, Kd // 2, generator=g).to(dev)
        xb = torch.randn(M, Kd // 2, generator=g).to(dev)
        labels = torch.randint(0, C, (M,), generator=g).to(dev)
        heads = {}
        for arm in ("fused", "baseline"):
            torch.manual_seed(0)
            m = K.LinearClassifier(Kd, C).to(dev).train()
            heads[arm] = (m, K.FusedAdamW(m, lr=1e-4, weight_decay=0.0, max_grad_norm=None))

        def fused():
            m, opt = heads["fused"]
            opt.zero_grad()
            m.loss(xa, labels, x2=xb).backward()
            opt.step()

        def baseline():
            m, opt = heads["baseline"]
            opt.zero_grad()
            x = torch.cat([xa, xb], dim=-1)
            torch.nn.functional.cross_entropy(KF.linear_f32(x, m.linear.weight, m.linear.bias), labels).backward()
            opt.step()

        mf = heads["fused"][0]
        one = torch.ones(1, device=dev)
        lse = ops.linear_ce_fwd(xa, mf.linear.weight, mf.linear.bias, labels, xb)[0]
        dw, db = torch.empty_like(mf.linear.weight), torch.empty_like(mf.linear.bias)

        def k_fwd():
            ops.linear_ce_fwd(xa, mf.linear.weight.detach(), mf.linear.bias.detach(), labels, xb)

        def k_bwd():
            ops.linear_ce_bwd(xa, mf.linear.weight.detach(), mf.linear.bias.detach(), labels, lse, one, x2=xb, dw=dw, dbias=db)

        iters = 5 if M > 4096 else 200
        arms = {"fused_step": fused, "baseline_step": baseline, "linear_ce_fwd": k_fwd, "linear_ce_bwd": k_bwd}
        for fn in arms.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                times[k].append(timed(fn, iters))
        cp = 16 * ((C + 15) // 16)
        rec = {"M": M, "K": Kd, "C": C, "iters": iters, "rounds": args.rounds}
        for k, v in times.items():
            rec[k + "_median_us"] = round(statistics.median(v) * 1e6, 2)
            rec[k + "_min_us"] = round(min(v) * 1e6, 2)
        for k, xbytes, flop in (("linear_ce_fwd", 4.0 * M * Kd, 2.0 * M * Kd * cp), ("linear_ce_bwd", 8.0 * M * Kd, 4.0 * M * Kd * cp)):
            t = statistics.median(times[k])
            rec[k + "_x_GBps"] = round(xbytes / t * 1e-9, 1)
            rec[k + "_mfma_TFLOPs"] = round(flop / t * 1e-12, 3)
        rec["fused_over_baseline"] = round(rec["fused_step_median_us"] / rec["baseline_step_median_us"], 3)
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del xa, xb, heads
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in records:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
