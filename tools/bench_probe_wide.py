#!/usr/bin/env python
"""Time one probe training step (forward, backward, Adam) of LinearClassifier at class counts beyond 64 - the class-tiled
Linear + cross-entropy kernels (clipk_linear_ce_tiled_*) - against what the library could run before them: torch.cat of
the two embedding tensors, head(x) through linear_f32 (clipk_gemm_f32 + clipk_gemm_wgrad_f32) and
torch.nn.functional.cross_entropy on the device, the same FusedAdamW.  The protocol of profiles/probe/README.md: one
process, the arms alternating by rounds, device events around `iters` calls, medians (and minima) over the rounds.  The
two fused entries are also timed alone (dW and dbias, no dX: frozen inputs), with the f32 MFMA operations they need
computed from the shapes (CP = C padded to the 64-class tile):

    forward   MFMA flop = 2 M K CP
    backward  MFMA flop = 2 M K (CP + C)     (Z again in the tiles, then G^T X in lce_wgrad_kernel<4, true>)

    python tools/bench_probe_wide.py --out profiles/probe/bench_probe_wide.jsonl
    python tools/bench_probe_wide.py --lib build_alt/libclipk.so --arms bwd --shapes 131072,1024,2547   # another build
Needs the GPU; there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(131072, 1024, 158), (131072, 1024, 2547), (32, 1024, 158), (32, 1024, 2547)]
MFMA_F32_PEAK = 155e12       # f32-input MFMA peak of one MI355X (profiles/probe/README.md)


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
    ap.add_argument("--shapes", default=None, help="M,K,C;M,K,C;... (default: the four shapes of profiles/probe/README.md)")
    ap.add_argument("--arms", default="fused_step,baseline_step,fwd,bwd")
    ap.add_argument("--lib", default=None, help="another build of libclipk.so (the backward-slab A/B)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_probe_wide.py needs the GPU")
    from clip_dplm_amd import _ffi
    if args.lib:
        _ffi.LIB_PATH = os.path.abspath(args.lib)
    import clip_dplm_amd as K
    from clip_dplm_amd import ops
    dev = torch.device("cuda:0")
    shapes = SHAPES if args.shapes is None else [tuple(int(v) for v in s.split(",")) for s in args.shapes.split(";")]
    want = args.arms.split(",")
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
            torch.nn.functional.cross_entropy(m(torch.cat([xa, xb], dim=-1)), labels).backward()
            opt.step()

        mf = heads["fused"][0]
        w, b = mf.linear.weight.detach(), mf.linear.bias.detach()
        one = torch.ones(1, device=dev)
        lse = ops.linear_ce_tiled_fwd(xa, w, b, labels, xb)[0]
        dw, db = torch.empty_like(w), torch.empty_like(b)

        def k_fwd():
            ops.linear_ce_tiled_fwd(xa, w, b, labels, xb)

        def k_bwd():
            ops.linear_ce_tiled_bwd(xa, w, b, labels, lse, one, x2=xb, dw=dw, dbias=db)

        iters = 3 if M > 4096 else 200
        arms = {k: fn for k, fn in (("fused_step", fused), ("baseline_step", baseline), ("fwd", k_fwd), ("bwd", k_bwd))
                if k in want}
        for fn in arms.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                times[k].append(timed(fn, iters))
        cp = 64 * ((C + 63) // 64)
        rec = {"M": M, "K": Kd, "C": C, "iters": iters, "rounds": args.rounds, "lib": args.lib or "default"}
        for k, v in times.items():
            rec[k + "_median_us"] = round(statistics.median(v) * 1e6, 2)
            rec[k + "_min_us"] = round(min(v) * 1e6, 2)
        for k, flop in (("fwd", 2.0 * M * Kd * cp), ("bwd", 2.0 * M * Kd * (cp + C))):
            if k in times:
                t = statistics.median(times[k])
                rec[k + "_mfma_TFLOPs"] = round(flop / t * 1e-12, 2)
                rec[k + "_mfma_fraction"] = round(flop / t / MFMA_F32_PEAK, 3)
        if "fused_step" in times and "baseline_step" in times:
            rec["baseline_over_fused"] = round(rec["baseline_step_median_us"] / rec["fused_step_median_us"], 3)
        print(json.dumps(rec), flush=True)
        records.append(rec)
        del xa, xb, heads, lse, dw, db, w, b, mf
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in records:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
