#!/usr/bin/env python3
"""bench.py — seq-pairs/sec of one full contrastive TRAINING step (forward + fused InfoNCE + backward + fused
AdamW with global-norm clip) of the BASELINE dual encoder on MI355X.

Default workload = the configuration BASELINE.json's metric is quoted on:

    ESM-2-35M protein encoder (12 x 480, 20 heads, hd 24, ffn 1920, RoPE) + 6 x 768 RNA transformer
    (8 heads, ffn 2048, gelu, post-LN) + ProjectionHeads (P = 512), B = 1024 pairs per GPU, L = 256, bf16 MFMA
    with f32 accumulate / residual stream / master weights, both encoders trained, synthetic data,
    random-init weights N(0, 0.02).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

--dump-outputs DIR writes the last timed step's loss and a fixed, seeded sample of the updated parameters and of the
gradients to DIR/*.npy (dump_outputs()); inputs and initial weights are seeded, so two builds can be compared.

A plain run only sets up, warms up, times the K steps, dumps (if asked) and prints its line, with the figures taken
inside the timed steps (`roofline` of the dominant kernel, `step_mfu`).  --full adds everything that costs work of its
own, in every --config: `parity` (and the training trajectory) against the CPU oracle, `cpu_baseline`, the per-kernel
breakdown from extra steps outside the timed region, and c5's eager comparison leg.

N > 1 without a torch.distributed environment: this process starts N fresh ranks itself
(`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ...`) BEFORE any HIP call
and exits with the launcher's return code; under torch.distributed.run it is one rank (RCCL over xGMI).

Prints ONE JSON line on rank 0 (contract in the task statement) with
  * `roofline`: dominant kernel = the bf16 MFMA Linear kernel clipk_gemm_nt, timed live with HIP events on its
    launch stream; `traffic` = HBM-side bytes per launch from the committed rocprofv3 --pmc passes of this same
    command (profiles/traffic_gemm_nt.json, written by tools/pmc_traffic.py; FETCH_SIZE doubled per
    MI355X_MICROARCH.md §HBM), null when that file is absent;
  * with --full, `parity`: the step-0 loss of a fixed 32-pair sub-batch on the GPU next to the CPU oracle's on the
    same weights;
  * with --full, `cpu_baseline`: the CPU oracle (kind "port") timed on this box's host cores on a bounded sample
    (B = 32).

Other BASELINE configurations (bench lines of their own, not the driver's default):
    --config c2 --batch 512    config 2 as written (B = 512)
    --config c4                frozen ESM-2-650M (33 x 1280) at L = 1024, B_local = 256 + trained RNA tower / heads
    --config c3sim             fused similarity + CE at one rank's config-3 shape (512 x 4096 x 512): achieved GB/s
    --config c5                ICNN transport system 512 / [512, 256], B = 4096 (eval transport maps)
    --config c1                old/clip.py tiny dual encoder (2 layers, d = 128) on 256 random pairs
    --config notebook          the model the reference actually trained (rna_clip_codes.ipynb:1925-1954) at its own
                               shapes [32, 48, 120] x [32, 600, 1280]; --variant full-bf16 = every position through the
                               bf16 kernels (round 3), default = position 0 sliced before the encoders, exact f32
With --full, every line carries `parity` (GPU vs the CPU oracle on the same inputs) and, where BASELINE.md §3 promises
one, a `cpu_baseline`.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_BF16_PEAK_TFLOPS = 2500.0       # dense bf16 MFMA peak, /opt/skills/guides/MI355X_MICROARCH.md §Chip-level parameters
HBM_PEAK_GBS = 8000.0
MFMA_F32_PEAK_TFLOPS = 157.3         # dense f32 MFMA (= the packed-f32 vector rate): 256 FLOP/clk/CU x 256 CUs x 2.4 GHz


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="c2", choices=["c1", "c2", "c3sim", "c4", "c5", "notebook", "stub"],
                    help="stub: the launch / rendezvous / timing / output plumbing of the multi-rank path on a trivial "
                         "CPU workload over gloo (tests/test_host_logic.py); never a measurement")
    ap.add_argument("--variant", default="sliced-f32", choices=["sliced-f32", "sliced-bf16", "full-bf16", "full-f32"],
                    help="notebook only: sliced = position 0 before the encoders (exact), full = every position as the "
                         "notebook computes them; f32 / bf16 = the arithmetic")
    ap.add_argument("--eager", action="store_true",
                    help="notebook / c1: issue the step's launches eagerly instead of replaying them from one hipGraph "
                         "(training.GraphedTrainStep, the default)")
    ap.add_argument("--batch", type=int, default=None, help="pairs per GPU (default: 1024 for c2, 256 for c4, 4096 for c5)")
    ap.add_argument("--seq-len", type=int, default=None)
    ap.add_argument("--esm", default=None)
    ap.add_argument("--freeze-esm", action="store_true", help="reference behaviour (3_esm_integration.py:83-84)")
    ap.add_argument("--lengths", default="full", choices=["full", "ragged-padded", "ragged-packed"],
                    help="c2 only. full: every sequence L tokens (the BASELINE metric).  ragged-*: SURVEY §8d's padded "
                         "variant, lengths uniform in [L/4, L]: -padded = [B, L] batches + key-padding masks (what the "
                         "reference does), -packed = cu_seqlens batches without any padded row (SURVEY §8f-4)")
    ap.add_argument("--dual-stream", action="store_true",
                    help="enqueue the two towers on separate HIP streams (a kernel's HIP-event time then includes "
                         "waiting for the other tower's kernels)")
    ap.add_argument("--dropout", type=float, default=0.0,
                    help="--config notebook: dropout of the encoder layers and projection heads in the timed training step "
                         "(the notebook trains with 0.1; 0 = the parity configuration)")
    ap.add_argument("--single-stream", action="store_true", help="--config notebook / c1: towers on one HIP stream in the captured step")
    ap.add_argument("--micro-batches", type=int, default=1, help="with --dual-stream: stream pairs per step")
    ap.add_argument("--wgrad-stream", action="store_true", help="weight-gradient GEMMs on a side stream per tower")
    ap.add_argument("--opt", action="append", default=[], metavar="NAME=VALUE",
                    help="libclipk kernel-selection option for this run (experiments; results never depend on options)")
    ap.add_argument("--graph", action="store_true",
                    help="c2 / c4, one GPU: replay the training step from one hipGraph (training.GraphedTrainStep)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what needs work outside the warm-up and timed steps: parity vs the "
                         "CPU oracle, cpu_baseline, the per-kernel breakdown steps, c5's eager leg")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline")
    ap.add_argument("--no-parity", action="store_true", help="with --full: skip parity")
    ap.add_argument("--no-kernel-timers", action="store_true")
    ap.add_argument("--all-kernel-timers", action="store_true",
                    help="HIP events around EVERY kernel launch of the timed region (costs ~1 %% of the step); "
                         "default: only the dominant kernel, clipk_gemm_nt")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="c2 / c4: after the timed steps write what the last timed step computed to DIR/<name>.npy "
                         "(dump_outputs()), so that two builds can be compared output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs is not None and args.config not in ("c2", "c4"):
        ap.error("--dump-outputs is implemented for --config c2 / c4")
    return args


def self_launch(args) -> int:
    """--gpus N > 1 outside torch.distributed.run: start N fresh ranks.  Nothing in this process has touched HIP."""
    port = 29500 + (os.getpid() % 2000)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    print(f"[bench] starting {args.gpus} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    return subprocess.run(cmd, env=env).returncode


def collective_report(device, world):
    """What the collective library actually saw, for the N > 1 line (VERDICT r03 #6a: the driver must be able to tell
    that RCCL had N ranks on N devices): backend, world size, an all-reduce of 1 over every rank, and each rank's
    (rank, device index, PCI bus id) gathered through the same process group the training step uses."""
    import torch
    import torch.distributed as dist
    if not dist.is_initialized():
        return None
    one = torch.ones(1, dtype=torch.int64, device=device)
    dist.all_reduce(one)
    bus = -1
    if device.type == "cuda":
        bus = int(getattr(torch.cuda.get_device_properties(device), "pci_bus_id", -1))
    mine = torch.tensor([dist.get_rank(), device.index if device.index is not None else -1, bus], dtype=torch.int64,
                        device=device)
    everyone = torch.empty(world * 3, dtype=torch.int64, device=device)
    dist.all_gather_into_tensor(everyone, mine)
    rows = everyone.view(world, 3).tolist()
    rep = {"backend": dist.get_backend(), "world": dist.get_world_size(), "ranks_seen": int(one.item()),
           "devices": [{"rank": r, "device_index": d, "pci_bus_id": b} for r, d, b in rows],
           "distinct_devices": len({(d, b) for _, d, b in rows})}
    if device.type == "cuda" and dist.get_backend() == "nccl":
        try:
            rep["library_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:                                    # version probing must never cost the line
            rep["library_version"] = None
    return rep


def synth_batch(B, L, rna_dim, device, seed):
    """protein ids uniform over the 20 standard amino-acid ids [4, 24) with <cls>=0 first and <eos>=2
    last, no padding; RNA side N(0,1) features [B, L, rna_dim] (the reference feeds precomputed RNABERT vectors)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(4, 24, (B, L), generator=g)
    ids[:, 0] = 0
    ids[:, -1] = 2
    rna = torch.randn(B, L, rna_dim, generator=g)
    return rna.to(device), ids.to(device)


def host_threads():
    try:
        n = len(os.sched_getaffinity(0))                  # the cores this process may actually use (cgroup share)
    except AttributeError:
        n = os.cpu_count() or 1
    return max(1, min(n, 64))


def cpu_baseline(model_sd, cfg, L, sample_b=32, steps=3, budget_s=75.0, probe=None):
    """Time the CPU oracle (kind 'port') on a bounded sample of the same workload: forward + backward + clip + AdamW
    (B = 32, >= 3 steps).  The first (warm-up) step runs on the initial weights, so its loss is also the
    oracle side of the `parity` object, and the loss of every later step (taken BEFORE that step's update, i.e. after
    `it` updates) is the oracle's training trajectory for `parity.trajectory`.
    probe (optional, from gpu_trajectory): {"grads0": name -> the fused path's step-0 gradient, "weights": [state_dict
    after 1, 2, ... fused updates]} - filled in here with (i) how many gradient entries differ in SIGN between the two
    paths at step 0 and what share of sum|g| they carry (AdamW's first update is lr * sign(g) for every entry, however
    small: such entries move the weights apart by 2 lr each), (ii) the oracle's loss AT the fused path's weights after
    each update, which splits a trajectory difference into forward arithmetic and weight divergence.
    Returns (cpu_baseline dict, [oracle loss after 0, 1, ... updates])."""
    import torch
    from oracle import model_ref
    ncores = host_threads()
    torch.set_num_threads(ncores)
    frozen = cfg.get("frozen_prefix")
    sd = {k: v.detach().float().cpu().clone().requires_grad_(v.is_floating_point() and not (frozen and k.startswith(frozen)))
          for k, v in model_sd.items()}
    params = [v for v in sd.values() if v.requires_grad]
    opt = torch.optim.AdamW(params, lr=1e-4, weight_decay=0.01)
    rna, ids = synth_batch(sample_b, L, cfg["rna_dim"], "cpu", 4321)
    if cfg.get("rna_len") and cfg["rna_len"] != L:
        rna = rna[:, : cfg["rna_len"]].contiguous()
    times, losses = [], []
    t_start = time.perf_counter()
    for it in range(steps + 1):
        t0 = time.perf_counter()
        opt.zero_grad()
        loss, _, _ = model_ref.protein_rna_clip_loss(sd, rna, ids, None, None, esm_layers=cfg["esm_layers"],
                                                     esm_heads=cfg["esm_heads"], rna_layers=cfg["rna_layers"],
                                                     rna_heads=cfg["rna_heads"])
        losses.append(float(loss.item()))
        loss.backward()
        if it == 0 and probe is not None and probe.get("grads0"):
            flips = total = 0
            carried = mass = 0.0
            for name, gg in probe["grads0"].items():
                r = sd[name].grad
                if r is None:
                    continue
                d = torch.sign(gg) != torch.sign(r)
                flips += int(d.sum()); total += d.numel()
                carried += float(r.abs()[d].sum()); mass += float(r.abs().sum())
            probe["sign_flips"] = {"entries": flips, "of": total, "share_of_entries": flips / max(total, 1),
                                   "share_of_sum_abs_grad": carried / max(mass, 1e-30)}
            probe["grads0"] = None
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        times.append(time.perf_counter() - t0)
        print(f"[cpu_baseline] step {it}: {times[-1]:.2f} s on {ncores} threads", file=sys.stderr, flush=True)
        if time.perf_counter() - t_start > budget_s:      # bounded sample: never hold the bench for minutes
            break
    if probe is not None and probe.get("weights"):
        probe["loss_oracle_at_gpu_weights"] = []
        for w in probe["weights"][: len(losses) - 1]:
            with torch.no_grad():
                lw, _, _ = model_ref.protein_rna_clip_loss(w, rna, ids, None, None, esm_layers=cfg["esm_layers"],
                                                           esm_heads=cfg["esm_heads"], rna_layers=cfg["rna_layers"],
                                                           rna_heads=cfg["rna_heads"])
            probe["loss_oracle_at_gpu_weights"].append(float(lw.item()))
        probe["weights"] = None
    steps = len(times) - 1
    timed = sorted(times[1:] if len(times) > 1 else times)   # drop the warm-up step when there is more than one
    dt = timed[len(timed) // 2]                              # median
    return ({"value": round(sample_b / dt, 3), "unit": "seq-pairs/s", "cores": ncores, "kind": "port",
             "sample": f"median of {len(timed)} training step(s) (fwd+bwd+clip+AdamW) of the CPU oracle at B={sample_b}, "
                       f"L={L}, f32, {'after 1 warm-up step' if len(times) > 1 else 'no warm-up (time budget)'}; "
                       f"{dt:.2f} s/step"}, losses)


def gpu_trajectory(build_model, sd_cpu, device, Lp, rna_dim=768, sample_b=32, updates=3):
    """The training trajectory of the fused path on the parity sub-batch: the same `updates` optimiser steps the CPU
    oracle takes in cpu_baseline() (rna_clip_codes.ipynb:2061-2089 / old/ablation.py:9-18: loss -> backward ->
    clip_grad_norm_(1.0) -> AdamW(lr 1e-4, weight_decay 0.01)) on the same 32 pairs from the same initial weights, on a
    private copy of the model (the timed model stays at its initial weights).  Returns (the loss after 0 .. updates
    updates, each taken before the next update as the oracle's; a probe for cpu_baseline(): the step-0 gradients and the
    weights after each update, on the host)."""
    import torch
    import clip_dplm_amd as K
    m = build_model()
    m.load_state_dict(sd_cpu)
    m = m.to(device).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    opt = K.FusedAdamW(m, lr=1e-4, weight_decay=0.01, max_grad_norm=1.0)
    rna, ids = synth_batch(sample_b, Lp, rna_dim, device, 4321)
    losses, probe = [], {"grads0": None, "weights": []}
    for it in range(updates + 1):
        opt.zero_grad()
        loss = m.loss(rna, ids)
        losses.append(float(loss.item()))
        loss.backward()
        if it == 0:
            probe["grads0"] = {n: p.grad.detach().float().cpu().clone() for n, p in m.named_parameters()
                               if p.grad is not None}
        if it == updates:
            break
        opt.step()
        probe["weights"].append({k: v.detach().float().cpu().clone() if v.is_floating_point() else v.detach().cpu().clone()
                                 for k, v in m.state_dict().items()})
    del opt, m, rna, ids
    torch.cuda.empty_cache()
    return losses, probe


def _gemm_sources():
    """Every source clipk_gemm_nt can dispatch to (csrc/gemm_nt*.hip by glob: ADVICE r03 - v4 was missing from a fixed
    list) + the shared epilogue / common headers."""
    import glob
    d = os.path.join(ROOT, "clip_dplm_amd", "csrc")
    return tuple(sorted(os.path.basename(f) for f in glob.glob(os.path.join(d, "gemm_nt*.hip")))) + ("gemm_epilogue.h", "common.h")


GEMM_SOURCES = _gemm_sources()


def gemm_source_hash() -> str:
    """sha256 over the sources of the dominant kernel (csrc/gemm_nt*.hip + the shared epilogue / common headers): a PMC
    traffic figure is only attached to a bench line whose kernels are the ones it was measured on."""
    import hashlib
    h = hashlib.sha256()
    for name in GEMM_SOURCES:
        with open(os.path.join(ROOT, "clip_dplm_amd", "csrc", name), "rb") as f:
            h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


def traffic_key(config, B, L, lengths="full", esm=None) -> str:
    return f"{config}_B{B}_L{L}_{lengths}" + (f"_{esm}" if esm else "")


def load_traffic(workload_key):
    """HBM-side bytes per clipk_gemm_nt launch from the committed rocprofv3 --pmc passes (tools/pmc_traffic.py), for
    exactly this workload (config, batch, length, length mode, encoder) — and only while the GEMM sources are the ones
    the passes ran on.  Returns (entry or None, stale flag)."""
    path = os.path.join(ROOT, "profiles", "traffic_gemm_nt.json")
    try:
        with open(path) as f:
            t = json.load(f)
    except (OSError, ValueError):
        return None, False
    e = t.get(workload_key)
    if e is None:
        return None, False
    if e.get("source_sha16") != gemm_source_hash():
        return None, True
    return e, False


DUMP_SAMPLE = 1 << 22                # entries per sampled array: 2 x 16 MB of f32, well under the 64 MB cap
DUMP_SEED = 20240
DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, loss, model) -> dict:
    """--dump-outputs: what the last timed training step handed its caller, as DIR/<name>.npy (float32).
      loss.npy           [1]  the step's loss
      params_sample.npy  [n]  the updated trainable parameters (module.parameters() order, flattened, concatenated)
      grads_sample.npy   [n]  the step's gradients (what p.grad holds after the optimiser step), same entries
    Both parameter-sized arrays hold the same fixed, seeded sample of DUMP_SAMPLE positions (sorted, duplicates
    dropped) when there are more entries than that, else every entry.  Returns {name: shape}."""
    import numpy as np
    import torch
    params = [p for p in model.parameters() if p.requires_grad]
    flat_p = torch.cat([p.detach().reshape(-1).float() for p in params])
    flat_g = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1).float()
                        for p in params])
    n = flat_p.numel()
    if n > DUMP_SAMPLE:
        idx = np.unique(np.random.default_rng(DUMP_SEED).integers(0, n, DUMP_SAMPLE))
        idx = torch.from_numpy(idx).to(flat_p.device)
        flat_p, flat_g = flat_p[idx], flat_g[idx]
    arrays = {"loss": loss.detach().float().reshape(1).cpu().numpy(),
              "params_sample": flat_p.cpu().numpy(),
              "grads_sample": flat_g.cpu().numpy()}
    assert sum(a.nbytes for a in arrays.values()) <= DUMP_MAX_BYTES
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), a.astype(np.float32))
    return {name: list(a.shape) for name, a in arrays.items()}


# ====================================================================================================== c2 / c4
def bench_clip(args):
    import torch
    import torch.distributed as dist

    import clip_dplm_amd as K
    from clip_dplm_amd import ops
    from clip_dplm_amd.distributed import init_distributed
    from clip_dplm_amd.encoders import ESM2_SHAPES
    import clip_dplm_amd.encoders as _enc

    c4 = args.config == "c4"
    esm = args.esm or ("esm2_t33_650M_UR50D" if c4 else "esm2_t12_35M_UR50D")
    B = args.batch or (256 if c4 else 1024)
    Lp = args.seq_len or (1024 if c4 else 256)
    Lr = 256 if c4 else Lp
    freeze = args.freeze_esm or c4

    rank, world, device = init_distributed()
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    for kv in args.opt:
        name, _, val = kv.partition("=")
        ops.set_option(name, int(val))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    force_dist = bool(os.environ.get("CLIPK_FORCE_DIST"))     # rehearse the RCCL code path with a 1-rank group
    if force_dist and not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=device)
    group = dist.group.WORLD if (world > 1 or force_dist) else None

    torch.manual_seed(0)                                  # identical weights on every rank
    model = K.ProteinRNACLIP(esm=esm, freeze_protein_encoder=freeze).to(device).train()
    for m in model.modules():                             # training-step timing with dropout p = 0
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    model.dual_stream = bool(args.dual_stream)
    model.micro_batches = args.micro_batches
    _enc.WGRAD_SIDE_STREAM = args.wgrad_stream
    nl, d, h, f = ESM2_SHAPES[esm]
    want_oracle = args.full and rank == 0 and world == 1 and not (args.no_cpu_baseline and args.no_parity)
    want_cpu = want_oracle and not c4
    want_c4_cpu = want_oracle and c4
    sd_cpu = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()} if want_cpu else None

    # ---- parity object, GPU side: step-0 loss of a fixed 32-pair sub-batch on the initial weights (eval mode == train
    # mode here: dropout p = 0).  The oracle side comes from cpu_baseline()'s first step on the same batch.
    parity = None
    if want_cpu and not args.no_parity:
        rna_s, ids_s = synth_batch(32, Lp, 768, device, 4321)
        with torch.no_grad():
            parity = {"sub_batch": 32, "loss_gpu": float(model.loss(rna_s, ids_s).item())}
        del rna_s, ids_s
        # ... and the first optimiser steps of the same sub-batch (the metric is a TRAINING step)
        parity["_traj_gpu"] = gpu_trajectory(lambda: K.ProteinRNACLIP(esm=esm, freeze_protein_encoder=freeze), sd_cpu,
                                             device, Lp)

    opt = K.FusedAdamW(model, lr=1e-4, weight_decay=0.01, max_grad_norm=1.0, group=group)
    g = torch.Generator().manual_seed(1234 + rank)
    ids = torch.randint(4, 24, (B, Lp), generator=g)
    ids[:, 0], ids[:, -1] = 0, 2
    rna = torch.randn(B, Lr, 768, generator=g).to(device)
    ids = ids.to(device)

    ragged = args.lengths != "full" and not c4
    if ragged:
        from clip_dplm_amd.data import unpad
        lp = torch.randint(Lp // 4, Lp + 1, (B,), generator=g)
        lr = torch.randint(Lr // 4, Lr + 1, (B,), generator=g)
        pmask = (torch.arange(Lp)[None] < lp[:, None])
        rmask = (torch.arange(Lr)[None] < lr[:, None])
        real_tokens = int(pmask.sum() + rmask.sum())
        if args.lengths == "ragged-packed":
            (rp, rcu, rmax), (ip, icu, imax) = unpad(rna.cpu(), rmask), unpad(ids.cpu(), pmask)
            rp, rcu, ip, icu = rp.to(device), rcu.to(device), ip.to(device), icu.to(device)
        else:
            pmask_d, rmask_d = pmask.to(device).long(), rmask.to(device).long()

    def step():
        opt.zero_grad()
        if not ragged:
            loss = model.loss(rna, ids, group=group)
        elif args.lengths == "ragged-packed":
            loss = model.loss_packed(rp, rcu, rmax, ip, icu, imax, group=group)
        else:
            loss = model.loss(rna, ids, rna_mask=rmask_d, protein_mask=pmask_d, group=group)
        loss.backward()
        opt.step()
        return loss

    eager_step = step
    if args.graph and world == 1 and not force_dist and not ragged and not model.dual_stream:
        from clip_dplm_amd.training import GraphedTrainStep
        gstep = GraphedTrainStep(model, opt, lambda a, b: model.loss(a, b), (rna, ids), warmup=2)
        step = lambda: gstep(rna, ids)
    tw = time.perf_counter()
    for i in range(args.warmup):
        step()
        torch.cuda.synchronize()
        if rank == 0:
            print(f"[bench] warm-up step {i}: {time.perf_counter() - tw:.2f} s since start", file=sys.stderr, flush=True)
    timer = None
    if not args.no_kernel_timers:
        # timed region: only the dominant kernel (the roofline object); --all-kernel-timers times every launch
        timer = ops.KernelTimer(None if args.all_kernel_timers else ("gemm_nt",))
        ops.set_kernel_timer(timer)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    ops.set_kernel_timer(None)
    # the last timed step's outputs, before the breakdown steps below move the weights on
    dumped = dump_outputs(args.dump_outputs, loss, model) if (args.dump_outputs and rank == 0) else None
    # --full: two more steps OUTSIDE the timed region, one HIP stream, HIP events around every launch: the per-class
    # breakdown (`kernels`) without taxing the timed region (~1 % when every launch is timed).
    timer_alone = None
    was_dual = model.dual_stream
    if args.full and timer is not None and rank == 0 and world == 1 and (was_dual or not args.all_kernel_timers):
        model.dual_stream = False
        eager_step(); torch.cuda.synchronize()
        timer_alone = ops.KernelTimer()
        ops.set_kernel_timer(timer_alone)
        for _ in range(2):
            eager_step()
        torch.cuda.synchronize()
        ops.set_kernel_timer(None)
        model.dual_stream = was_dual
    tmax = torch.tensor([dt], device=device)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = tmax.item()
    coll = collective_report(device, world) if (world > 1 or force_dist) else None      # every rank takes part
    if rank == 0:
        print(f"[bench] {args.steps} timed steps: {dt:.3f} s", file=sys.stderr, flush=True)
    if rank != 0:
        if dist.is_initialized():
            dist.destroy_process_group()
        return

    if c4:
        workload = (f"BASELINE config 4 (one rank's share): frozen {esm} protein encoder (33 x 1280, hd 64) at L={Lp}, "
                    f"B={B} sequences/GPU + trained 6x768 RNA transformer (L={Lr}) and projection heads, full training "
                    f"step (fwd + fused InfoNCE + bwd of the trained parts + fused AdamW/clip)")
        metric = "seq-pairs/sec/node, contrastive training step, frozen ESM-2-650M dual encoder (config 4)"
    else:
        workload = (f"BASELINE metric config: {esm} protein encoder + 6x768 RNA transformer, B={B} pairs/GPU, L={Lp}, "
                    f"full training step (fwd + fused InfoNCE + bwd + fused AdamW/clip), "
                    + ("ESM frozen" if freeze else "both encoders trained"))
        metric = "seq-pairs/sec/node, contrastive training step, ESM-2-35M dual encoder"
    out = {
        "metric": metric,
        "value": round(B * world * args.steps / dt, 2),
        "unit": "seq-pairs/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1e3 * dt / args.steps, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "config": {"workload": workload, "global_batch": B * world, "seq_len": Lp, "parallelism": f"dp{world}",
                   "projection_dim": 512, "hip_streams": 2 if model.dual_stream else 1,
                   "launch": "hipGraph replay" if step is not eager_step else "eager"},
        "loss": round(float(loss.item()), 5),
    }
    if coll is not None:
        out["rccl"] = coll
    if dumped is not None:
        out["dump_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
    if ragged:
        out["config"]["lengths"] = (f"{args.lengths}: lengths uniform in [L/4, L]; {real_tokens} real tokens of "
                                    f"{B * (Lp + Lr)} padded positions ({real_tokens / (B * (Lp + Lr)):.3f})")
    # algorithmic FLOP of one step (8d^2 + 4Ld + 4df per token.layer forward; x3 trained, x1 frozen)
    fl_esm = (8 * d * d + 4 * Lp * d + 4 * d * f) * nl * Lp * (1 if freeze else 3)
    fl_rna = (8 * 768 * 768 + 4 * Lr * 768 + 4 * 768 * 2048) * 6 * Lr * 3
    step_tflop = B * (fl_esm + fl_rna) / 1e12
    out["step_mfu"] = {"algorithmic_tflop_per_step": round(step_tflop, 2),
                       "achieved_tflops": round(step_tflop / (dt / args.steps), 1),
                       "frac_of_bf16_peak": round(step_tflop / (dt / args.steps) / MFMA_BF16_PEAK_TFLOPS, 4)}
    if ragged:
        # the REAL tokens' work: per sequence and layer (8d^2 + 4df) * len + 4 d len^2 (attention is quadratic in the
        # sequence's own length); the padded figure above counts positions that hold no token
        lpf, lrf = lp.double(), lr.double()
        real_esm = float(((8 * d * d + 4 * d * f) * lpf + 4 * d * lpf * lpf).sum()) * nl * (1 if freeze else 3)
        real_rna = float(((8 * 768 * 768 + 4 * 768 * 2048) * lrf + 4 * 768 * lrf * lrf).sum()) * 6 * 3
        real_tflop = (real_esm + real_rna) / 1e12
        out["step_mfu"] = {"algorithmic_tflop_per_step": round(real_tflop, 2),
                           "achieved_tflops": round(real_tflop / (dt / args.steps), 1),
                           "frac_of_bf16_peak": round(real_tflop / (dt / args.steps) / MFMA_BF16_PEAK_TFLOPS, 4),
                           "counts": "real tokens only",
                           "padded_positions_tflop_per_step": round(step_tflop, 2),
                           "padded_positions_frac_of_bf16_peak": round(step_tflop / (dt / args.steps) / MFMA_BF16_PEAK_TFLOPS, 4)}
    if timer is not None:
        summ = timer.summary()
        gm = summ.get("gemm_nt")
        if gm:
            achieved = gm["work"] / (gm["total_ms"] * 1e-3) / 1e12
            traffic, traffic_stale = load_traffic(traffic_key(args.config, B, Lp, args.lengths if not c4 else "full",
                                                              args.esm))
            out["roofline"] = {"bound": "mfma",
                               "kernel": "clipk_gemm_nt = gemm_nt_v3_kernel / gemm_nt_v2_kernel (bf16 16x16x32 MFMA Linear fwd/dgrad)",
                               "achieved": round(achieved, 2), "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                               "frac": round(achieved / MFMA_BF16_PEAK_TFLOPS, 4),
                               "traffic": traffic["bytes_per_launch"] if traffic else None,
                               # the same launches against the OTHER roof: HBM-side bytes (PMC) per average launch
                               "frac_hbm": round(traffic["bytes_per_launch"] / (gm["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
                               if traffic else None,
                               "frac_hbm_algorithmic": round(gm["bytes"] / (gm["total_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                               "avg_launch_us": round(gm["avg_us"], 2), "launches": gm["launches"],
                               "share_of_step": round(gm["total_ms"] / (1e3 * dt), 4),
                               "algorithmic_bytes_per_launch": round(gm["bytes"] / max(gm["launches"], 1)),
                               "peak_note": "nominal dense bf16 peak at 2.4 GHz; these MFMA loops hold 1.8-2.0 GHz in-kernel "
                                            "on random data (measured: profiles/r02/wgrad_trace_v2.txt, DESIGN.md 3.2), and the "
                                            "K = 480 shapes are bounded by their output stores, not by the matrix pipe"}
            if traffic:
                out["roofline"]["traffic_detail"] = {k: traffic[k] for k in traffic if k != "bytes_per_launch"}
            elif traffic_stale:
                out["roofline"]["traffic_stale"] = True     # the GEMM sources changed since the PMC passes: re-measure
                                                            # with tools/profile_bench.sh
            # per epilogue mode (the GELU pair is the slowest class of the dominant kernel: VERDICT r02 weak #7)
            out["roofline"]["by_epilogue"] = {
                k: {"launches": v["launches"], "avg_us": round(v["avg_us"], 1),
                    "tflops": round(v["work"] / (v["total_ms"] * 1e-3) / 1e12, 1),
                    "frac": round(v["work"] / (v["total_ms"] * 1e-3) / 1e12 / MFMA_BF16_PEAK_TFLOPS, 4),
                    "share_of_kernel": round(v["total_ms"] / gm["total_ms"], 4)}
                for k, v in sorted(timer.summary_by_sub("gemm_nt").items(), key=lambda kv: -kv[1]["total_ms"])}
        src, steps_src, tag = (summ, args.steps, "timed region") if (args.all_kernel_timers or timer_alone is None) \
            else (timer_alone.summary(), 2, "2 extra steps, one HIP stream, outside the timed region")
        out["kernels"] = {k: {"launches_per_step": v["launches"] // steps_src, "avg_us": round(v["avg_us"], 2),
                              "ms_per_step": round(v["total_ms"] / steps_src, 3),
                              "rate": round(v["work"] / (v["total_ms"] * 1e-3) / 1e12, 3),
                              "rate_unit": "TFLOP/s" if ("gemm" in k or "attn" in k) else "TB/s"}
                          for k, v in src.items()}
        out["kernels"]["_source"] = tag
    if want_cpu:
        del opt, model, rna, ids
        torch.cuda.empty_cache()
        probe = parity["_traj_gpu"][1] if parity is not None else None
        cb, traj_or = cpu_baseline(sd_cpu, {"rna_dim": 768, "esm_layers": nl, "esm_heads": h, "rna_layers": 6,
                                            "rna_heads": 8}, Lp, probe=probe)
        loss0 = traj_or[0]
        if not args.no_cpu_baseline:
            out["cpu_baseline"] = cb
        if parity is not None:
            traj_gpu, _ = parity.pop("_traj_gpu")
            parity["loss_oracle"] = loss0
            parity["loss_abs_err"] = abs(parity["loss_gpu"] - loss0)
            parity["bar"] = 1e-3
            parity["note"] = "step-0 loss, initial weights, 32 pairs (seed 4321), full depth; oracle = CPU f32 restatement"
            parity["trajectory"] = [{"step": i, "loss_gpu": lg, "loss_oracle": lo, "abs_err": abs(lg - lo)}
                                    for i, (lg, lo) in enumerate(zip(traj_gpu, traj_or))]
            at_w = [loss0] + list(probe.get("loss_oracle_at_gpu_weights") or [])
            for t_, lw in zip(parity["trajectory"], at_w):
                # |gpu - oracle| = forward arithmetic at the SAME weights (+) how far the two weight sets have moved apart
                t_["loss_oracle_at_gpu_weights"] = lw
                t_["forward_abs_err"] = abs(t_["loss_gpu"] - lw)
                t_["weight_divergence_abs_err"] = abs(lw - t_["loss_oracle"])
            parity["trajectory_max_abs_err"] = max(t_["abs_err"] for t_ in parity["trajectory"])
            parity["trajectory_max_forward_abs_err"] = max(t_.get("forward_abs_err", 0.0) for t_ in parity["trajectory"])
            parity["trajectory_sign_flips_step0"] = probe.get("sign_flips")
            parity["trajectory_note"] = (
                "loss after `step` fused optimiser updates (clip 1.0 + AdamW lr 1e-4, wd 0.01) of the same 32 pairs vs the "
                "CPU oracle's torch.optim.AdamW trajectory, bar 1e-3; forward_abs_err = GPU loss vs the oracle evaluated at "
                "the GPU path's own weights (the parity claim at every trained step), weight_divergence_abs_err = the "
                "oracle at the GPU path's weights vs the oracle's own trajectory: AdamW's first update is lr * sign(g) for "
                "every entry, so the entries whose bf16 gradient differs in sign (trajectory_sign_flips_step0: a fraction "
                "of a percent of the entries, carrying ~1e-5 of sum|g|) move by 2 lr each")
            out["parity"] = parity
    if want_c4_cpu:
        sd_full = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        del opt, model, rna, ids
        torch.cuda.empty_cache()
        if not args.no_parity:
            out["parity"] = c4_parity(device, Lp)
        if not args.no_cpu_baseline:
            # config 4 on the host at B = 1, one step (frozen 650M forward at L = 1024 + trained RNA tower)
            cb, _traj = cpu_baseline(sd_full, {"rna_dim": 768, "esm_layers": nl, "esm_heads": h, "rna_layers": 6,
                                           "rna_heads": 8, "rna_len": Lr, "frozen_prefix": "protein_model."},
                                 Lp, sample_b=1, steps=1, budget_s=60.0)
            out["cpu_baseline"] = cb
    emit(out)
    if dist.is_initialized():
        dist.destroy_process_group()


def c4_parity(device, Lp):
    """Config 4's arithmetic at reduced DEPTH: two layers of the ESM-2-650M shape (1280 / 20 x 64 / 5120, frozen) at
    L = 1024 + two RNA layers + heads, step-0 loss of 8 pairs, GPU vs CPU oracle (bar 1e-3)."""
    import torch

    import clip_dplm_amd as K
    from clip_dplm_amd.encoders import ESM2_SHAPES
    from oracle import model_ref
    ESM2_SHAPES["c4_parity"] = (2, 1280, 20, 5120)
    torch.manual_seed(5)
    m = K.ProteinRNACLIP(esm="c4_parity", rna_layers=2, freeze_protein_encoder=True).eval()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(99)
    ids = torch.randint(4, 24, (8, Lp), generator=g)
    ids[:, 0], ids[:, -1] = 0, 2
    rna = torch.randn(8, 256, 768, generator=g)
    m = m.to(device)
    with torch.no_grad():
        lg = float(m.loss(rna.to(device), ids.to(device)).item())
    del m
    torch.cuda.empty_cache()
    torch.set_num_threads(host_threads())
    with torch.no_grad():
        lo, _, _ = model_ref.protein_rna_clip_loss(sd, rna, ids, None, None, esm_layers=2, esm_heads=20, rna_layers=2,
                                                   rna_heads=8)
    return {"sub_batch": 8, "loss_gpu": lg, "loss_oracle": float(lo.item()), "loss_abs_err": abs(lg - float(lo.item())),
            "bar": 1e-3, "note": f"two layers of the 650M shape (1280 / 20 x 64 / 5120) at L={Lp} + two RNA layers + heads, "
                                 "step-0 loss of 8 pairs (seed 99); oracle = CPU f32 restatement"}


# ====================================================================================================== stub
def bench_stub(args):
    """The multi-rank plumbing of bench_clip on a trivial workload (CPU tensors, gloo): same init_distributed(), the
    same WORLD_SIZE / --gpus check, barrier-bracketed timed region, MAX over ranks, ONE JSON line from rank 0, every
    other rank silent.  CLIPK_BENCH_STUB_FAIL_RANK=r makes rank r fail after the rendezvous (the launcher's return code
    must show it).  Touches no GPU."""
    import torch
    import torch.distributed as dist
    from clip_dplm_amd.distributed import init_distributed
    rank, world, _ = init_distributed(backend="gloo", cpu_only=True)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    fail = os.environ.get("CLIPK_BENCH_STUB_FAIL_RANK")
    if fail is not None and int(fail) == rank:
        raise SystemExit(f"[stub] rank {rank} fails on request")
    print("library chatter that must not reach the JSON stream")          # (fd 1 points at stderr by now)
    x = torch.ones(1024) * (rank + 1)

    def step():
        y = x * 2.0
        if world > 1:
            dist.all_reduce(y)
        return y
    for _ in range(args.warmup):
        step()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        y = step()
    if world > 1:
        dist.barrier()
    tmax = torch.tensor([time.perf_counter() - t0])
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = max(tmax.item(), 1e-9)
    coll = collective_report(torch.device("cpu"), world) if world > 1 else None
    if rank == 0:
        emit({"metric": "stub", "rccl": coll, "value": round(1024 * world * args.steps / dt, 1), "unit": "elements/s", "n_gpus": world,
              "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 4),
              "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
              "config": {"workload": "plumbing stub (CPU, gloo)"}, "checksum": float(y.sum().item())})
    if dist.is_initialized():
        dist.destroy_process_group()


# ====================================================================================================== c1
def bench_c1(args):
    """BASELINE config 1 (plumbing): old/clip.py's tiny dual encoder — 2 x Linear(128)+ReLU, LayerNorm, ProjectionHead
    (128 -> 256 -> 128) per tower — on 256 random pairs: one TRAINING step = forward + one-sided CE (old/ablation.py:16)
    + backward + fused AdamW (lr 1e-4).  SURVEY §8d inputs: weights torch.manual_seed(0), x ~ N(0,1) from seed 1234.
    Launch-latency bound (~60 launches of microsecond kernels); reported for completeness, never optimised."""
    import torch
    from types import SimpleNamespace as NS

    import clip_dplm_amd as K
    from clip_dplm_amd import ops
    dev = torch.device("cuda:0")
    B = args.batch or 256
    sub = lambda hh: NS(hidden_size=hh, num_hidden_layers=2, layer_norm_eps=1e-12)
    cfg = NS(rna_config=sub(128), protein_config=sub(128), diffmap_config=sub(128), projection_dim=128,
             logit_scale_init_value=2.6592)
    torch.manual_seed(0)
    model = K.RNAProteinCLIPModule(cfg).eval()             # eval: dropout off, gradients still flow
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(1234)
    xa, xb = torch.randn(B, 128, generator=g), torch.randn(B, 128, generator=g)
    model = model.to(dev)
    xa_d, xb_d = xa.to(dev), xb.to(dev)
    if args.full:
        with torch.no_grad():
            loss_gpu0 = float(model.loss(xa_d, xb_d, symmetric=False).item())
    model.dual_stream = bool(args.dual_stream) or (not args.eager and not args.single_stream)   # towers = graph branches
    opt = K.FusedAdamW(model, lr=1e-4, weight_decay=0.01, max_grad_norm=None)

    def step():
        opt.zero_grad()
        loss = model.loss(xa_d, xb_d, symmetric=False)
        loss.backward()
        opt.step()
        return loss
    run = step
    if not args.eager:
        # ~60 launches of microsecond kernels: the step is replayed from one hipGraph (training.GraphedTrainStep)
        from clip_dplm_amd.training import GraphedTrainStep
        gstep = GraphedTrainStep(model, opt, lambda a, b: model.loss(a, b, symmetric=False), (xa_d, xb_d))
        run = lambda: gstep(xa_d, xb_d)
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"metric": "seq-pairs/sec, contrastive training step, old/clip.py tiny dual encoder (config 1)",
           "value": round(B * args.steps / dt, 1), "unit": "seq-pairs/s", "n_gpus": 1, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 4), "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
           "config": {"workload": f"BASELINE config 1: old/clip.py RNAProteinCLIPModule (2 layers, d=128, P=128), B={B} "
                                  "random pairs, training step (fwd + one-sided CE + bwd + fused AdamW), "
                                  + ("launches issued eagerly" if args.eager else "step replayed from one hipGraph"),
                      "hip_streams": 2 if model.dual_stream else 1},
           "loss": round(float(loss.item()), 5)}
    if args.full:
        from oracle import clip_ref
        # the dominant kernel's own time: eager steps, outside the timed region
        timer = ops.KernelTimer(("gemm_nt",))
        ops.set_kernel_timer(timer)
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        ops.set_kernel_timer(None)
        gm = timer.summary().get("gemm_nt")
        # CPU oracle: the same training step (>= 10 steps), and the step-0 loss for parity
        ncores = host_threads()
        torch.set_num_threads(ncores)
        sd = {k: v.clone().requires_grad_(True) for k, v in sd0.items()}
        topt = torch.optim.AdamW(list(sd.values()), lr=1e-4, weight_decay=0.01)
        times, loss_or0 = [], None
        for it in range(13):
            t1 = time.perf_counter()
            topt.zero_grad()
            lo = clip_ref.ce_diag(clip_ref.rna_protein_clip_forward(sd, xa, xb)["logits_per_rna_protein"])
            if it == 0:
                loss_or0 = float(lo.item())
            lo.backward()
            topt.step()
            times.append(time.perf_counter() - t1)
        timed = sorted(times[3:])
        cdt = timed[len(timed) // 2]
        flop_step = 3 * 2 * (2 * B * 128 * 128 * 2 + 2 * B * (128 * 256 + 256 * 128))  # fwd + dgrad + wgrad, 2 towers
        ach = gm["work"] / (gm["total_ms"] * 1e-3) / 1e12 if gm else 0.0
        out["roofline"] = {"bound": "mfma",
                           "kernel": "clipk_gemm_nt (launch-latency bound at these sizes: 8.4 MFLOP per launch)",
                           "achieved": round(ach, 3), "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                           "frac": round(ach / MFMA_BF16_PEAK_TFLOPS, 6), "traffic": None,
                           "avg_launch_us": round(gm["avg_us"], 2) if gm else None,
                           "launches": gm["launches"] if gm else 0,
                           "algorithmic_gflop_per_step": round(flop_step / 1e9, 3)}
        out["parity"] = {"loss_gpu": loss_gpu0, "loss_oracle": loss_or0, "loss_abs_err": abs(loss_gpu0 - loss_or0),
                         "bar": 1e-3, "known_answer": 5.915865,
                         "note": "one-sided CE at the initial weights (SURVEY §8c known answer 5.915865)"}
        out["cpu_baseline"] = {"value": round(B / cdt, 1), "unit": "seq-pairs/s", "cores": ncores, "kind": "port",
                               "sample": f"median of {len(timed)} training steps of the CPU oracle (fwd + CE + bwd + "
                                         f"torch AdamW) at B={B}, f32, after 3 warm-up steps; {1e3 * cdt:.2f} ms/step"}
    emit(out)


# ====================================================================================================== notebook
def bench_notebook(args):
    """The one variant the reference trained (current/rna_clip_codes.ipynb:1925-1954, 71.6 M parameters): RNA features
    [32, 48, 120] and RBP features [32, 600, 1280] (the notebook's RBP lengths are 557-2542), ragged NaN padding, one
    TRAINING step = forward + symmetric InfoNCE + backward + clip + fused AdamW (ipynb:2061-2089), dropout 0.
    The encoders attend over the BATCH axis per position and only position 0 is read (App. A-8), so all the work that
    reaches the loss is 32 rows per tower through 3 layers: with the slice the step is bound by reading the f32 weights
    (fwd + dgrad), writing their gradients and the AdamW pass - ~8 passes over 287 MB."""
    import torch

    import clip_dplm_amd as K
    from clip_dplm_amd import ops
    dev = torch.device("cuda:0")
    B, Lr, Lp = args.batch or 32, 48, args.seq_len or 600
    sliced, prec = args.variant.startswith("sliced"), args.variant.split("-")[1]
    torch.manual_seed(0)
    pdrop = float(args.dropout)          # 0 (parity / metric runs) or the notebook's own 0.1
    model = K.RNARBPCLIPModel(rna_dim=120, rbp_dim=1280, projection_dim=512, dropout=pdrop, precision=prec,
                              slice_first_position=sliced)
    nparam = sum(p.numel() for p in model.parameters())
    sd0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(7)
    rna = torch.randn(B, Lr, 120, generator=g)
    rbp = torch.randn(B, Lp, 1280, generator=g)
    lr_ = torch.randint(10, Lr + 1, (B,), generator=g)
    lp_ = torch.randint(Lp // 3, Lp + 1, (B,), generator=g)
    lr_[0], lp_[0] = Lr, Lp
    for i in range(B):
        rna[i, lr_[i]:] = float("nan")
        rbp[i, lp_[i]:] = float("nan")
    model = model.to(dev).eval()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = pdrop                                       # (the heads' nn.Dropout(0.1) of ipynb:1887-1903)
    rna_d, rbp_d = rna.to(dev), rbp.to(dev)
    want_oracle = args.full and not (args.no_parity and args.no_cpu_baseline)
    if want_oracle:
        with torch.no_grad():
            loss_gpu0 = float(model(rna_d, rbp_d)[2].item())  # eval forward: what the oracle computes
    model.train()
    # the two towers as parallel branches of the captured step (default for the replayed step; eager launches are
    # host-bound either way): --single-stream switches it off, --dual-stream forces it for --eager
    model.dual_stream = bool(args.dual_stream) or (not args.eager and not args.single_stream)
    opt = K.FusedAdamW(model, lr=1e-4, weight_decay=0.01, max_grad_norm=1.0)

    def step():
        opt.zero_grad()
        loss = model(rna_d, rbp_d)[2]
        loss.backward()
        opt.step()
        return loss
    run = step
    if not args.eager:
        # the sliced step is ~350 launches of microsecond kernels: replayed from ONE hipGraph (inputs, learning rate and
        # AdamW's bias corrections live in device memory)
        from clip_dplm_amd.training import GraphedTrainStep
        gstep = GraphedTrainStep(model, opt, lambda a, b: model(a, b)[2], (rna_d, rbp_d))
        run = lambda: gstep(rna_d, rbp_d)
    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = run()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # whole-step floor of the sliced model: weights read by fwd and dgrad, gradients written, AdamW's 16 B per parameter
    step_bytes = nparam * 4.0 * 3 + nparam * 16.0
    out = {"metric": "seq-pairs/sec, contrastive training step, RNA-RBP notebook model (rna_clip_codes.ipynb:1925-1954)",
           "value": round(B * args.steps / dt, 1), "unit": "seq-pairs/s", "n_gpus": 1, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 4), "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": prec, "data": "synthetic",
           "config": {"workload": f"RNARBPCLIPModel(120, 1280, 512), {nparam} parameters, rna [{B}, {Lr}, 120] x rbp "
                                  f"[{B}, {Lp}, 1280] with ragged NaN padding, training step (fwd + symmetric InfoNCE + bwd + "
                                  f"clip + fused AdamW), variant {args.variant}, "
                                  + ("launches issued eagerly" if args.eager else "step replayed from one hipGraph"),
                      "hip_streams": 2 if model.dual_stream else 1, "dropout": pdrop},
           "loss": round(float(loss.item()), 5),
           "step_hbm_floor": {"algorithmic_bytes_per_step": int(step_bytes),
                              "ms_at_8TBps": round(step_bytes / 8e12 * 1e3, 4),
                              "frac_of_floor": round(step_bytes / 8e12 / (dt / args.steps), 4),
                              "note": "sliced model only: weights read by forward and dgrad, weight gradients written, "
                                      "AdamW 16 B / parameter"}}
    if args.full:
        timer = ops.KernelTimer()
        ops.set_kernel_timer(timer)
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        ops.set_kernel_timer(None)
        summ = timer.summary()
        dom = max(summ, key=lambda k: summ[k]["total_ms"])
        dv = summ[dom]
        if dv["bytes"] > 0 and prec == "f32":
            ach = dv["bytes"] / (dv["total_ms"] * 1e-3) / 1e9
            out["roofline"] = {"bound": "hbm",
                               "kernel": f"clipk_{dom} (exact-f32 Linear fwd / dgrad / wgrad at M = {B} rows: one pass "
                                         "over the f32 weight per launch)",
                               "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": None,
                               "avg_launch_us": round(dv["avg_us"], 2), "launches": dv["launches"],
                               "algorithmic_bytes_per_launch": round(dv["bytes"] / max(dv["launches"], 1))}
        else:
            ach = dv["work"] / (dv["total_ms"] * 1e-3) / 1e12
            out["roofline"] = {"bound": "mfma", "kernel": f"clipk_{dom}", "achieved": round(ach, 2),
                               "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                               "frac": round(ach / MFMA_BF16_PEAK_TFLOPS, 4), "traffic": None,
                               "avg_launch_us": round(dv["avg_us"], 2), "launches": dv["launches"]}
        out["kernels"] = {k: {"launches_per_step": v["launches"] // 2, "avg_us": round(v["avg_us"], 2),
                              "ms_per_step": round(v["total_ms"] / 2, 4)} for k, v in summ.items()}
    if want_oracle:
        from oracle import model_ref
        ncores = host_threads()
        torch.set_num_threads(ncores)
        sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in sd0.items()}
        t1 = time.perf_counter()
        _, _, lo = model_ref.rnarbp_clip_forward(sd, rna, rbp)
        lo.backward()
        cdt = time.perf_counter() - t1
        out["parity"] = {"loss_gpu": loss_gpu0, "loss_oracle": float(lo.item()), "loss_abs_err": abs(loss_gpu0 - float(lo.item())),
                         "bar": 1e-3, "note": "step-0 loss at the initial weights; oracle = CPU f32 restatement computing "
                                              "EVERY position, as the notebook does"}
        out["cpu_baseline"] = {"value": round(B / cdt, 3), "unit": "seq-pairs/s", "cores": ncores, "kind": "port",
                               "sample": f"ONE forward + backward of the CPU oracle on the same batch (every position, "
                                         f"f32, no optimiser step, no warm-up); {cdt:.2f} s"}
    emit(out)


# ====================================================================================================== c3sim
def bench_c3sim(args):
    """Fused similarity + symmetric CE at one rank's share of config 3: B_l = 512 local pairs against B_g = 4096
    gathered keys, P = 512 (f32 embeddings, exact-f32 MFMA).  A 'step' = forward (row + column LSE) + backward (dA, dB,
    d scale) for this rank; the logits never reach HBM.  HBM-bound by the survey's accounting: algorithmic bytes per
    launch = keys read once (B_g * P * 4) + local rows (B_l * P * 4) (+ B_l * P * 4 written by the gradient kernel)."""
    import torch
    import torch.nn.functional as F
    from clip_dplm_amd import ops
    dev = torch.device("cuda:0")
    Bl, W, P = args.batch or 512, 8, 512
    Bg = Bl * W
    g = torch.Generator().manual_seed(3)
    a = F.normalize(torch.randn(Bg, P, generator=g), dim=-1).to(dev)
    b = F.normalize(torch.randn(Bg, P, generator=g), dim=-1).to(dev)
    sc = torch.tensor([14.2849], device=dev)
    al, bl = a[:Bl].contiguous(), b[:Bl].contiguous()

    def step():
        lr_, pr_ = ops.simce_lse(al, b, sc, label_offset=0)
        lc_, pc_ = ops.simce_lse(bl, a, sc, label_offset=0)
        lrg = lr_.repeat(W)                                   # stand-in for the all-gathered LSE vectors
        lcg = lc_.repeat(W)
        da, _ = ops.simce_grad(al, b, sc, lr_, lcg, 0.5, 0.5, 1.0 / Bg, label_offset=0)
        db, _ = ops.simce_grad(bl, a, sc, lc_, lrg, 0.5, 0.5, 1.0 / Bg, label_offset=0)
        return da, db

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(4)]
    tl, tg = 0.0, 0.0
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ev[0][0].record(); l1 = ops.simce_lse(al, b, sc); ev[0][1].record()
        ev[1][0].record(); l2 = ops.simce_lse(bl, a, sc); ev[1][1].record()
        lrg, lcg = l1[0].repeat(W), l2[0].repeat(W)
        ev[2][0].record(); ops.simce_grad(al, b, sc, l1[0], lcg, 0.5, 0.5, 1.0 / Bg); ev[2][1].record()
        ev[3][0].record(); ops.simce_grad(bl, a, sc, l2[0], lrg, 0.5, 0.5, 1.0 / Bg); ev[3][1].record()
        torch.cuda.synchronize()
        tl += ev[0][0].elapsed_time(ev[0][1]) + ev[1][0].elapsed_time(ev[1][1])
        tg += ev[2][0].elapsed_time(ev[2][1]) + ev[3][0].elapsed_time(ev[3][1])
    dt = time.perf_counter() - t0
    n = 2 * args.steps
    lse_us, grad_us = 1e3 * tl / n, 1e3 * tg / n
    bytes_lse = (Bg + Bl) * P * 4 + 2 * Bl * 4
    bytes_grad = (Bg + Bl) * P * 4 + Bl * P * 4 + (Bl + Bg) * 4
    flop_lse = 2.0 * Bl * Bg * P
    out = {"metric": "seq-pairs/sec/rank, fused similarity + symmetric CE fwd+bwd at the config-3 shape",
           "value": round(Bl * args.steps / dt, 1), "unit": "seq-pairs/s", "n_gpus": 1, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 4), "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": f"BASELINE config 3, one rank's loss block: {Bl} local pairs x {Bg} gathered keys, P={P}, "
                                  "simce_lse x2 + simce_grad x2 (host-synchronised per step)"},
           # the fusion removed the logits from HBM: what binds the kernel is its 2 * Bl * Bg * P exact-f32 MFMA FLOP
           "roofline": {"bound": "mfma", "kernel": "simce_lse_tiled_kernel (exact-f32 MFMA similarity + online LSE)",
                        "achieved": round(flop_lse / (lse_us * 1e-6) / 1e12, 2), "peak": MFMA_F32_PEAK_TFLOPS,
                        "unit": "TFLOP/s", "frac": round(flop_lse / (lse_us * 1e-6) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4),
                        "traffic": None, "avg_launch_us": round(lse_us, 2), "algorithmic_bytes_per_launch": bytes_lse,
                        "frac_hbm_algorithmic": round(bytes_lse / (lse_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 4),
                        "peak_note": "dense f32 MFMA peak (v_mfma_f32_32x32x2_f32: 256 FLOP/clk/CU x 256 CUs x 2.4 GHz)"},
           "kernels": {"simce_lse": {"avg_us": round(lse_us, 2), "GBps": round(bytes_lse / (lse_us * 1e-6) / 1e9, 1)},
                       "simce_grad": {"avg_us": round(grad_us, 2), "GBps": round(bytes_grad / (grad_us * 1e-6) / 1e9, 1),
                                      "f32_mfma_tflops": round(2 * flop_lse / (grad_us * 1e-6) / 1e12, 1)}}}
    if args.full:
        out["parity"] = c3sim_parity(al, bl, a, b, sc, Bl, Bg)
    emit(out)


def c3sim_parity(al, bl, a, b, sc, Bl, Bg):
    """This rank's share of the global symmetric loss from the fused kernels against the CPU oracle on the MATERIALISED
    logits block (oracle/clip_ref.py ce_diag arithmetic, f64): 0.5 * (row CE of the local rows vs all keys + column CE
    of the local columns vs all rows)."""
    import torch
    from clip_dplm_amd import ops
    lr_, pr_ = ops.simce_lse(al, b, sc, label_offset=0)
    lc_, pc_ = ops.simce_lse(bl, a, sc, label_offset=0)
    got = 0.5 * ((lr_ - pr_).mean() + (lc_ - pc_).mean()).item()
    A, Bm, s = a.double().cpu(), b.double().cpu(), float(sc.item())
    S_r = (A[:Bl] @ Bm.t()) * s                               # local rows x all keys
    S_c = (Bm[:Bl] @ A.t()) * s                               # local columns (as rows) x all rows
    want = 0.5 * ((torch.logsumexp(S_r, 1) - S_r[:, :Bl].diagonal()).mean() +
                  (torch.logsumexp(S_c, 1) - S_c[:, :Bl].diagonal()).mean()).item()
    return {"loss_gpu": got, "loss_oracle": want, "loss_abs_err": abs(got - want), "bar": 1e-5,
            "note": f"rank 0's {Bl} rows / columns of the {Bg}-pair symmetric InfoNCE; oracle = f64 CE on the materialised "
                    "logits block (oracle/clip_ref.ce_diag arithmetic)"}


# ====================================================================================================== c5
def bench_c5(args):
    """ICNN transport system at its factory dims (512 / [512, 256]): eval-mode transport maps T(x) = dPsi/dx of the three
    maps for B samples.  HBM accounting: 4 KiB per sample and map (x in, T out, f32) + 3.2 MB of weights."""
    import torch
    from clip_dplm_amd import icnn
    dev = torch.device("cuda:0")
    B = args.batch or 4096
    torch.manual_seed(0)
    model = icnn.create_transport_system(512, 512, 512).to(dev).eval()
    g = torch.Generator().manual_seed(0)
    cell, pert, prot = (torch.randn(B, 512, generator=g).to(dev) for _ in range(3))
    if args.full:
        for _ in range(args.warmup):
            model(cell, pert, prot)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out_ = model(cell, pert, prot)
        torch.cuda.synchronize()
        dt_eager = time.perf_counter() - t0
    # launch-bound in eager mode (~45 small launches per step): replay the same launches from one hipGraph, the three
    # maps as three parallel branches of it (--single-stream: one chain)
    model.multi_stream = not args.single_stream
    graphed = icnn.GraphedTransport(model, cell, pert, prot)
    for _ in range(args.warmup):
        graphed(cell, pert, prot)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out_g = graphed(cell, pert, prot)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    per_map_bytes = B * 512 * 4 * 2 + 0.79e6 * 4
    flop = 3 * B * 2.0 * 2 * (512 * 512 + 2 * 256 * 512)              # three maps, forward + input-gradient products
    ach = 3 * per_map_bytes * args.steps / dt / 1e9
    out = {"metric": "samples/sec, ICNN triple transport maps (eval)", "value": round(B * args.steps / dt, 1),
           "unit": "samples/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(1e3 * dt / args.steps, 4), "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": f"BASELINE config 5: create_transport_system(512, 512, 512), hidden [512, 256], B={B}, "
                                  "three eval-mode transport maps per step"},
           # exact-f32 matrix work (2.1 MFLOP per sample and map): the f32 matrix pipe is the bound, not HBM
           "roofline": {"bound": "mfma", "kernel": "ICNN transport map (whole op: all launches of the three maps, hipGraph "
                                                   "replay; gemm_f32_kernel dominates)",
                        "achieved": round(flop * args.steps / dt / 1e12, 2), "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(flop * args.steps / dt / 1e12 / MFMA_F32_PEAK_TFLOPS, 4), "traffic": None,
                        "algorithmic_bytes_per_step": int(3 * per_map_bytes),
                        "frac_hbm_algorithmic": round(ach / HBM_PEAK_GBS, 5),
                        "peak_note": "dense f32 MFMA peak (v_mfma_f32_32x32x2_f32: 256 FLOP/clk/CU x 256 CUs x 2.4 GHz)"}}
    if args.full:
        assert all(torch.equal(out_g[k], out_[k]) for k in out_)      # same kernels, same inputs: same bits
        # parity: the three maps of the first 64 samples against the CPU oracle's autograd-of-autograd
        from oracle import icnn_ref
        sd_c = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        srcs = {"cell_to_pert": cell, "cell_to_protein": cell, "pert_to_protein": pert}
        perr = 0.0
        for name, src in srcs.items():
            ref = icnn_ref.single_cell_transport(src[:64].cpu(), sd_c, name, 2)
            perr = max(perr, (out_[name][:64].cpu() - ref).abs().max().item())
        out["parity"] = {"max_abs_err": perr, "bar": 2e-4, "samples": 64,
                         "note": "T(x) of the three maps (LayerNorm'ed, O(1)) vs oracle/icnn_ref.single_cell_transport "
                                 "(CPU f32 autograd)"}
        out["eager_ms_per_step"] = round(1e3 * dt_eager / args.steps, 4)
    emit(out)


_JSON_FD = None


def emit(obj) -> None:
    """The ONE JSON line, on the process's original stdout."""
    line = (json.dumps(obj) + "\n").encode()
    if _JSON_FD is None:
        sys.stdout.write(line.decode()); sys.stdout.flush()
    else:
        os.write(_JSON_FD, line)


def main():
    global _JSON_FD
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        if args.config not in ("c2", "c4", "stub"):
            raise SystemExit(f"--config {args.config} is a one-GPU kernel bench")
        sys.exit(self_launch(args))
    # stdout carries exactly one JSON line: library chatter (RCCL prints a version banner on stdout at the first
    # collective) is sent to stderr by pointing fd 1 there; the JSON goes to a duplicate of the original stdout
    sys.stdout.flush()
    _JSON_FD = os.dup(1)
    os.dup2(2, 1)
    if args.config in ("c2", "c4"):
        bench_clip(args)
    elif args.config == "stub":
        bench_stub(args)
    elif args.config == "c1":
        bench_c1(args)
    elif args.config == "c3sim":
        bench_c3sim(args)
    elif args.config == "notebook":
        bench_notebook(args)
    else:
        bench_c5(args)


if __name__ == "__main__":
    main()
