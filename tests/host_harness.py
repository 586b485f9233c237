"""Shared scaffold of the CPU tests of the host logic (loss.py's rank bookkeeping, distributed.py, optim.py).

The HIP kernels cannot run without a device, so torch restatements stand in for clip_dplm_amd.ops.*: tests/ops_emulator.py
for the plain ops, tests/class_aware_ref.py and tests/hard_negative_ref.py for the ops of the two InfoNCE variants.  A
plain module, imported like those (not a conftest): the stand-in installation, the seeded unit-norm inputs and the gloo
spawn scaffold, which takes each test's own per-rank body.
"""
import os
import sys
import tempfile

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def install(set_attr=setattr):
    """Route clip_dplm_amd.ops.* to the stand-ins.  A spawned rank keeps them for its lifetime; the pytest process passes
    monkeypatch.setattr, so that the kernels are back for the tests that run after this one."""
    sys.path[:0] = [ROOT, HERE]
    import class_aware_ref
    import hard_negative_ref
    import ops_emulator
    from clip_dplm_amd import ops
    for n in ops_emulator._NAMES:
        if hasattr(ops, n) and n != "KernelTimer":
            set_attr(ops, n, getattr(ops_emulator, n))
    for ref, names in ((class_aware_ref, ("simce_lse_cls", "simce_grad_cls")),
                       (hard_negative_ref, ("simce_lse_hard", "simce_grad_hard"))):
        for n in names:
            set_attr(ops, n, getattr(ref, n))


def unit(n, p, seed, dtype=torch.float32):
    """Seeded [n, p] rows of unit norm (drawn and normalised in f64)."""
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n, p, generator=g, dtype=torch.float64), dim=-1).to(dtype)


def trap_calls(set_attr, names):
    """Wrap the installed ops `names`; returns the list that receives a name at each of its calls."""
    from clip_dplm_amd import ops
    calls = []

    def trap(name, fn):
        return lambda *args, **kw: (calls.append(name), fn(*args, **kw))[1]
    for n in names:
        set_attr(ops, n, trap(n, getattr(ops, n)))
    return calls


def spy_gathers(loss_module):
    """Record (dtype, shape) of every tensor loss._gather_cat is given from here on; returns the list."""
    gathered = []
    plain_gather = loss_module._gather_cat

    def spy(t, group):
        gathered.append((t.dtype, tuple(t.shape)))
        return plain_gather(t, group)
    loss_module._gather_cat = spy
    return gathered


def clip_loss_cases(cases, log, rank, world, Bl=12, P=16, Nc=5):
    """This rank's rows of a seeded global batch (class ids i % 5: every class has members on every rank) through
    clip_loss and backward, once per case = (with class ids, with cache, clip_loss keywords).  log: a list some spy
    appends to, emptied before each case.  Returns per case (loss, da, db, dscale, the log's entries)."""
    from clip_dplm_amd.loss import clip_loss
    a_g, b_g = unit(world * Bl, P, 1), unit(world * Bl, P, 2)
    ids_g = torch.arange(world * Bl) % 5
    sl = slice(rank * Bl, (rank + 1) * Bl)
    out = []
    for with_ids, with_cache, kw in cases:
        del log[:]
        a, b = a_g[sl].clone().requires_grad_(True), b_g[sl].clone().requires_grad_(True)
        s = torch.tensor(14.2849, requires_grad=True)
        loss = clip_loss(a, b, s, group=dist.group.WORLD if world > 1 else None, cache=unit(Nc, P, 3) if with_cache else None,
                         class_ids=ids_g[sl].clone() if with_ids else None, **kw)
        loss.backward()
        out.append((loss.item(), a.grad.clone(), b.grad.clone(), s.grad.clone(), list(log)))
    return out


def _rank_main(rank, world, initfile, results, body):
    torch.set_num_threads(1)
    install()
    dist.init_process_group("gloo", init_method=f"file://{initfile}", rank=rank, world_size=world)
    try:
        results[rank] = body(rank, world)
    finally:
        dist.destroy_process_group()


def run_ranks(body, world=2):
    """body(rank, world) -> picklable result (a module-level function), run in `world` spawned gloo ranks with the
    stand-ins installed.  Returns the results in rank order."""
    mp.set_sharing_strategy("file_system")
    with tempfile.TemporaryDirectory() as d:
        results = mp.Manager().dict()
        mp.spawn(_rank_main, args=(world, os.path.join(d, "init"), results, body), nprocs=world, join=True)
        return [results[r] for r in range(world)]
