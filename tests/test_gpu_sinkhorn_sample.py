"""GPU: the plan sampler (include/clipk.h: clipk_sim_sample; ops.sim_sample; SinkhornResult.sample_targets / sample_pairs;
flow.SchrodingerBridgeConditionalFlowMatcher) against the restatement of tests/sinkhorn_sample_ref.py.

The winning value `score` follows the rule of test_gpu_sinkhorn.py (`_close`, restated here): the f64 restatement is the
reference, the kernel may deviate from it by at most 8 x the deviation of the f32 restatement on the same inputs, with a
floor of 64 * 2^-24 x the magnitude.  Call that bound B.  The drawn index must equal the f64 arg max on every row whose
f64 top-two gap exceeds 2 B; on the other rows the chosen key's f64 value must lie within 2 B of the maximum, and such
rows may be at most 1 % of a case's 1000 rows (an arg max is only as well defined as its runner-up is far).  The measured
figures are printed before each assertion."""
import math

import numpy as np
import pytest
import torch

from clip_dplm_amd import flow, ops, ot

import sinkhorn_sample_ref as sref

ref = sref.ref
pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F64, F32 = torch.float64, torch.float32
SEED = 12345


def _bound(r64, r32):
    dev_32, mag = float((r32.double() - r64).abs().max()), float(r64.abs().max())
    return max(8 * dev_32, 64 * U * mag), dev_32, mag


def _close(name, got, r64, r32):
    got, r64, r32 = (torch.as_tensor(t).detach().double().cpu() for t in (got, r64, r32))
    assert got.shape == r64.shape, (name, got.shape, r64.shape)
    assert torch.isfinite(got).all(), name
    dev_k = float((got - r64).abs().max())
    bound, dev_32, mag = _bound(r64, r32)
    print(f"{name}: kernel {dev_k:.3e}  f32 restatement {dev_32:.3e}  magnitude {mag:.3e}  bound {bound:.3e}")
    assert dev_k <= bound, (name, dev_k, bound)
    return bound


def _scalar(v, dev):
    return torch.tensor([v], dtype=F32, device=dev)


def _check_draws(tag, idx, score, d64, d32, x, y, scale, bias, seed, streams, n=None):
    """idx / score of the kernel for the first n rows of the restatements d64, d32 (x, y, bias: the restatement's inputs
    on its device; streams: each row's stream id)."""
    n = len(idx) if n is None else n
    idx = idx.cpu()
    assert idx.dtype == torch.int64 and idx.shape == (n,)
    assert int(idx.min()) >= 0 and int(idx.max()) < y.shape[0], tag
    s64, s32, i64, gap = d64.score[:n].cpu(), d32.score[:n].cpu(), d64.idx[:n].cpu(), d64.gap[:n].cpu()
    if score is not None:
        B = _close(f"score {tag}", score, s64, s32)
    else:
        B = _bound(s64, s32)[0]
    near = gap <= 2 * B
    wrong = idx != i64
    print(f"idx {tag}: {int(wrong.sum())} of {n} rows differ from the f64 arg max, {int(near.sum())} rows have a top-two "
          f"gap within 2 B = {2 * B:.3e}; the f32 restatement differs on {int((d32.idx[:n].cpu() != i64).sum())}")
    assert not bool((wrong & ~near).any()), (tag, "a row with a clear winner drew another key")
    if bool(wrong.any()):
        rows = torch.nonzero(wrong).reshape(-1)
        rd = rows.to(x.device)
        got, best = sref.values_at(x[rd], y, scale, bias, seed, [streams[int(r)] for r in rows], idx[rows])
        assert bool((best.cpu() - got.cpu() <= 2 * B).all()), (tag, "the drawn key is not within 2 B of the maximum")
    return B


# ------------------------------------------------------------------------------------------------ 1: kernel parity
CASES = [(P, Ny, True) for P in (4, 60, 768) for Ny in (1, 63, 65, 4097, 100003)] + [(60, 4097, False)]


@pytest.mark.parametrize("P,Ny,biased", CASES)
def test_kernel_parity(dev, P, Ny, biased):
    """ops.sim_sample: rows are independent given the stream id, so one reference of 1000 rows serves Mx = 1, 63, 65,
    1000.  Unit clouds, scale 10 and a bias uniform in +-20; the last case has no bias and scale 4."""
    g = torch.Generator().manual_seed(1000 * P + Ny)
    x_all, y = ref.unit_clouds(1000, Ny, P, 5 * P + Ny)
    scale = 10.0 if biased else 4.0
    bias = (torch.rand(Ny, generator=g, dtype=F64) * 40 - 20).float() if biased else None
    if Ny > 4097:                                   # the restatement of 1000 x 100003 problems on the device: seconds less
        x_all, y, bias = x_all.to(dev), y.to(dev), bias.to(dev)
    d64 = sref.draw(x_all, y, scale, bias, SEED, 0, F64)
    d32 = sref.draw(x_all, y, scale, bias, SEED, 0, F32)
    B_all = _bound(d64.score.cpu(), d32.score.cpu())[0]
    near = int((d64.gap.cpu() <= 2 * B_all).sum())
    print(f"P={P} Ny={Ny}: {near} of 1000 rows have a top-two gap within 2 B = {2 * B_all:.3e}")
    assert near <= 10
    yd, sd = y.to(dev), _scalar(scale, dev)
    bd = None if bias is None else bias.to(dev)
    streams = list(range(1000))
    split_seen = False
    for Mx in (1, 63, 65, 1000):
        tag = f"Mx={Mx} Ny={Ny} P={P}"
        xd = x_all[:Mx].to(dev)
        split_seen |= ops.sim_lse_bias_plan(Mx, Ny)[1] > 1
        idx, score = ops.sim_sample(xd, yd, sd, bias=bd, seed=SEED, want_score=True)
        assert score.dtype == F32 and score.shape == (Mx,)
        _check_draws(tag, idx, score, d64, d32, x_all, y, scale, bias, SEED, streams)
        # two runs, and the call without the score, give the same bits
        idx2, score2 = ops.sim_sample(xd, yd, sd, bias=bd, seed=SEED, want_score=True)
        assert torch.equal(idx, idx2) and torch.equal(score, score2), tag
        assert torch.equal(idx, ops.sim_sample(xd, yd, sd, bias=bd, seed=SEED)), tag
        # the seed and the offset read from device memory
        st = torch.tensor([SEED, 0], dtype=torch.int64, device=dev)
        assert torch.equal(idx, ops.sim_sample(xd, yd, sd, bias=bd, seed=st)), tag
    if Ny >= 4097:
        assert split_seen, "no shape of this case splits the key range"
    # ---- geometry independence: rows 64..127 of the 1000-row launch against a launch of those rows alone (another grid,
    # another key split), bit for bit
    part_i, part_s = ops.sim_sample(x_all[64:128].to(dev), yd, sd, bias=bd, seed=SEED, stream_offset=64, want_score=True)
    assert torch.equal(part_i, idx[64:128]) and torch.equal(part_s, score[64:128])
    st = torch.tensor([SEED, 64], dtype=torch.int64, device=dev)
    assert torch.equal(part_i, ops.sim_sample(x_all[64:128].to(dev), yd, sd, bias=bd, seed=st))
    if not biased:
        other = ops.sim_sample(x_all.to(dev), yd, sd, seed=SEED + 1)
        changed = int((other != idx).sum())
        print(f"another seed changes {changed} of 1000 indices")
        assert changed > 500


@pytest.mark.parametrize("seed,stream0", [(-1, (1 << 32) - 32), ((1 << 63) + 5, (1 << 40) + 1), (7 << 32, -64)])
def test_wide_seeds_and_streams(dev, seed, stream0):
    """Both halves of the 64-bit seed and of the 64-bit stream id reach the generator: streams across 2^32, beyond it and
    wrapping through 0; Python ints are taken modulo 2^64."""
    x, y = ref.unit_clouds(65, 63, 8, 3)
    d64 = sref.draw(x, y, 4.0, None, seed, stream0, F64)
    d32 = sref.draw(x, y, 4.0, None, seed, stream0, F32)
    idx, score = ops.sim_sample(x.to(dev), y.to(dev), _scalar(4.0, dev), seed=seed, stream_offset=stream0, want_score=True)
    _check_draws(f"seed={seed} stream0={stream0}", idx, score, d64, d32, x, y, 4.0, None, seed,
                 [stream0 + k for k in range(65)])
    assert int((d64.idx != sref.draw(x, y, 4.0, None, seed & 0xFFFFFFFF, stream0, F64).idx).sum()) > 32


# ------------------------------------------------------------------------------------------------ 2: ot level
@pytest.mark.parametrize("eps", [0.5, 0.05])
def test_sample_targets_on_solved_plans(dev, eps):
    """130 x 257 x 64 after 100 iterations: the restatement is fed the result's own v (the conditional needs no u)."""
    M, N, P = 130, 257, 64
    x, y = ref.unit_clouds(M, N, P, M + N + P)
    r = ot.sinkhorn(x.to(dev), y.to(dev), eps=eps, n_iters=100, tol=None)
    v = r.v.cpu()
    scale = float(r._scale.cpu())
    d64, d32 = sref.draw(x, y, scale, v, 99, 0, F64), sref.draw(x, y, scale, v, 99, 0, F32)
    j = r.sample_targets(seed=99)
    _check_draws(f"sample_targets eps={eps}", j, None, d64, d32, x, y, scale, v, 99, list(range(M)))
    assert torch.equal(j, r.sample_targets(rows=torch.arange(M, device=dev), seed=99))
    # given rows, with repeats: draw k uses stream k
    rows = torch.tensor([5, 5, 129, 0, 64, 5, 63], dtype=torch.int64)
    e64, e32 = sref.draw(x[rows], y, scale, v, 99, 0, F64), sref.draw(x[rows], y, scale, v, 99, 0, F32)
    _check_draws(f"sample_targets(rows) eps={eps}", r.sample_targets(rows.to(dev), seed=99), None, e64, e32, x[rows], y,
                 scale, v, 99, list(range(len(rows))))
    with pytest.raises(IndexError):
        r.sample_targets(torch.tensor([0, M], device=dev))


def test_draw_statistics(dev):
    """37 x 63 x 12, every row drawn 2000 times (74000 streams): column counts and per-row means against the f64 plan.
    The f64 restatement alone passes both checks with this seed (test_sinkhorn_sample_host.py holds it to that)."""
    x, y, eps, rows, seed = sref.statistics_problem()
    r = ot.sinkhorn(x.to(dev), y.to(dev), eps=eps, n_iters=100, tol=None)
    j = r.sample_targets(rows.to(dev), seed=seed).cpu()
    r64 = ref.solve(x, y, eps, n_iters=100)
    sref.check_statistics(j, rows, y, r64)
    # the same draws from the restatement fed the result's own v: the same rule as everywhere
    v, scale = r.v.cpu(), float(r._scale.cpu())
    n = 4096
    d64, d32 = sref.draw(x[rows[:n]], y, scale, v, seed, 0, F64, rows=n), sref.draw(x[rows[:n]], y, scale, v, seed, 0, F32, rows=n)
    _check_draws("statistics draws", j[:n], None, d64, d32, x[rows[:n]], y, scale, v, seed, list(range(n)))


def test_sample_pairs(dev):
    M, N, P, n = 37, 63, 12, 20000
    x, y = ref.unit_clouds(M, N, P, 17)
    a = ref.random_weights(M, 3)
    r = ot.sinkhorn(x.to(dev), y.to(dev), eps=0.5, a=a.to(dev), n_iters=100, tol=None)
    gen = torch.Generator(device=dev).manual_seed(5)
    i, j = r.sample_pairs(n, seed=8, generator=gen)
    assert i.shape == j.shape == (n,) and i.dtype == j.dtype == torch.int64
    assert 0 <= int(i.min()) and int(i.max()) < M and 0 <= int(j.min()) and int(j.max()) < N
    assert torch.equal(j, r.sample_targets(i, seed=8))
    chi = sref.chi_square(np.bincount(i.cpu().numpy(), minlength=M), a.double().numpy() / float(a.double().sum()))
    bar = 36 + 5 * math.sqrt(72)
    print(f"i against a: chi-square {chi:.1f} at 36 degrees of freedom (threshold {bar:.1f})")
    assert chi < bar
    # defaults: n = M, uniform weights
    r2 = ot.sinkhorn(x.to(dev), y.to(dev), eps=0.5, n_iters=10, tol=None)
    i2, j2 = r2.sample_pairs()
    assert i2.shape == j2.shape == (M,) and int(i2.max()) < M and int(j2.max()) < N


# ------------------------------------------------------------------------------------------------ 3: the matcher
def test_matcher(dev):
    M, N, P, sigma = 130, 257, 64, 0.5
    x0, x1 = ref.unit_clouds(M, N, P, 23)
    x0d, x1d = x0.to(dev), x1.to(dev)
    m = flow.SchrodingerBridgeConditionalFlowMatcher(sigma, n_iters=30)
    gen = torch.Generator(device=dev).manual_seed(1)
    t, xt, ut, noise, (i, j) = m.sample_location_and_conditional_flow(x0d, x1d, return_noise=True, return_indices=True,
                                                                      seed=31, generator=gen)
    assert t.shape == (M,) and xt.shape == ut.shape == noise.shape == (M, P) and i.shape == j.shape == (M,)
    assert 0 <= float(t.min()) and float(t.max()) < 1
    wx, wu = flow.conditional_flow(x0d[i], x1d[j], t, noise, sigma)
    assert torch.equal(xt, wx) and torch.equal(ut, wu)
    # against the formulae in f64
    rx, ru = flow.conditional_flow(x0d[i].double(), x1d[j].double(), t.double(), noise.double(), sigma)
    assert float((xt - rx).abs().max()) < 1e-5 and float((ut - ru).abs().max()) <= 1e-5 * float(ru.abs().max()) + 1e-5
    # j is the restatement's draw on the plan of the same solve (eps = 2 sigma^2)
    r = ot.sinkhorn(x0d, x1d, eps=2 * sigma * sigma, n_iters=30, tol=None)
    ic = i.cpu()
    v, scale = r.v.cpu(), float(r._scale.cpu())
    assert abs(scale - 2.0 / (2 * sigma * sigma)) < 1e-6
    d64, d32 = sref.draw(x0[ic], x1, scale, v, 31, 0, F64), sref.draw(x0[ic], x1, scale, v, 31, 0, F32)
    _check_draws("matcher j", j, None, d64, d32, x0[ic], x1, scale, v, 31, list(range(M)))
    # a given t is returned as it is; without the flags three values come back
    tt = torch.linspace(0.1, 0.9, M, device=dev)
    out = m.sample_location_and_conditional_flow(x0d, x1d, t=tt, seed=31)
    assert len(out) == 3 and out[0] is tt
    loss = flow.flow_matching_loss(torch.zeros_like(out[2]), out[2])
    assert abs(float(loss) - float((out[2].double() ** 2).mean())) < 1e-5 * float(loss)


def test_solve_and_sample_are_capturable(dev):
    """A fixed-iteration solve plus a draw with the seed in device memory, captured once: replayed with the seed bumped it
    gives the eager call's bits for that seed (the pattern of test_fixed_iteration_solve_is_capturable)."""
    M, N, P = 130, 257, 64
    x0, y0 = ref.unit_clouds(M, N, P, 41)
    sx, sy = x0.to(dev), y0.to(dev)
    seed_t = torch.tensor([100, 0], dtype=torch.int64, device=dev)

    def run():
        r = ot.sinkhorn(sx, sy, eps=0.5, n_iters=10, tol=None)
        return r.sample_targets(seed=seed_t)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph, keep = torch.cuda.CUDAGraph(), []
    with ops.owned_by_capture(keep), torch.cuda.graph(graph):
        out = run()
    eager = ot.sinkhorn(sx, sy, eps=0.5, n_iters=10, tol=None)
    seen = []
    for s in (100, 101, 102, 100):
        seed_t.copy_(torch.tensor([s, 0], dtype=torch.int64))
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone()
        assert torch.equal(got, eager.sample_targets(seed=s)), s
        seen.append(got)
    assert torch.equal(seen[0], seen[3]) and int((seen[0] != seen[1]).sum()) > M // 4
