"""GPU: the exact coupling (include/clipk.h: clipk_sim_top2_bias, clipk_auction_rounds; ops.sim_top2_bias,
ops.auction_rounds; ot.exact_assignment, ot.wasserstein2_exact; flow.ExactOptimalTransportConditionalFlowMatcher) against
the restatement of tests/auction_ref.py and scipy's optimum on the f64 matrix.

Values follow the rule of test_gpu_sinkhorn_sample.py: the f64 restatement is the reference, the kernel may deviate from it
by at most B = max(8 x the deviation of the f32 restatement on the same inputs, 64 * 2^-24 x the magnitude).  Order
statistics are 1-Lipschitz in the sup norm, so the runner-up and with it the top-two gap stay within 2 B on every row, also
where winners swap; the arg max must be the f64 one wherever the f64 gap exceeds 2 B, elsewhere the chosen key's f64 value
must lie within 2 B of the maximum.  For a solve B is taken on the values the rows bid on, z = 2 x y^T + bias with the
solve's final bias: the matching's mean cost and the dual bound are means of such values (and of squared norms formed in
f64), so they inherit the bound.  The measured figures are printed before each assertion."""
import math

import numpy as np
import pytest
import torch

from clip_dplm_amd import flow, ops, ot

import auction_ref as aref

ref = aref.ref
pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F64, F32 = torch.float64, torch.float32


def _bound(r64, r32):
    dev_32, mag = float((r32.double() - r64).abs().max()), float(r64.abs().max())
    return max(8 * dev_32, 64 * U * mag), dev_32, mag


def _scalar(v, dev):
    return torch.tensor([v], dtype=F32, device=dev)


def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


# ------------------------------------------------------------------------------------------------ 1: top-two parity
def _check_top2(tag, got, d64, d32, x, y, scale, bias, rows=None):
    """got = (idx, best, gap) of the kernel for the rows `rows` (default: the first len(idx)) of the restatements."""
    idx, best, gap = (t.cpu() for t in got)
    n = len(idx)
    sel = torch.arange(n) if rows is None else rows.cpu().long()
    assert idx.dtype == torch.int32 and best.dtype == gap.dtype == F32 and best.shape == gap.shape == (n,)
    Ny = y.shape[0]
    assert int(idx.min()) >= 0 and int(idx.max()) < Ny, tag
    b64, b32, g64, i64 = d64.best.cpu()[sel], d32.best.cpu()[sel], d64.gap.cpu()[sel], d64.idx.cpu()[sel]
    B, dev_32, mag = _bound(d64.best.cpu(), d32.best.cpu())
    dev_best = float((best.double() - b64).abs().max())
    print(f"best {tag}: kernel {dev_best:.3e}  f32 restatement {dev_32:.3e}  magnitude {mag:.3e}  bound {B:.3e}")
    assert torch.isfinite(best).all() and dev_best <= B, (tag, dev_best, B)
    if Ny == 1:
        assert bool((torch.isinf(gap) & (gap > 0)).all()), tag
    else:
        dev_gap = float((gap.double() - g64).abs().max())
        print(f"gap {tag}: kernel {dev_gap:.3e}  bound 2 B = {2 * B:.3e}")
        assert torch.isfinite(gap).all() and float(gap.min()) >= 0 and dev_gap <= 2 * B, (tag, dev_gap, 2 * B)
    near = g64 <= 2 * B
    wrong = idx.long() != i64
    print(f"idx {tag}: {int(wrong.sum())} of {n} rows differ from the f64 arg max, {int(near.sum())} rows have a gap within 2 B")
    assert not bool((wrong & ~near).any()), (tag, "a row with a clear winner chose another key")
    if bool(wrong.any()):
        r = torch.nonzero(wrong).reshape(-1)
        xr = x[sel[r].to(x.device)]
        v, m = aref.values_at(xr, y, scale, bias, idx[r].to(x.device))
        assert bool((m.cpu() - v.cpu() <= 2 * B).all()), (tag, "the chosen key is not within 2 B of the maximum")
    return B


@pytest.mark.parametrize("P", [4, 60, 768])
@pytest.mark.parametrize("Ny", [1, 2, 63, 65, 4097, 100003])
def test_top2_parity(dev, P, Ny):
    """Unit clouds, scale 10, bias uniform in +-20 / sqrt(P); rows are independent, so one reference of 1000 rows serves
    Mx = 1, 63, 65, 1000."""
    g = torch.Generator().manual_seed(1000 * P + Ny)
    x_all, y = ref.unit_clouds(1000, Ny, P, 5 * P + Ny)
    scale = 10.0
    bias = ((torch.rand(Ny, generator=g, dtype=F64) * 40 - 20) / math.sqrt(P)).float()
    if Ny > 4097:                                   # the restatement of 1000 x 100003 problems on the device: seconds less
        x_all, y, bias = x_all.to(dev), y.to(dev), bias.to(dev)
    d64 = aref.top2(x_all, y, scale, bias, F64)
    d32 = aref.top2(x_all, y, scale, bias, F32)
    B_all = _bound(d64.best.cpu(), d32.best.cpu())[0]
    if Ny >= 2:
        near = int((d64.gap.cpu() <= 2 * B_all).sum())
        winners = int(d64.idx.unique().numel())
        print(f"P={P} Ny={Ny}: {near} of 1000 rows have a gap within 2 B = {2 * B_all:.3e}; {winners} distinct winners")
        assert near <= 10 and winners >= 2
    xd, yd, bd, sd = x_all.to(dev), y.to(dev), bias.to(dev), _scalar(scale, dev)
    full = None
    for Mx in (1, 63, 65, 1000):
        tag = f"Mx={Mx} Ny={Ny} P={P}"
        xm = xd[:Mx].contiguous()
        got = ops.sim_top2_bias(xm, yd, sd, bias=bd)
        _check_top2(tag, got, d64, d32, x_all, y, scale, bias)
        again = ops.sim_top2_bias(xm, yd, sd, bias=bd)                # two runs give the same bits
        assert all(torch.equal(a, b) for a, b in zip(got, again)), tag
        only = ops.sim_top2_bias(xm, yd, sd, bias=bd, want_best=False, want_gap=False)
        assert only[1] is None and only[2] is None and torch.equal(only[0], got[0]), tag
        full = got
    nqb, ks = ops.sim_top2_bias_plan(1000, Ny)
    assert nqb == 16 and (ks > 1 if Ny >= 4097 else True)
    # ---- geometry independence: rows 64..127 of the 1000-row launch against a launch of those rows alone, bit for bit
    part = ops.sim_top2_bias(xd[64:128].contiguous(), yd, sd, bias=bd)
    assert all(torch.equal(a, b[64:128]) for a, b in zip(part, full))
    # ---- a row list: a shuffled subset with repeats, n_active below its length, against the same rows launched densely
    rows = torch.randperm(1000, generator=torch.Generator().manual_seed(Ny + P))[:300]
    rows[7] = rows[3]
    rd = rows.to(device=dev, dtype=torch.int32)
    n_act = 201
    out = (torch.full((300,), -7, dtype=torch.int32, device=dev), torch.full((300,), -7.0, device=dev),
           torch.full((300,), -7.0, device=dev))
    got = ops.sim_top2_bias(xd, yd, sd, bias=bd, rows=rd, n_active=_i32([n_act], dev), out=out)
    assert got[0] is out[0] and got[1] is out[1] and got[2] is out[2]
    dense = ops.sim_top2_bias(xd[rows.to(dev)].contiguous(), yd, sd, bias=bd)
    for a, b in zip(got, dense):
        assert torch.equal(a[:n_act], b[:n_act]) and bool((a[n_act:] == -7).all())
    _check_top2(f"rows Ny={Ny} P={P}", tuple(t[:n_act] for t in got), d64, d32, x_all, y, scale, bias, rows=rows[:n_act])
    # the whole list (no count), and a count beyond the list's length
    whole = ops.sim_top2_bias(xd, yd, sd, bias=bd, rows=rd)
    beyond = ops.sim_top2_bias(xd, yd, sd, bias=bd, rows=rd, n_active=_i32([5000], dev))
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(whole, dense, beyond))
    # a count of zero touches nothing
    zero = ops.sim_top2_bias(xd, yd, sd, bias=bd, rows=rd, n_active=_i32([0], dev),
                             out=tuple(torch.full_like(t, -7) for t in out))
    assert all(bool((t == -7).all()) for t in zero)


def test_top2_exact_ties(dev):
    """Duplicated keys: the lower key of an exact tie wins and the gap is exactly 0, across tiles and key splits; no bias."""
    x, y = ref.unit_clouds(130, 300, 8, 5)
    yy = torch.cat([y, y, y[:37]])                                    # key j ties with j + 300 (and j + 600 for j < 37)
    idx, best, gap = ops.sim_top2_bias(x.to(dev), yy.to(dev), _scalar(3.0, dev))
    assert int(idx.max()) < 300 and bool((gap == 0).all())
    single = ops.sim_top2_bias(x.to(dev), y.to(dev), _scalar(3.0, dev))
    assert torch.equal(idx, single[0]) and torch.equal(best, single[1]) and bool((single[2] > 0).all())


# ------------------------------------------------------------------------------------------------ 2: one round
def _round_instance():
    """N = 256, P = 16: rows 4k + 2 hold their planted key, rows 4k hold the planted key of row 4k + 1 (to be evicted), rows
    4k + 1 and 4k + 3 are unassigned, and row 4k + 3 sits next to row 4k + 1 while its own key is moved away, so both bid
    for one key.  Some prices are raised.  (x, y, bias, assigned, owner) as numpy f32 / int64."""
    N, P = 256, 16
    x, y, pi = aref.planted(N, P, 11)
    g = torch.Generator().manual_seed(12)
    x, y = x.clone(), y.clone()
    for k in range(N // 4):
        d = torch.nn.functional.normalize(torch.randn(P, generator=g), dim=0)
        x[4 * k + 3] = x[4 * k + 1] + 0.3 * d
        y[pi[4 * k + 3]] = torch.nn.functional.normalize(torch.randn(P, generator=g), dim=0) * 3.0
    st = aref.new_state(y.numpy(), np.float32)
    price = (torch.rand(N, generator=g) < 0.25).float() * 0.125
    st.bias = (st.bias - price.numpy()).astype(np.float32)
    for k in range(N // 4):
        for row, key in ((4 * k, int(pi[4 * k + 1])), (4 * k + 2, int(pi[4 * k + 2]))):
            st.assigned[row], st.owner[key] = key, row
    return x, y, st


def test_one_round_from_a_given_state(dev):
    x, y, st0 = _round_instance()
    eps = 0.01
    N = len(x)
    out = {}
    for dt in (np.float64, np.float32):
        st = aref.new_state(y.numpy(), dt)
        st.bias, st.assigned, st.owner = st0.bias.astype(dt), st0.assigned.copy(), st0.owner.copy()
        bidders = aref.one_round(x.numpy(), y.numpy(), st, eps, dt)
        out[dt] = st
    r64, r32 = out[np.float64], out[np.float32]
    assert bidders == N // 2 and not r64.stalled
    assert np.array_equal(r64.assigned, r32.assigned) and np.array_equal(r64.owner, r32.owner)      # clear gaps
    evicted = int(((st0.assigned >= 0) & (r64.assigned < 0)).sum())
    lost = int((r64.assigned < 0).sum()) - evicted
    print(f"one round: {bidders} bidders, {evicted} owners evicted, {lost} bidders lost their contest")
    assert evicted >= N // 8 and lost >= N // 8
    bias = torch.from_numpy(st0.bias).to(dev)
    assigned, owner = _i32(st0.assigned.tolist(), dev), _i32(st0.owner.tolist(), dev)
    state = torch.zeros(2, dtype=torch.int32, device=dev)
    xd, yd = x.to(dev), y.to(dev)
    ops.auction_rounds(xd, yd, bias, _scalar(eps, dev), assigned, owner, state[0:1], state[1:2], 0)
    assert state.tolist() == [N // 2, 0] and torch.equal(bias.cpu(), torch.from_numpy(st0.bias))      # 0 rounds only count
    ops.auction_rounds(xd, yd, bias, _scalar(eps, dev), assigned, owner, state[0:1], state[1:2], 1)
    assert np.array_equal(assigned.cpu().numpy(), r64.assigned) and np.array_equal(owner.cpu().numpy(), r64.owner)
    assert state.tolist() == [int((r64.assigned < 0).sum()), 0]
    B, dev_32, mag = _bound(torch.from_numpy(r64.bias), torch.from_numpy(r32.bias))
    dev_k = float((bias.cpu().double() - torch.from_numpy(r64.bias)).abs().max())
    print(f"bias after one round: kernel {dev_k:.3e}  f32 restatement {dev_32:.3e}  magnitude {mag:.3e}  bound {B:.3e}")
    assert dev_k <= B


# ------------------------------------------------------------------------------------------------ 3: solves
def _z_bound(x, y, bias):
    """B on the values the rows bid on, and those values in f64 (numpy)."""
    b = bias.cpu()
    z64 = 2.0 * (x.double() @ y.double().T) + b.double()[None, :]
    z32 = 2.0 * (x @ y.T) + b[None, :]
    return _bound(z64, z32)[0], z64.numpy()


def _check_solve(tag, r, x, y, opt=None):
    N = len(x)
    perm = r.perm.cpu().numpy()
    assert r.perm.dtype == torch.int64 and sorted(perm.tolist()) == list(range(N)), tag
    assert r.converged and r.reason == "converged", (tag, r.reason)
    assigned, owner = r.assigned.cpu().numpy(), r.owner.cpu().numpy()
    assert np.array_equal(assigned, perm) and np.array_equal(owner[assigned], np.arange(N)), tag
    B, z = _z_bound(x, y, r.bias)
    if opt is None:
        opt, _ = aref.scipy_optimum(x, y)
    cost64, lower64 = aref.certificate(x, y, r.bias.cpu().numpy(), perm)
    slack = float((z.max(1) - z[np.arange(N), perm]).max())
    print(f"{tag}: {r.n_rounds} rounds in {r.n_phases} phases {r.phase_rounds}; cost {r.cost:.6e} optimum {opt:.6e} "
          f"cost - optimum {r.cost - opt:.3e} gap {r.gap:.3e} eps {r.eps:.3e} B {B:.3e}; worst row slack {slack:.3e}; "
          f"lower bound {r.lower_bound:.6e} (f64 matrix {lower64:.6e})")
    assert abs(r.cost - cost64) <= 1e-12 * max(1.0, cost64) and abs(r.lower_bound - lower64) <= B
    assert math.isclose(r.gap, r.cost - r.lower_bound, rel_tol=0, abs_tol=1e-15)
    assert r.gap <= r.eps + B, tag
    assert r.cost - opt <= r.gap + B, tag
    assert r.cost >= opt - B, tag
    assert slack <= r.eps + 2 * B, tag                               # eps-complementary slackness, row by row in f64
    f, g = r.duals()
    assert f.dtype == g.dtype == F64 and abs(float(f.mean() + g.mean()) - r.lower_bound) <= 1e-9
    return B


SOLVES = [(N, P) for N in (1, 2, 63, 65, 257, 1024) for P in (4, 128, 768)] + [(4096, 64)]


@pytest.mark.parametrize("N,P", SOLVES)
def test_solve(dev, N, P):
    x, y = ref.unit_clouds(N, N, P, 3 * N + P)
    r = ot.exact_assignment(x.to(dev), y.to(dev))
    _check_solve(f"N={N} P={P}", r, x, y)
    assert r.n_phases == (0 if N == 1 else 4) and sum(r.phase_rounds) == r.n_rounds and r.n_rounds % 32 == 0
    assert abs(r.eps - 1e-4 * aref.mean_cost(x, y)) <= 1e-9


def test_solve_planted_matching(dev):
    for N, P, seed in ((257, 64, 1), (1024, 128, 2)):
        x, y, pi = aref.planted(N, P, seed)
        r = ot.exact_assignment(x.to(dev), y.to(dev), check_every=1)
        print(f"planted N={N} P={P}: {r.n_rounds} rounds")
        assert r.converged and torch.equal(r.perm.cpu(), pi) and r.n_rounds <= 12


def test_solve_duplicated_targets(dev):
    x, _ = ref.unit_clouds(256, 1, 64, 9)
    _, half = ref.unit_clouds(1, 128, 64, 10)
    y = torch.cat([half, half])
    r = ot.exact_assignment(x.to(dev), y.to(dev))
    _check_solve("duplicated targets", r, x, y)


def test_solve_identical_clouds(dev):
    x, _ = ref.unit_clouds(300, 1, 32, 4)
    r = ot.exact_assignment(x.to(dev), x.clone().to(dev))
    assert r.converged and torch.equal(r.perm.cpu(), torch.arange(300)) and r.cost == 0.0
    assert abs(r.gap) <= r.eps + _z_bound(x, x, r.bias)[0]


def test_solve_does_not_depend_on_the_chunking(dev):
    x, y = ref.unit_clouds(257, 257, 128, 21)
    xd, yd = x.to(dev), y.to(dev)
    r1 = ot.exact_assignment(xd, yd, check_every=1)
    assert r1.converged and r1.n_rounds == sum(r1.phase_rounds)
    for ce in (32, 500):
        r = ot.exact_assignment(xd, yd, check_every=ce)
        want = tuple(-(-p // ce) * ce for p in r1.phase_rounds)
        print(f"check_every={ce}: rounds {r.phase_rounds} against {r1.phase_rounds}")
        assert r.phase_rounds == want and r.n_rounds == sum(want)
        assert torch.equal(r.perm, r1.perm) and torch.equal(r.bias, r1.bias) and torch.equal(r.owner, r1.owner)
        assert r.cost == r1.cost and r.gap == r1.gap
    again = ot.exact_assignment(xd, yd, check_every=1)               # two runs are bit-identical
    assert torch.equal(again.perm, r1.perm) and torch.equal(again.bias, r1.bias) and again.phase_rounds == r1.phase_rounds


def test_solve_reports_a_stall_and_the_round_limit(dev):
    """eps = 1e-12 on clouds scaled by 100: prices ~ 1e4 have an f32 spacing ~ 1e-3, a tied bidder's offer leaves its key's
    price unchanged.  The solve says so and stops."""
    x, y = ref.unit_clouds(65, 65, 4, 7)
    r = ot.exact_assignment((100 * x).to(dev), (100 * y).to(dev), eps=1e-12, max_rounds=20000)
    print(f"stall: reason {r.reason} after {r.n_rounds} rounds in {r.n_phases} phases")
    assert not r.converged and r.reason == "stalled" and r.n_rounds < 20000
    x, y = ref.unit_clouds(257, 257, 128, 21)
    r = ot.exact_assignment(x.to(dev), y.to(dev), max_rounds=3)
    assert not r.converged and r.reason == "max_rounds" and r.n_rounds == 3 and r.n_phases == 1
    assert int((r.perm < 0).sum()) > 0 and math.isnan(r.cost) and math.isnan(r.gap)
    with pytest.raises(RuntimeError):
        ot.wasserstein2_exact(x.to(dev), y.to(dev), max_rounds=3)


def test_auction_rounds_are_capturable(dev):
    """Five rounds captured once and replayed on a fresh state equal five eager rounds, and 2 + 3 eager rounds."""
    N, P = 257, 64
    x, y = ref.unit_clouds(N, N, P, 33)
    xd, yd = x.to(dev), y.to(dev)
    eps = _scalar(0.01, dev)
    bias0 = -(yd * yd).sum(1)

    def fresh():
        return (bias0.clone(), torch.full((N,), -1, dtype=torch.int32, device=dev),
                torch.full((N,), -1, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev))

    def run(st, k):
        ops.auction_rounds(xd, yd, st[0], eps, st[1], st[2], st[3][0:1], st[3][1:2], k)

    eager, split = fresh(), fresh()
    run(eager, 5)
    run(split, 2)
    run(split, 3)
    assert all(torch.equal(a, b) for a, b in zip(eager, split))
    assert 0 < int(eager[3][0]) < N and int((eager[1] >= 0).sum()) == N - int(eager[3][0])
    st = fresh()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(st, 5)
    torch.cuda.current_stream().wait_stream(side)
    graph, keep = torch.cuda.CUDAGraph(), []
    with ops.owned_by_capture(keep), torch.cuda.graph(graph):
        run(st, 5)
    for _ in range(2):
        for t, f in zip(st, fresh()):
            t.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(st, eager))


# ------------------------------------------------------------------------------------------------ 4: matcher, gradient
def test_matcher(dev):
    N, P, sigma = 130, 64, 0.25
    x0, x1 = ref.unit_clouds(N, N, P, 23)
    x0d, x1d = x0.to(dev), x1.to(dev)
    perm = ot.exact_assignment(x0d, x1d).perm
    m = flow.ExactOptimalTransportConditionalFlowMatcher(sigma)
    gen = torch.Generator(device=dev).manual_seed(1)
    t, xt, ut, noise, (i, j) = m.sample_location_and_conditional_flow(x0d, x1d, return_noise=True, return_indices=True,
                                                                      generator=gen)
    assert t.shape == (N,) and xt.shape == ut.shape == noise.shape == (N, P) and i.shape == j.shape == (N,)
    assert i.dtype == j.dtype == torch.int64 and 0 <= int(i.min()) and int(i.max()) < N
    assert 0 <= float(t.min()) and float(t.max()) < 1
    assert torch.equal(j, perm[i]) and 1 < i.unique().numel() < N            # with replacement: repeats
    wx, wu = flow.linear_conditional_flow(x0d[i], x1d[j], t, noise, sigma)
    assert torch.equal(xt, wx) and torch.equal(ut, wu)
    rx, ru = flow.linear_conditional_flow(x0d[i].double(), x1d[j].double(), t.double(), noise.double(), sigma)
    assert float((xt - rx).abs().max()) < 1e-5 and float((ut - ru).abs().max()) < 1e-5
    # replace=False visits every row once; a given t is returned as it is; sigma = 0 lies on the chord
    m0 = flow.ExactOptimalTransportConditionalFlowMatcher(replace=False)
    tt = torch.linspace(0.1, 0.9, N, device=dev)
    out = m0.sample_location_and_conditional_flow(x0d, x1d, t=tt, return_indices=True)
    assert len(out) == 4 and out[0] is tt
    i0, j0 = out[3]
    assert torch.equal(i0, torch.arange(N, device=dev)) and torch.equal(j0, perm)
    assert torch.equal(out[2], x1d[perm] - x0d)
    assert float((out[1] - (tt[:, None] * x1d[perm] + (1 - tt[:, None]) * x0d)).abs().max()) < 1e-6
    assert len(m0.sample_location_and_conditional_flow(x0d, x1d)) == 3


def test_wasserstein2_exact_and_its_gradients(dev):
    N, P = 130, 64
    x, y = ref.unit_clouds(N, N, P, 29)
    xd, yd = x.to(dev).requires_grad_(), y.to(dev).requires_grad_()
    w = ot.wasserstein2_exact(xd, yd)
    r = ot.exact_assignment(xd, yd)
    opt, cols = aref.scipy_optimum(x, y)
    B, _ = _z_bound(x, y, r.bias)
    print(f"W2^2 {float(w):.6e}, optimum {opt:.6e}, cost {r.cost:.6e}")
    assert abs(float(w) - r.cost) <= 64 * U * r.cost and r.cost - opt <= r.eps + B
    w.backward()
    perm = r.perm.cpu()
    gx64 = 2.0 * (x.double() - y.double()[perm]) / N
    gy64 = torch.zeros(N, P, dtype=F64).index_add_(0, perm, -gx64)
    gx32 = 2.0 * (x - y[perm]) / N
    gy32 = torch.zeros(N, P).index_add_(0, perm, -gx32)
    for name, got, g64, g32 in (("dx", xd.grad, gx64, gx32), ("dy", yd.grad, gy64, gy32)):
        bound, dev_32, mag = _bound(g64, g32)
        dev_k = float((got.cpu().double() - g64).abs().max())
        print(f"{name}: kernel {dev_k:.3e}  f32 restatement {dev_32:.3e}  magnitude {mag:.3e}  bound {bound:.3e}")
        assert dev_k <= bound
