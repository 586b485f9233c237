"""Host-side tests of the exact coupling (clipk_sim_top2_bias, clipk_auction_rounds, ops.sim_top2_bias, ops.auction_rounds,
ot.exact_assignment, flow.ExactOptimalTransportConditionalFlowMatcher): the restatement of tests/auction_ref.py against
scipy's optimum, the merge rule of (z1, k1, z2) triples, the exports and signatures, the refusals of the C entries (they
return before any launch, so they run without a device), every argument error before any launch, and
flow.linear_conditional_flow against its formulae in f64."""
import inspect
import math
import random

import numpy as np
import pytest
import torch

import auction_ref as aref

ref = aref.ref
F64 = torch.float64


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("N,P,seed", [(2, 4, 0), (63, 4, 1), (65, 16, 2), (257, 128, 3), (300, 8, 4)])
def test_restatement_reaches_the_optimum_within_n_eps(N, P, seed):
    """Total cost within N eps of scipy's optimum = mean cost within eps, and never below it; the dual certificate of the
    final prices brackets the optimum with a gap of at most eps."""
    x, y = ref.unit_clouds(N, N, P, 100 * seed + N)
    opt, _ = aref.scipy_optimum(x, y)
    r = aref.solve(x.numpy(), y.numpy())
    assert r.converged and sorted(r.perm) == list(range(N)) and np.array_equal(r.owner[r.perm], np.arange(N))
    cost, lower = aref.certificate(x, y, r.bias, r.perm)
    print(f"N={N} P={P}: {r.n_rounds} rounds {r.phase_rounds}, cost - optimum {r.cost - opt:.3e}, gap {cost - lower:.3e}, eps {r.eps:.3e}")
    assert abs(cost - r.cost) < 1e-14
    assert -1e-12 <= r.cost - opt <= r.eps + 1e-12
    assert lower - 1e-12 <= opt and cost - lower <= r.eps + 1e-12
    # eps-complementary slackness row by row
    z = 2.0 * x.double().numpy() @ y.double().numpy().T + r.bias[None, :]
    assert (z[np.arange(N), r.perm] >= z.max(1) - r.eps - 1e-12).all()


def test_restatement_is_exact_on_planted_matchings():
    for N, P, seed in ((64, 8, 0), (257, 64, 1), (1024, 128, 2)):
        x, y, pi = aref.planted(N, P, seed)
        r = aref.solve(x.numpy(), y.numpy())
        _, cols = aref.scipy_optimum(x, y)
        print(f"planted N={N} P={P}: {r.n_rounds} rounds")
        assert np.array_equal(cols, pi.numpy()) and np.array_equal(r.perm, pi.numpy()) and r.n_rounds <= 12


def test_restatement_f32_stalls_below_the_price_resolution():
    """eps = 1e-12 on clouds scaled by 100 (prices ~ 1e4, f32 spacing ~ 1e-3): an offer of a tied bidder leaves the price
    unchanged; the solver reports it instead of spinning."""
    x, y = ref.unit_clouds(65, 65, 4, 7)
    r = aref.solve(100 * x.numpy(), 100 * y.numpy(), eps=1e-12, dtype=np.float32, max_rounds=20000)
    assert r.stalled and not r.converged and r.n_rounds < 20000


def test_one_round_rules():
    """Two bidders for one key: the larger offer wins; equal offers go to the lower row; the evicted owner is freed."""
    x = np.array([[1.0, 0, 0, 0], [1.0, 0, 0, 0], [0.9, 0.1, 0, 0]])
    y = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])
    st = aref.new_state(y)
    assert aref.one_round(x, y, st, 0.25) == 3
    # rows 0 and 1 offer 2 + 0.25 for key 0, row 2 offers 1.6 + 0.25: row 0 wins (equal offers, lower row)
    assert list(st.owner) == [0, -1, -1] and list(st.assigned) == [0, -1, -1]
    assert np.allclose(st.bias, [-1 - 2.25, -1, -1], atol=1e-15) and not st.stalled
    assert aref.one_round(x, y, st, 0.25) == 2
    # key 0 is now worth 2 - 3.25 = -1.25 to row 1 against -1 for keys 1, 2 (a tie: the lower key, gap 0, offer eps)
    assert list(st.owner) == [0, 1, -1] or list(st.owner)[0] == 0
    for _ in range(20):
        if aref.one_round(x, y, st, 0.25) == 0:
            break
    assert sorted(st.assigned) == [0, 1, 2] and np.array_equal(st.owner[st.assigned], np.arange(3))
    before = (st.bias.copy(), st.assigned.copy(), st.owner.copy())
    assert aref.one_round(x, y, st, 0.25) == 0                       # no bidders: nothing changes
    assert all(np.array_equal(a, b) for a, b in zip(before, (st.bias, st.assigned, st.owner)))


def test_top2_restatement():
    x, y = ref.unit_clouds(9, 65, 8, 2)
    bias = torch.linspace(-2, 2, 65)
    d = aref.top2(x, y, 4.0, bias, rows=torch.tensor([3, 3, 0, 8]))
    z = (4.0 * (x.double() @ y.double().T) + bias.double()[None, :]).numpy()[[3, 3, 0, 8]]
    srt = np.sort(z, axis=1)
    assert np.array_equal(d.idx.numpy(), z.argmax(1)) and np.array_equal(d.best.numpy(), srt[:, -1])
    assert np.allclose(d.gap.numpy(), srt[:, -1] - srt[:, -2], rtol=0, atol=1e-15)
    one = aref.top2(torch.zeros(2, 4), torch.zeros(1, 4), 1.0)
    assert one.idx.tolist() == [0, 0] and all(math.isinf(g) and g > 0 for g in one.gap.tolist())
    tie = aref.top2(torch.zeros(1, 4), torch.zeros(5, 4), 1.0, torch.tensor([0.0, 1.0, 1.0, -1.0, 1.0]))
    assert int(tie.idx[0]) == 1 and float(tie.gap[0]) == 0.0 and float(tie.best[0]) == 1.0


def test_merge_is_associative_and_commutative():
    """Random rows with many exact ties, cut into shuffled partitions and merged in shuffled tree orders: always the rule
    applied to the whole row."""
    rng = random.Random(0)
    for trial in range(300):
        n = rng.randint(1, 40)
        vals = [float(rng.randint(-3, 3)) for _ in range(n)]       # few distinct values: ties at the top are common
        want = aref.top2_of(vals)
        items = [aref.leaf(v, k) for k, v in enumerate(vals)] + [aref.EMPTY] * rng.randint(0, 3)
        rng.shuffle(items)
        while len(items) > 1:                                       # merge two random entries, in a random order
            a = items.pop(rng.randrange(len(items)))
            b = items.pop(rng.randrange(len(items)))
            items.append(aref.merge(a, b) if rng.random() < 0.5 else aref.merge(b, a))
        assert items[0] == want, (vals, items[0], want)
    a, b, c = aref.leaf(1.0, 5), aref.leaf(1.0, 2), aref.leaf(0.5, 0)
    assert aref.merge(a, b) == aref.merge(b, a) == (1.0, 2, 1.0)
    assert aref.merge(aref.merge(a, b), c) == aref.merge(a, aref.merge(b, c)) == (1.0, 2, 1.0)
    assert aref.merge(aref.EMPTY, c) == aref.merge(c, aref.EMPTY) == c


def test_eps_schedule():
    from clip_dplm_amd import ot
    for args in ((0.06, 2e-4, 8.0), (1e-5, 2e-4, 8.0), (2e-4, 2e-4, 8.0), (600.0, 1e-12, 8.0), (1.0, 0.1, 1.5)):
        s = ot.eps_schedule(*args)
        assert s == aref.eps_schedule(*args) and s[-1] == args[1] and all(a > b for a, b in zip(s, s[1:]))
    assert len(ot.eps_schedule(0.06, 2e-4, 8.0)) == 4 and ot.eps_schedule(1e-5, 2e-4, 8.0) == [2e-4]


# ------------------------------------------------------------------------------------------------ exports, C entries
def test_exports_and_signatures():
    import clip_dplm_amd as K
    from clip_dplm_amd import _ffi, flow, ops, ot
    lib = _ffi.load()
    assert lib.clipk_version() == _ffi.ABI_VERSION
    want = {"clipk_sim_top2_bias_plan": 4, "clipk_sim_top2_bias_workspace": 3, "clipk_sim_top2_bias": 16,
            "clipk_auction_rounds_workspace": 2, "clipk_auction_rounds": 14}
    for n, nargs in want.items():
        assert n in _ffi.SIGNATURES and hasattr(lib, n) and len(_ffi.SIGNATURES[n][1]) == nargs
    assert callable(ops.sim_top2_bias) and callable(ops.auction_rounds) and ops.AUCTION_MAX_N == 65536
    for n in ("AssignmentResult", "exact_assignment", "wasserstein2_exact"):
        assert getattr(K, n) is getattr(ot, n) and n in K.__all__ and n in ot.__all__
    for n in ("ExactOptimalTransportConditionalFlowMatcher", "linear_conditional_flow"):
        assert getattr(K, n) is getattr(flow, n) and n in K.__all__ and n in flow.__all__
    sig = inspect.signature(ot.exact_assignment)
    assert list(sig.parameters) == ["x", "y", "eps", "eps_rel", "eps_start_rel", "theta", "check_every", "max_rounds"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["eps"], d["eps_rel"], d["eps_start_rel"], d["theta"], d["check_every"]) == (None, 1e-4, 0.03, 8.0, 32)
    for f in ("perm", "cost", "gap", "eps", "n_rounds", "n_phases", "converged", "reason"):
        assert f in ot.AssignmentResult.__dataclass_fields__
    assert callable(ot.AssignmentResult.duals)
    # the matcher's method: the Schrodinger matcher's signature minus `seed`
    sb = list(inspect.signature(flow.SchrodingerBridgeConditionalFlowMatcher.sample_location_and_conditional_flow).parameters)
    ex = list(inspect.signature(flow.ExactOptimalTransportConditionalFlowMatcher.sample_location_and_conditional_flow).parameters)
    assert ex == [p for p in sb if p != "seed"]
    m = flow.ExactOptimalTransportConditionalFlowMatcher()
    assert m.sigma == 0.0 and m.replace is True and m.solver_kw == {}


def _top2(lib, Mx, Mr, Ny, P):
    return lib.clipk_sim_top2_bias(None, Mx, None, Mr, None, None, Ny, P, None, None, None, None, None, None, 0, None)


def _rounds(lib, N, P, n_rounds=1):
    return lib.clipk_auction_rounds(None, None, N, P, None, None, None, None, None, None, n_rounds, None, 0, None)


@pytest.mark.parametrize("Mr,Ny,P", [(0, 8, 8), (8, 0, 8), (-1, 8, 8), (8, 8, 0), (8, 8, 6), (8, 8, 772), (8, 8, 1028)])
def test_top2_entry_refuses(Mr, Ny, P):
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    assert lib.clipk_sim_top2_bias_workspace(Mr, Ny, P) == 0
    assert _top2(lib, 8, Mr, Ny, P) == (-2 if Mr > 0 and Ny > 0 and P > 0 else -1)


@pytest.mark.parametrize("N,P", [(0, 8), (-1, 8), (8, 0), (8, 6), (8, 772), (65537, 8), (1 << 20, 64)])
def test_auction_entry_refuses(N, P):
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    assert lib.clipk_auction_rounds_workspace(N, P) == 0
    assert _rounds(lib, N, P) == (-2 if N > 0 and P > 0 else -1)


def test_entry_limits_and_null_pointers():
    from clip_dplm_amd import _ffi, ops
    lib = _ffi.load()
    assert _top2(lib, 0, 8, 8, 8) == -1 and _top2(lib, 8, 8, 8, 64) == -1      # a supported shape, null pointers: no launch
    assert _rounds(lib, 8, 64) == -1 and _rounds(lib, 65536, 768) == -1 and _rounds(lib, 8, 64, -1) == -1
    assert lib.clipk_sim_top2_bias_workspace(1, 1, 4) > 0 and lib.clipk_auction_rounds_workspace(65536, 768) > 0
    # the key split does not depend on the row count; three words per row and split
    for Mr, Ny in ((1, 1), (1000, 4097), (65, 100003), (65536, 65536)):
        nqb, ks = ops.sim_top2_bias_plan(Mr, Ny)
        assert nqb == (Mr + 63) // 64 and ks == ops.sim_top2_bias_plan(1, Ny)[1] and 1 <= ks <= (Ny + 63) // 64
        assert lib.clipk_sim_top2_bias_workspace(Mr, Ny, 64) == ks * Mr * 12
    assert lib.clipk_auction_rounds_workspace(4096, 64) >= 4096 * 12 + lib.clipk_sim_top2_bias_workspace(4096, 4096, 64)


# ------------------------------------------------------------------------------------------------ argument errors
@pytest.fixture
def no_launch(monkeypatch):
    """Any use of the library after this point is a failure: the argument checks come before every launch."""
    from clip_dplm_amd import ops

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "_lib", boom)


def test_ops_argument_errors(no_launch):
    from clip_dplm_amd import ops
    x, y, s = torch.zeros(6, 8), torch.zeros(5, 8), torch.ones(1)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32)                 # noqa: E731
    with pytest.raises(TypeError):
        ops.sim_top2_bias(x.double(), y, s)
    with pytest.raises(TypeError):
        ops.sim_top2_bias(x, y, 2.0)
    with pytest.raises(TypeError):
        ops.sim_top2_bias(x, y, s, bias=torch.zeros(5, dtype=F64))
    with pytest.raises(ValueError):
        ops.sim_top2_bias(x, y, s, bias=torch.zeros(6))
    with pytest.raises(ValueError):
        ops.sim_top2_bias(x, torch.zeros(5, 12), s)
    with pytest.raises(ValueError):
        ops.sim_top2_bias(torch.zeros(6, 772), torch.zeros(5, 772), s)
    with pytest.raises(ValueError):
        ops.sim_top2_bias(torch.zeros(6, 6), torch.zeros(5, 6), s)
    for bad in ([0, 1], torch.zeros(3, dtype=torch.int64), i32(2, 2), i32(0)):
        with pytest.raises(TypeError):
            ops.sim_top2_bias(x, y, s, rows=bad)
    with pytest.raises(ValueError):
        ops.sim_top2_bias(x, y, s, rows=i32(3).to("meta"))
    with pytest.raises(TypeError):
        ops.sim_top2_bias(x, y, s, n_active=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.sim_top2_bias(x, y, s, n_active=i32(2))
    with pytest.raises(ValueError):
        ops.sim_top2_bias(x, y, s, out=(i32(5), torch.zeros(6), torch.zeros(6)))
    with pytest.raises(ValueError):
        ops.sim_top2_bias(x, y, s, out=(i32(6), None, torch.zeros(6)))
    with pytest.raises(ValueError):
        ops.sim_top2_bias(x, y, s, rows=i32(3), out=(i32(3), torch.zeros(6), torch.zeros(3)))
    with pytest.raises(ValueError):
        ops.sim_top2_bias(x, y, s)                                  # host tensors
    # ---- auction_rounds
    y6, b, e = torch.zeros(6, 8), torch.zeros(6), torch.ones(1)
    good = dict(bias=b, eps=e, assigned=i32(6), owner=i32(6), n_unassigned=i32(1), stalled=i32(1), n_rounds=1)
    for key, bad, err in (("n_rounds", -1, ValueError), ("n_rounds", 1.5, ValueError), ("n_rounds", True, ValueError),
                          ("eps", 0.5, TypeError), ("eps", torch.ones(2), TypeError), ("eps", torch.ones(1, dtype=F64), TypeError),
                          ("bias", None, ValueError), ("bias", torch.zeros(5), ValueError), ("bias", b.double(), TypeError),
                          ("assigned", torch.zeros(6, dtype=torch.int64), TypeError), ("assigned", i32(5), ValueError),
                          ("owner", i32(7), ValueError), ("owner", None, TypeError),
                          ("n_unassigned", i32(2), ValueError), ("stalled", torch.zeros(1), TypeError)):
        with pytest.raises(err):
            ops.auction_rounds(x, y6, **dict(good, **{key: bad}))
    with pytest.raises(ValueError):
        ops.auction_rounds(x, y, **good)                             # 6 rows against 5
    with pytest.raises(ValueError):
        ops.auction_rounds(torch.zeros(6, 6), torch.zeros(6, 6), **good)
    big = torch.zeros(1, 8).expand(65537, 8)
    with pytest.raises(ValueError):
        ops.auction_rounds(big, big, **good)
    with pytest.raises(ValueError):
        ops.auction_rounds(x, y6, **good)                            # host tensors


def test_ot_argument_errors(no_launch):
    from clip_dplm_amd import ot
    x, y = torch.zeros(6, 8), torch.zeros(6, 8)
    with pytest.raises(ValueError, match="sinkhorn"):
        ot.exact_assignment(x, torch.zeros(5, 8))                    # unequal sizes: no permutation plan
    with pytest.raises(TypeError):
        ot.exact_assignment(x.double(), y)
    with pytest.raises(TypeError):
        ot.exact_assignment(x, [[0.0] * 8] * 6)
    with pytest.raises(ValueError):
        ot.exact_assignment(x, torch.zeros(6, 12))
    with pytest.raises(ValueError):
        ot.exact_assignment(torch.zeros(6, 6), torch.zeros(6, 6))
    with pytest.raises(ValueError):
        ot.exact_assignment(torch.zeros(6, 772), torch.zeros(6, 772))
    with pytest.raises(ValueError):
        ot.exact_assignment(torch.zeros(0, 8), torch.zeros(0, 8))
    with pytest.raises(ValueError):
        ot.exact_assignment(torch.zeros(6), torch.zeros(6))
    big = torch.zeros(1, 8).expand(65537, 8)
    with pytest.raises(ValueError):
        ot.exact_assignment(big, big)
    for kw in (dict(eps=0.0), dict(eps=-1.0), dict(eps=float("inf")), dict(eps=torch.ones(())), dict(eps_rel=0.0),
               dict(eps_rel=float("nan")), dict(eps_start_rel=0.0), dict(theta=1.0), dict(theta=0.5), dict(theta=float("inf")),
               dict(check_every=0), dict(max_rounds=0)):
        with pytest.raises(ValueError):
            ot.exact_assignment(x, y, **kw)
    with pytest.raises(ValueError):
        ot.exact_assignment(x, y)                                    # host tensors
    with pytest.raises(ValueError):
        ot.wasserstein2_exact(x, torch.zeros(5, 8))


def test_flow_argument_errors(no_launch):
    from clip_dplm_amd import flow
    M = flow.ExactOptimalTransportConditionalFlowMatcher
    for kw in (dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf"))):
        with pytest.raises(ValueError):
            M(**kw)
    with pytest.raises(TypeError):
        M(0.1, n_iters=5)                                            # not an argument of the exact solver
    m = M(0.25, replace=False, eps_rel=1e-3, check_every=8)
    assert m.sigma == 0.25 and m.replace is False and m.solver_kw == dict(eps_rel=1e-3, check_every=8)
    x0 = torch.zeros(6, 8)
    with pytest.raises(ValueError):
        m.sample_location_and_conditional_flow(x0, x0)              # host tensors
    with pytest.raises(ValueError, match="sinkhorn"):
        m.sample_location_and_conditional_flow(x0, torch.zeros(5, 8))
    with pytest.raises(TypeError):
        m.sample_location_and_conditional_flow(x0.double(), x0)
    with pytest.raises(ValueError):
        m.sample_location_and_conditional_flow(x0, x0, t=torch.zeros(5))
    with pytest.raises(TypeError):
        m.sample_location_and_conditional_flow(x0, x0, seed=1)      # the exact coupling draws no j: there is no seed
    z = torch.zeros(4, 3)
    with pytest.raises(ValueError):
        flow.linear_conditional_flow(z, torch.zeros(4, 2), 0.5, z, 1.0)
    with pytest.raises(ValueError):
        flow.linear_conditional_flow(z, z, torch.zeros(3), z, 1.0)
    with pytest.raises(TypeError):
        flow.linear_conditional_flow(z, z, 0.5, None, 1.0)


# ------------------------------------------------------------------------------------------------ the flow arithmetic
def test_linear_conditional_flow_formulae():
    from clip_dplm_amd import flow
    g = torch.Generator().manual_seed(0)
    n, P, sigma = 33, 12, 0.7
    x0, x1, noise = (torch.randn(n, P, generator=g, dtype=F64) for _ in range(3))
    t = torch.rand(n, generator=g, dtype=F64)
    t[0], t[1] = 0.0, 1.0
    xt, ut = flow.linear_conditional_flow(x0, x1, t, noise, sigma)
    assert xt.dtype == F64 and xt.shape == ut.shape == (n, P)
    for k in range(n):
        tk = float(t[k])
        want = tk * x1[k] + (1 - tk) * x0[k] + sigma * noise[k]
        assert float((xt[k] - want).abs().max()) < 1e-14
    assert torch.equal(ut, x1 - x0)
    x_clean, _ = flow.linear_conditional_flow(x0, x1, t, noise, 0.0)
    assert torch.equal(x_clean[0], x0[0]) and torch.equal(x_clean[1], x1[1])      # the end points, without noise
    xs, us = flow.linear_conditional_flow(x0, x1, 0.25, noise, sigma)            # one time for every row
    xr, ur = flow.linear_conditional_flow(x0, x1, torch.full((n,), 0.25, dtype=F64), noise, sigma)
    assert torch.equal(xs, xr) and torch.equal(us, ur)
    # the bridge's own formulae are untouched by the shared argument checks
    xb, ub = flow.conditional_flow(x0, x1, t, noise, sigma)
    mu = t[:, None] * x1 + (1 - t[:, None]) * x0
    assert float((xb - (mu + sigma * torch.sqrt(t * (1 - t))[:, None] * noise)).abs().max()) < 1e-14
