"""Restatement of the exact coupling (include/clipk.h: clipk_sim_top2_bias, clipk_auction_rounds; ot.exact_assignment) in
numpy / torch on explicit matrices: the top-two rule, the merge of (z1, k1, z2) triples, one Jacobi bidding round and the
eps-scaled solver.  Not a test module; test_exact_ot_host.py holds it to scipy's optimum and test_gpu_exact_ot.py holds
the kernels to it."""
from types import SimpleNamespace

import numpy as np
import torch

import sinkhorn_ref as ref

NO_KEY = 0x7FFFFFFF


# ------------------------------------------------------------------------------------------------ the top-two rule
def top2(x, y, scale, bias=None, dtype=torch.float64, rows=None, chunk=256):
    """idx = argmax_j z, best = max_j z, gap = best - max_{j != idx} z (+inf with one key) of z = scale <x[rows], y_j> +
    bias_j in `dtype`, a higher z best and equal z to the lower key.  The rows in chunks, on the inputs' device."""
    x, y = x.to(dtype), y.to(dtype)
    if rows is not None:
        x = x[rows.long()]
    b = None if bias is None else bias.to(dtype)
    idx, best, gap = [], [], []
    for i in range(0, len(x), chunk):
        z = scale * (x[i:i + chunk] @ y.T)
        if b is not None:
            z = z + b[None, :]
        m = z.max(1).values
        k = (z == m[:, None]).to(torch.int8).argmax(1)               # the first (lowest) key that reaches the maximum
        z.scatter_(1, k[:, None], -float("inf"))
        idx.append(k)
        best.append(m)
        gap.append(m - z.max(1).values)
    return SimpleNamespace(idx=torch.cat(idx), best=torch.cat(best), gap=torch.cat(gap))


def values_at(x, y, scale, bias, keys, dtype=torch.float64):
    """(z at the given key of every row, the row maximum) in `dtype`."""
    x, y = x.to(dtype), y.to(dtype)
    z = scale * (x @ y.T)
    if bias is not None:
        z = z + bias.to(dtype)[None, :]
    return z.gather(1, keys.long()[:, None])[:, 0], z.max(1).values


EMPTY = (-float("inf"), NO_KEY, -float("inf"))


def leaf(z, k):
    return (float(z), int(k), -float("inf"))


def merge(a, b):
    """The merge of two (z1, k1, z2) triples: the higher z1 wins, equal z1 goes to the lower key, the runner-up is the
    maximum of what is left (the loser's z1 and the winner's z2)."""
    (za, ka, sa), (zb, kb, sb) = a, b
    if zb > za or (zb == za and kb < ka):
        return (zb, kb, max(za, sb))
    return (za, ka, max(sa, zb))


def top2_of(values):
    """The rule applied to one row of values directly: (max, lowest key of the max, max of the others)."""
    v = np.asarray(values, dtype=np.float64)
    k = int(np.argmax(v))
    rest = np.delete(v, k)
    return (float(v[k]), k, float(rest.max()) if len(rest) else -float("inf"))


# ------------------------------------------------------------------------------------------------ one round, the solver
def new_state(y, dtype=np.float64):
    y = np.asarray(y, dtype=dtype)
    n = len(y)
    return SimpleNamespace(bias=-(y * y).sum(1), assigned=np.full(n, -1, np.int64), owner=np.full(n, -1, np.int64),
                           stalled=False)


def one_round(x, y, st, eps, dtype=np.float64):
    """One Jacobi round on the state st (bias, assigned, owner, stalled), in place, in `dtype`: every unassigned row bids
    inc = gap + eps for its best key; a key keeps the largest offer, an equal offer goes to the lower row; it frees its
    previous owner, takes the winner and lowers its bias by inc (stalled when that leaves the bias unchanged).  Returns
    the number of bidders."""
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    rows = np.nonzero(st.assigned < 0)[0]
    if len(rows) == 0:
        return 0
    z = dtype(2.0) * (x[rows] @ y.T) + st.bias[None, :].astype(dtype)
    ar = np.arange(len(rows))
    idx = z.argmax(1)                                                 # numpy: the first maximum, the lower key
    best = z[ar, idx]
    z[ar, idx] = -np.inf
    inc = ((best - z.max(1)) + dtype(eps)).astype(dtype)
    order = np.lexsort((rows, -inc, idx))                             # by key, then the larger offer, then the lower row
    first = np.ones(len(rows), bool)
    first[1:] = idx[order][1:] != idx[order][:-1]
    for r in order[first]:
        j, row = int(idx[r]), int(rows[r])
        prev = st.owner[j]
        if prev >= 0:
            st.assigned[prev] = -1
        st.owner[j], st.assigned[row] = row, j
        nb = dtype(st.bias[j] - inc[r])
        st.stalled |= bool(nb == st.bias[j])
        st.bias[j] = nb
    return len(rows)


def eps_schedule(eps_start, eps, theta):
    out, e = [], float(eps_start)
    while e > eps:
        out.append(e)
        e /= theta
    out.append(float(eps))
    return out


def mean_cost(x, y):
    return float(ref.mean_cost_explicit(torch.as_tensor(x).double(), torch.as_tensor(y).double()))


def solve(x, y, eps=None, eps_rel=1e-4, eps_start_rel=0.03, theta=8.0, dtype=np.float64, max_rounds=200000):
    """The eps-scaled auction: phases from eps_start_rel x mean cost down to eps by theta, the prices kept, the assignment
    reset.  Returns perm, bias, cost (mean squared distance in f64), eps, n_rounds, phase_rounds, bidders (per round),
    converged, stalled."""
    xd, yd = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    mc = mean_cost(xd, yd)
    eps = float(eps) if eps is not None else eps_rel * mc
    st = new_state(np.asarray(y, dtype=dtype), dtype)
    total, phases, bidders, ok = 0, [], [], True
    for e in eps_schedule(eps_start_rel * mc, eps, theta):
        st.assigned[:] = -1
        st.owner[:] = -1
        done = 0
        while ok and (st.assigned < 0).any():
            bidders.append(one_round(x, y, st, e, dtype))
            total, done = total + 1, done + 1
            ok = not st.stalled and total < max_rounds
        phases.append(done)
        if not ok:
            break
    conv = not (st.assigned < 0).any() and not st.stalled
    cost = float(((xd - yd[st.assigned]) ** 2).sum(1).mean()) if not (st.assigned < 0).any() else float("nan")
    return SimpleNamespace(perm=st.assigned.copy(), owner=st.owner.copy(), bias=st.bias.copy(), cost=cost, eps=eps,
                           n_rounds=total, phase_rounds=tuple(phases), bidders=bidders, converged=conv, stalled=st.stalled)


def scipy_optimum(x, y):
    """(mean cost, column indices) of the optimal matching on the f64 matrix."""
    from scipy.optimize import linear_sum_assignment
    c = ref.cost_matrix(torch.as_tensor(x).double(), torch.as_tensor(y).double()).numpy()
    r, cidx = linear_sum_assignment(c)
    return float(c[r, cidx].mean()), cidx


def certificate(x, y, bias, perm):
    """(cost, lower bound) in f64 on the explicit matrix: L = (sum |x_i|^2 - sum_j p_j - sum_i max_j z_ij) / N with
    p_j = -|y_j|^2 - bias_j."""
    xd, yd, b = (np.asarray(v, dtype=np.float64) for v in (x, y, bias))
    z = 2.0 * xd @ yd.T + b[None, :]
    lower = ((xd * xd).sum() + (yd * yd).sum() + b.sum() - z.max(1).sum()) / len(xd)
    return float(((xd - yd[perm]) ** 2).sum(1).mean()), float(lower)


def planted(N, P, seed, noise=0.05):
    """x unit rows, y[pi[i]] = x[i] + noise * randn / sqrt(P) in f32: (x, y, pi)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.normalize(torch.randn(N, P, generator=g, dtype=torch.float64), dim=1)
    pi = torch.randperm(N, generator=g)
    y = torch.empty_like(x)
    y[pi] = x + noise * torch.randn(N, P, generator=g, dtype=torch.float64) / P ** 0.5
    return x.float(), y.float(), pi
