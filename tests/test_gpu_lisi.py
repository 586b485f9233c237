"""GPU: the label-mass walk (include/clipk.h: clipk_label_kernel_sums; ops.label_kernel_sums) and clip_dplm_amd.mixing on top
of it against the restatement of tests/lisi_ref.py.

Tolerance rule of every comparison (`_close`, the rule of tests/test_gpu_tsne.py): the f64 restatement (d from coordinate
differences) is the reference; the kernel may deviate from it by at most 8 x the deviation of the f32 restatement (d from
the norm expansion, as in the kernel) on the same inputs - the factor covers the different summation order - with a
floor of 64 * 2^-24 x the quantity's magnitude (the largest entry of the reference).  Label columns are compared one by
one (`_close_columns`: their magnitudes run from the whole mass to nothing).  The measured deviations and the fraction of
the bound they use are printed before each assertion.

Shapes: N in {3, 63, 65, 130, 1000} (one row block short, one over, three key splits at 130, sixteen blocks), P in
{4, 60, 512} (one K-step, a ragged one, the limit), G in {1, 2, 10, 32, 33, 64, 65, 130, 512}: the key-split form of the
second product with one and two 32-label blocks at and past their edges, the row-split form with one to four label tiles
per wave.  The weights of a shape are formed once and serve every G."""
import functools

import pytest
import torch

from clip_dplm_amd import manifold, mixing, ops

import lisi_ref as ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F64, F32 = torch.float64, torch.float32
SHAPES = [(N, P) for N in (3, 63, 65, 130, 1000) for P in (4, 60, 512)]
LABEL_COUNTS = (1, 2, 10, 32, 33, 64, 65, 130, 512)
VOTE_CASES = [(130, 60, 2), (130, 60, 10), (1000, 60, 10), (1000, 60, 64), (1000, 60, 130)]     # tests/test_lisi_host.py


def _close(name, got, r64, r32):
    got, r64, r32 = (torch.as_tensor(t).detach().double().cpu() for t in (got, r64, r32))
    assert got.shape == r64.shape, (name, got.shape, r64.shape)
    assert torch.isfinite(got).all(), name
    dev_k, dev_32 = float((got - r64).abs().max()), float((r32 - r64).abs().max())
    mag = float(r64.abs().max())
    bound = max(8 * dev_32, 64 * U * mag)
    print(f"{name}: kernel {dev_k:.3e}  f32 restatement {dev_32:.3e}  magnitude {mag:.3e}  bound {bound:.3e}  "
          f"fraction {dev_k / bound if bound else 0.0:.3f}")
    assert dev_k <= bound, (name, dev_k, bound)
    return bound


def _close_columns(name, got, r64, r32):
    """_close on every label column with the column's own deviation, magnitude and bound; the column that uses the largest
    fraction of its bound is printed.  A label without keys is a column of zeros on all three sides: bound 0, deviation 0."""
    got, r64, r32 = (torch.as_tensor(t).detach().double().cpu() for t in (got, r64, r32))
    assert got.shape == r64.shape, (name, got.shape, r64.shape)
    assert torch.isfinite(got).all(), name
    dev_k = (got - r64).abs().max(0).values
    bound = ref.column_bounds(r64, r32)
    frac = torch.where(bound > 0, dev_k / bound, (dev_k > 0).double() * float("inf"))
    g = int(frac.argmax())
    print(f"{name}: worst column {g} of {got.shape[1]}: kernel {float(dev_k[g]):.3e}  bound {float(bound[g]):.3e}  "
          f"fraction {float(frac[g]):.3f}")
    assert bool((dev_k <= bound).all()), (name, g, float(dev_k[g]), float(bound[g]))


@functools.lru_cache(maxsize=None)
def _weights(N, P):
    """(x f32, beta f32, shift f32, w64, w32) of the shape's cloud against itself, the diagonal left out: on the host, for
    N = 1000 on the device (torch's own kernels take seconds off a case); shared by the tests of a shape, never changed.
    beta, shift: the f64 calibration rounded to f32 - kernel and both restatements get the same inputs."""
    x = ref.cloud(N, P, 17 * N + P)
    if N >= 1000:
        x = x.cuda()
    d64, d32 = ref.sq_dists(x.double()), ref.sq_dists(x)
    beta, shift = ref.calibrated(x, ref.case_perplexity(N), d64)
    return x, beta, shift, ref.weights(d64, beta.double(), shift.double()), ref.weights(d32, beta, shift)


def _labels(N, G, seed):
    """int32 [N] in [0, G), a few entries outside (where N allows it): they belong to no column."""
    lab = torch.randint(0, G, (N,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    if N >= 63:
        lab[5], lab[17], lab[N - 2] = -1, G, G + 5
    return lab


def _padding(out, G):
    """The padding columns of the [Mx, Gp] buffer behind the [Mx, G] view ops.label_kernel_sums returns."""
    base = out if out._base is None else out._base
    assert base.shape == (out.shape[0], (G + 3) // 4 * 4) and base.data_ptr() == out.data_ptr()
    return base[:, G:]


# ------------------------------------------------------------------------------------------------ 1: sums
@pytest.mark.parametrize("N,P", SHAPES)
def test_label_kernel_sums(dev, N, P):
    """out column by column, mass, sumsq and best against the restatement for every label count; two runs bit-identical;
    the statistics without `out` equal those with it bit for bit; the padding columns are zero; labels outside [0, G)
    enter no column."""
    x, beta, shift, w64, w32 = _weights(N, P)
    xd, bd, sd = x.to(dev), beta.to(dev), shift.to(dev)
    nqb, ks = ops.cond_entropy_sums_plan(N)
    assert nqb == (N + 63) // 64 and 1 <= ks <= (N + 63) // 64
    if N == 130:
        assert ks == 3, "130 rows no longer split the key range three ways"
    for G in LABEL_COUNTS:
        lab = _labels(N, G, 1000 * N + G)
        ld = lab.to(dev)
        o64, o32 = ref.label_sums(w64, lab, G), ref.label_sums(w32, lab, G)
        out, mass, sumsq, top, best = ops.label_kernel_sums(xd, xd, ld, G, bd, sd, diag_offset=0)
        tag = f"N={N} P={P} G={G}"
        assert out.shape == (N, G) and top.dtype == torch.int32 and all(t.shape == (N,) for t in (mass, sumsq, top, best))
        _close_columns(f"out {tag}", out, o64, o32)
        s64, s32 = ref.stats(o64), ref.stats(o32)
        _close(f"mass {tag}", mass, s64[0], s32[0])
        _close(f"sumsq {tag}", sumsq, s64[1], s32[1])
        _close(f"best {tag}", best, s64[3], s32[3])
        assert torch.equal(_padding(out, G), torch.zeros_like(_padding(out, G))), tag
        assert bool((top >= 0).all()) and bool((top < G).all()), tag
        # the statistics are those of the kernel's own out, in the order the header states
        assert torch.equal(best, out.max(1).values) and torch.equal(out.gather(1, top.long()[:, None])[:, 0], best), tag
        again = ops.label_kernel_sums(xd, xd, ld, G, bd, sd, diag_offset=0)
        assert all(torch.equal(a, b) for a, b in zip(again, (out, mass, sumsq, top, best))), tag
        none, *only = ops.label_kernel_sums(xd, xd, ld, G, bd, sd, diag_offset=0, want_out=False)
        assert none is None and all(torch.equal(a, b) for a, b in zip(only, (mass, sumsq, top, best))), tag
        o2, *nostats = ops.label_kernel_sums(xd, xd, ld, G, bd, sd, diag_offset=0, want_stats=False)
        assert nostats == [None] * 4 and torch.equal(o2, out), tag


# ------------------------------------------------------------------------------------------------ 2: top
@pytest.mark.parametrize("N,P,G", VOTE_CASES)
def test_top(dev, N, P, G):
    """Blobs, the labels following the blobs with a tenth flipped.  top equals the f64 arg max on every decided row
    (lisi_ref.decided_rows: the two largest f64 masses differ by more than twice the bound); the rest are near-ties and
    may go either way, but at most 1 % of the rows may be near-ties (tests/test_lisi_host.py checks the restatement alone
    against that cap)."""
    x, lab = ref.vote_case(N, P, G, 100 + G)
    d64, d32 = ref.sq_dists(x.double()), ref.sq_dists(x)
    beta, shift = ref.calibrated(x, ref.case_perplexity(N), d64)
    o64 = ref.label_sums(ref.weights(d64, beta.double(), shift.double()), lab, G)
    o32 = ref.label_sums(ref.weights(d32, beta, shift), lab, G)
    decided = ref.decided_rows(o64, o32)
    xd = x.to(dev)
    _, mass, _, top, best = ops.label_kernel_sums(xd, xd, lab.int().to(dev), G, beta.to(dev), shift.to(dev), diag_offset=0,
                                                  want_out=False)
    t64 = ref.stats(o64)[2]
    wrong = int((top.cpu().long() != t64)[decided].sum())
    print(f"top N={N} P={P} G={G}: {int((~decided).sum())} near-ties, {wrong} decided rows off the f64 arg max")
    assert int((~decided).sum()) <= N // 100
    assert wrong == 0


@pytest.mark.parametrize("G,a,b", [(5, 1, 3), (40, 2, 37), (130, 7, 100), (512, 100, 511)])
def test_exact_ties_go_to_the_lower_label(dev, G, a, b):
    """Every key is there twice, side by side, first under label b, then under label a < b, and no other label has keys:
    the two columns receive the same terms in the same order - the other label's term is an exact 0 in each product - so
    they are equal bit for bit, and every row's vote goes to a."""
    Mx, Nz, P = 100, 150, 16
    g = torch.Generator().manual_seed(G)
    xq, z = torch.randn(Mx, P, generator=g), torch.randn(Nz, P, generator=g)
    y = z.repeat_interleave(2, dim=0).contiguous()
    lab = torch.tensor([b, a], dtype=torch.int32).repeat(Nz)
    beta = torch.rand(Mx, generator=g) * 0.2 + 0.05
    out, mass, sumsq, top, best = ops.label_kernel_sums(xq.to(dev), y.to(dev), lab.to(dev), G, beta.to(dev))
    assert bool((out[:, a] > 0).all()) and torch.equal(out[:, a], out[:, b])
    assert torch.equal(top, torch.full_like(top, a)) and torch.equal(best, out[:, a])
    assert torch.equal(mass, out[:, a] + out[:, b])                       # the other columns are exact zeros


# ------------------------------------------------------------------------------------------------ 3: the nearest term
@pytest.mark.parametrize("N,P,G", [(130, 60, 10), (1000, 4, 33), (130, 512, 130)])
def test_nearest_term_is_exactly_one(dev, N, P, G):
    """shift = dmin from ops.cond_entropy_sums, beta = 400 / (the gap between the two smallest distances of the row): the
    nearest neighbour's term is exp(0) = 1 only if the walk forms its d bit for bit as the calibration walk did, and every
    other term underflows.  So mass == 1 and out[i, label(nn_i)] == 1 exactly, for the whole cloud and for a row block
    (Mx < Ny, diag_offset = r0).
    Rows [r0, r1) of the full call equal the row-block call bit for bit because the two calls share one key-split plan:
    with (N / 64)^2 <= 512 the plan gives every 64-key tile a split of its own whatever Mx <= N is (asserted below)."""
    x = ref.cloud(N, P, 17 * N + P)
    d = ref.sq_dists(x.double()).masked_fill(torch.eye(N, dtype=torch.bool), float("inf"))
    two, idx = d.topk(2, dim=1, largest=False)
    gap = two[:, 1] - two[:, 0]
    # generic: the gap is well above the rounding of an f32 distance (measured on the f32 restatement), so the kernel's own
    # second-nearest t is at least 3/4 of it and beta t >= 300: 2^(-300 log2 e) is far below the smallest f32
    err = float((ref.sq_dists(x).double() - ref.sq_dists(x.double())).abs().max())
    assert float(gap.min()) > 8 * err, "the cloud is not generic: two nearest neighbours at nearly one distance"
    beta = (400.0 / gap).float()
    lab = torch.randint(0, G, (N,), generator=torch.Generator().manual_seed(N), dtype=torch.int32)
    xd, bd, ld = x.to(dev), beta.to(dev), lab.to(dev)
    dmin = ops.cond_entropy_sums(xd)[0]
    out, mass, sumsq, top, best = ops.label_kernel_sums(xd, xd, ld, G, bd, dmin, diag_offset=0)
    nn_label = lab[idx[:, 0]].long().to(dev)
    one = torch.ones(N, device=dev)
    assert torch.equal(mass, one) and torch.equal(sumsq, one) and torch.equal(best, one)
    assert torch.equal(out.gather(1, nn_label[:, None])[:, 0], one) and torch.equal(top.long(), nn_label)
    full = (out, mass, sumsq, top, best)
    ntiles = (N + 63) // 64
    for r0, r1 in ((64, N), (37, 101)):
        assert ops.sim_lse_bias_plan(r1 - r0, N)[1] == ntiles == ops.sim_lse_bias_plan(N, N)[1]
        block = ops.label_kernel_sums(xd[r0:r1], xd, ld, G, bd[r0:r1], dmin[r0:r1], diag_offset=r0)
        assert torch.equal(block[1], one[r0:r1])
        assert all(torch.equal(a, b[r0:r1]) for a, b in zip(block, full)), (r0, r1)
    # with a calibrated beta too: the row block's sums are those of the full call, bit for bit
    soft = (1.0 / gap).float().to(dev)
    full = ops.label_kernel_sums(xd, xd, ld, G, soft, dmin, diag_offset=0)
    block = ops.label_kernel_sums(xd[37:101], xd, ld, G, soft[37:101], dmin[37:101], diag_offset=37)
    assert bool((full[1] > 1).any()) and all(torch.equal(a, b[37:101]) for a, b in zip(block, full))


# ------------------------------------------------------------------------------------------------ 4: the diagonal
def test_diagonal_is_dropped_not_subtracted(dev):
    """The norm-30 rows of test_gpu_tsne.test_cond_entropy_diagonal_is_dropped_not_subtracted: the computed d_ii is
    rounding noise of the size of an ulp of 1800.  beta = 1: every off-diagonal term is exp(-~1800) = 0, so with the
    diagonal skipped every output is exactly 0.  beta = 1 / 1800: full minus skipped is the diagonal's term - 1 within
    4 ulp of the column in the point's own label column, exactly 0 in the others."""
    M, P, G = 200, 64, 10
    g = torch.Generator().manual_seed(2)
    x = torch.nn.functional.normalize(torch.randn(M, P, generator=g, dtype=F64), dim=1).mul(30.0).float().to(dev)
    lab = torch.randint(0, G, (M,), generator=g, dtype=torch.int32).to(dev)
    one = torch.ones(M, dtype=F32, device=dev)
    out, mass, sumsq, top, best = ops.label_kernel_sums(x, x, lab, G, one, diag_offset=0)
    zero = torch.zeros(M, device=dev)
    assert torch.equal(out, torch.zeros_like(out)) and torch.equal(mass, zero) and torch.equal(sumsq, zero)
    assert torch.equal(best, zero) and torch.equal(top, torch.zeros_like(top))
    beta = one / 1800.0
    full = ops.label_kernel_sums(x, x, lab, G, beta, diag_offset=-1)[0].double()
    skip = ops.label_kernel_sums(x, x, lab, G, beta, diag_offset=0)[0].double()
    own = torch.zeros_like(full, dtype=torch.bool).scatter_(1, lab.long()[:, None], True)
    diff = full - skip
    ulp = torch.exp2(torch.floor(torch.log2(full[own])) - 23)
    dev_ulp = float(((diff[own] - 1.0).abs() / ulp).max())
    print(f"diagonal rule: own column in [{float(full[own].min()):.3f}, {float(full[own].max()):.3f}], (full - skipped - 1) "
          f"up to {dev_ulp:.3f} ulp of it; other columns differ by up to {float(diff[~own].abs().max()):.1e}")
    assert dev_ulp <= 4.0
    assert torch.equal(diff[~own], torch.zeros_like(diff[~own]))


# ------------------------------------------------------------------------------------------------ 5: the public API
@functools.lru_cache(maxsize=None)
def _api_case(metric):
    """N = 1000, P = 60: (x f32 on the host, prepared d64, d32 on the device, the modality of two clouds of 500 rows, ten
    labels following ten blobs with a tenth flipped)."""
    x, lab = ref.vote_case(1000, 60, 10, 31)
    modality = (torch.arange(1000) >= 500).long()
    p64, p32 = ref.prepare(x.cuda(), metric), ref.prepare(x.cuda(), metric, F32)
    return x, ref.sq_dists(p64), ref.sq_dists(p32), modality, lab


def _restated(metric, labels, G=None):
    """(o64, o32) [N, G]: each restatement with the calibration of its own precision - the bandwidth rule of
    test_gpu_tsne.test_perplexity_bandwidths."""
    x, d64, d32, _, _ = _api_case(metric)
    o64 = ref.label_sums_exact(ref.prepare(x.cuda(), metric), labels, 30.0, d=d64, G=G)
    o32 = ref.label_sums_exact(ref.prepare(x.cuda(), metric, F32), labels, 30.0, dtype=F32, d=d32, G=G)
    return o64, o32


@pytest.mark.parametrize("metric", ["sqeuclidean", "cosine"])
def test_lisi_and_label_transfer(dev, metric):
    x, _, _, modality, lab = _api_case(metric)
    xd = x.to(dev)
    for name, labels in (("two modalities", modality), ("ten labels", lab + 7)):     # + 7: any values, relabelled
        o64, o32 = _restated(metric, labels)
        got = mixing.lisi(xd, labels.to(dev), metric=metric)
        assert got.shape == (1000,) and got.dtype == F32 and got.is_cuda
        _close(f"lisi {metric} {name}", got, ref.lisi_from_sums(o64), ref.lisi_from_sums(o32))
        predicted, conf = mixing.label_transfer(xd, labels, metric=metric)              # host labels are taken too
        (t64, c64), (_, c32) = ref.vote(o64), ref.vote(o32)
        decided = ref.decided_rows(o64, o32)
        values = torch.unique(labels)
        assert int((~decided).sum()) <= 10
        assert torch.equal(predicted.cpu()[decided], values[t64.cpu()][decided])
        _close(f"confidence {metric} {name}", conf, c64, c32)
        acc = mixing.label_transfer_accuracy(xd, labels, metric=metric)
        assert acc.dim() == 0 and acc.is_cuda
        assert abs(float(acc) - int((predicted.cpu() == labels).sum()) / 1000) <= 2 * U     # an f32 mean of 0 / 1 values
        m = mixing.label_masses(xd, labels, metric=metric, return_matrix=True)
        p64, p32 = o64 / o64.sum(1, keepdim=True), o32 / o32.sum(1, keepdim=True)
        _close(f"p {metric} {name}", m.p, p64, p32)
        assert m.num_labels == len(values) and torch.equal(m.values.cpu(), values)
        assert torch.equal(m.lisi, got) and torch.equal(m.confidence, conf)            # the matrix changes no statistic


def test_six_hundred_labels_take_two_walks(dev):
    x, _, _, _, _ = _api_case("sqeuclidean")
    labels = torch.randperm(1000, generator=torch.Generator().manual_seed(8)) % 600
    o64, o32 = _restated("sqeuclidean", labels)
    m = mixing.label_masses(x.to(dev), labels.to(dev), return_matrix=True)
    assert m.num_labels == 600 and m.p.shape == (1000, 600)
    _close("lisi 600 labels", m.lisi, ref.lisi_from_sums(o64), ref.lisi_from_sums(o32))
    s64, s32 = ref.stats(o64), ref.stats(o32)
    _close("mass 600 labels", m.mass, s64[0], s32[0])
    _close("sumsq 600 labels", m.sumsq, s64[1], s32[1])
    _close("confidence 600 labels", m.confidence, ref.vote(o64)[1], ref.vote(o32)[1])
    # the merged vote is the vote over the kernel's own 600 columns, ties to the lower label
    own = ref.stats(m.p)
    assert torch.equal(m.top, own[2]) and bool((m.top >= 512).any()) and bool((m.top < 512).any())
    decided = ref.decided_rows(o64, o32)
    print(f"600 labels: {int((~decided).sum())} near-ties")
    assert torch.equal(m.top.cpu()[decided], s64[2].cpu()[decided])


def test_bandwidth_reuse_and_row_blocks(dev):
    x, _, _, modality, lab = _api_case("sqeuclidean")
    xd, ld = x.to(dev), lab.to(dev)
    base = mixing.label_masses(xd, ld)
    bw = manifold.perplexity_bandwidths(xd, 30.0)
    reuse = mixing.label_masses(xd, ld, bandwidths=bw)
    for f in ("mass", "sumsq", "top", "confidence", "beta", "entropy"):
        assert torch.equal(getattr(base, f), getattr(reuse, f)), f
    # row blocks of 64 against the whole cloud: 1000 keys are 16 tiles, and 16 query blocks x 16 <= 512 workgroups, so
    # the full call and every row block give each key tile a split of its own - one plan, the same bits
    assert ops.sim_lse_bias_plan(1000, 1000)[1] == 16 == ops.sim_lse_bias_plan(64, 1000)[1] == ops.sim_lse_bias_plan(40, 1000)[1]
    blocked = mixing.label_masses(xd, ld, bandwidths=bw, row_block=64)
    for f in ("mass", "sumsq", "top", "confidence"):
        assert torch.equal(getattr(base, f), getattr(blocked, f)), f
    assert torch.equal(mixing.lisi(xd, ld, row_block=64), base.lisi)


def test_integration_scores(dev):
    """The medians are compared within the bound of the per-point values: the median moves by no more than the largest
    move of a point.  The accuracy may differ from the f64 vote's by the near-tie rows alone."""
    x, _, _, modality, lab = _api_case("cosine")
    xd = x.to(dev)
    got = mixing.integration_scores({"pert_emb": xd[500:], "cell_emb": xd[:500]}, labels=lab, perplexity=30.0)
    assert set(got) == {"ilisi", "ilisi_scaled", "clisi", "clisi_scaled", "label_transfer_accuracy"}
    assert all(isinstance(v, float) for v in got.values())
    for key, labels, G in (("ilisi", modality, 2), ("clisi", lab, 10)):
        o64, o32 = _restated("cosine", labels)
        l64, l32 = ref.lisi_from_sums(o64), ref.lisi_from_sums(o32)
        bound = max(8 * float((l32.double() - l64).abs().max()), 64 * U * float(l64.max()))
        med = ref.median(l64)
        print(f"{key}: kernel {got[key]:.6f}  f64 restatement {med:.6f}  difference {abs(got[key] - med):.3e}  bound "
              f"{bound:.3e}  fraction {abs(got[key] - med) / bound:.3f}")
        assert abs(got[key] - med) <= bound
        scaled = ref.ilisi_scaled(got[key], G) if key == "ilisi" else ref.clisi_scaled(got[key], G)
        assert got[key + "_scaled"] == scaled
    near = int((~ref.decided_rows(o64, o32)).sum())
    acc64 = float((ref.vote(o64)[0].cpu() == lab).double().mean())
    assert abs(got["label_transfer_accuracy"] - acc64) <= near / 1000 + 1e-12
    only = mixing.integration_scores([xd[:500], xd[500:]])
    assert set(only) == {"ilisi", "ilisi_scaled"} and only["ilisi"] == got["ilisi"]


# ------------------------------------------------------------------------------------------------ 6: meaning
def test_meaning(dev):
    N, P = 1000, 60
    both, blob = ref.blobs(2 * N, P, 77)                                   # four blobs of spread 0.35, two samples of N rows
    x, other, blob = both[:N].contiguous(), both[N:].clone(), blob[:N]
    xd = x.to(dev)
    # labels = the blob: neighbourhoods of one label
    clisi = mixing.median_score(mixing.lisi(xd, blob.to(dev)))
    print(f"four blobs, labels = blob: median cLISI {clisi:.6f}")
    assert abs(clisi - 1.0) <= 1e-3
    # two balanced labels assigned at random: the restatement's value within the per-point bound
    rnd = torch.randperm(N, generator=torch.Generator().manual_seed(5)) % 2
    d64, d32 = ref.sq_dists(x.double().cuda()), ref.sq_dists(x.cuda())
    l64 = ref.lisi_from_sums(ref.label_sums_exact(x.double().cuda(), rnd, 30.0, d=d64))
    l32 = ref.lisi_from_sums(ref.label_sums_exact(x.cuda(), rnd, 30.0, dtype=F32, d=d32))
    got = mixing.lisi(xd, rnd.to(dev))
    bound = _close("lisi of random labels", got, l64, l32)
    ilisi, med = mixing.median_score(got), ref.median(l64)
    print(f"random balanced labels: median iLISI {ilisi:.6f}  f64 restatement {med:.6f}  bound {bound:.3e}")
    assert abs(ilisi - med) <= bound and ilisi > 1.8
    # two modalities, the second a fresh sample of the same blobs moved 10 blob spreads away along the first axis
    other[:, 0] += 10 * 0.35
    scores = mixing.integration_scores([xd, other.to(dev)], metric="sqeuclidean")
    print(f"two modalities 10 spreads apart: {scores}")
    assert scores["ilisi_scaled"] < 0.01
    mixed = mixing.integration_scores([xd[:N // 2], xd[N // 2:]], metric="sqeuclidean")
    print(f"one cloud cut into two modalities: {mixed}")
    assert mixed["ilisi_scaled"] > 0.8


# ------------------------------------------------------------------------------------------------ 7: graph capture
def test_label_masses_graph_capture(dev):
    x, _, _, _, lab = _api_case("sqeuclidean")
    xd, ld = x.to(dev), lab.to(dev)
    bw = manifold.perplexity_bandwidths(xd, 30.0)
    eager = mixing.label_masses(xd, ld, num_labels=10, bandwidths=bw, return_matrix=True)
    assert eager.values is None and torch.equal(eager.predicted, eager.top)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mixing.label_masses(xd, ld, num_labels=10, bandwidths=bw, return_matrix=True)
    torch.cuda.current_stream().wait_stream(side)
    graph, keep = torch.cuda.CUDAGraph(), []
    with ops.owned_by_capture(keep), torch.cuda.graph(graph):                         # one stream, no parallel branches
        out = mixing.label_masses(xd, ld, num_labels=10, bandwidths=bw, return_matrix=True)
    for _ in range(2):
        for t in (out.mass, out.sumsq, out.confidence, out.p):
            t.fill_(-1.0)
        out.top.fill_(-1)
        graph.replay()
        torch.cuda.synchronize()
        for f in ("mass", "sumsq", "top", "confidence", "p"):
            assert torch.equal(getattr(out, f), getattr(eager, f)), f
        assert torch.equal(out.lisi, eager.lisi)
