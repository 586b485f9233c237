"""CPU: the host side of clip_dplm_amd.mixing (argument errors, the small reductions, the >512-label merge), the binding of
clipk_label_kernel_sums, and the restatement of tests/lisi_ref.py against itself (truncation at k = N - 1, the near-tie
cap of the vote cases the GPU test uses)."""
import pytest
import torch

import lisi_ref as ref

F64 = torch.float64

VOTE_CASES = [(130, 60, 2), (130, 60, 10), (1000, 60, 10), (1000, 60, 64), (1000, 60, 130)]     # tests/test_gpu_lisi.py


# ------------------------------------------------------------------------------------------------ argument errors
def test_every_argument_error_of_mixing():
    """Raised before the device is touched: the clouds below live on the host."""
    import clip_dplm_amd
    from clip_dplm_amd import mixing
    assert clip_dplm_amd.lisi is mixing.lisi and clip_dplm_amd.mixing is mixing
    assert clip_dplm_amd.integration_scores is mixing.integration_scores
    x, lab = torch.zeros(100, 8), torch.arange(100) % 3
    bw = tuple(torch.ones(100) for _ in range(4))
    bad = [
        (dict(x=x, labels=lab, perplexity=99.0), "perplexity"), (dict(x=x, labels=lab, perplexity=0.0), "perplexity"),
        (dict(x=x, labels=lab, perplexity="30"), "perplexity"),
        (dict(x=torch.zeros(2, 8), labels=lab[:2], perplexity=0.5), "rows"),
        (dict(x=x.double(), labels=lab), "float32"), (dict(x=torch.zeros(100, 6), labels=lab), "multiple of 4"),
        (dict(x=torch.zeros(100, 516), labels=lab), "at most 512"), (dict(x=torch.zeros(100), labels=lab), "2-D"),
        (dict(x=[[0.0] * 8] * 100, labels=lab), "tensor"),
        (dict(x=x, labels=lab, metric="euclidean"), "metric"),
        (dict(x=x, labels=lab.float()), "integer"), (dict(x=x, labels=lab[:99]), "entries"),
        (dict(x=x, labels=lab[:, None]), "1-D"), (dict(x=x, labels=list(range(100))), "integer"),
        (dict(x=x, labels=lab, num_labels=0), "num_labels"), (dict(x=x, labels=lab, num_labels=3.0), "num_labels"),
        (dict(x=x, labels=lab, num_labels=True), "num_labels"), (dict(x=x, labels=lab, num_labels=1 << 20), "num_labels"),
        (dict(x=x, labels=lab, row_block=0), "row_block"), (dict(x=x, labels=lab, row_block=64.0), "row_block"),
        (dict(x=x, labels=lab, return_matrix=1), "return_matrix"),
        (dict(x=x, labels=lab, bandwidths=bw[:3]), "bandwidths"), (dict(x=x, labels=lab, bandwidths=bw[0]), "bandwidths"),
        (dict(x=x, labels=lab, bandwidths=(bw[0], bw[1], bw[2], torch.ones(99))), "bandwidths"),
        (dict(x=x, labels=lab, bandwidths=(bw[0].double(),) + bw[1:]), "bandwidths"),
        (dict(x=x, labels=lab), "device"),                               # a host cloud: there is no CPU fallback
        (dict(x=x, labels=lab, bandwidths=bw, num_labels=3), "device"),
    ]
    for kw, word in bad:
        for fn in (mixing.label_masses, mixing.lisi, mixing.label_transfer, mixing.label_transfer_accuracy):
            with pytest.raises((ValueError, TypeError), match=word):
                fn(**kw)
    y = torch.zeros(50, 8)
    bad = [
        (dict(clouds=[x]), "two clouds"), (dict(clouds=x), "sequence"), (dict(clouds={"cell_emb": x}), "two clouds"),
        (dict(clouds=[x, torch.zeros(50, 12)]), "one width"), (dict(clouds=[x, y.double()]), "float32"),
        (dict(clouds=[x, torch.zeros(0, 8)]), "empty"), (dict(clouds=[x, [0.0] * 8]), "float32"),
        (dict(clouds=[x, y], labels=lab), "entries"), (dict(clouds=[x, y], labels=torch.zeros(150)), "integer"),
        (dict(clouds=[x, y], perplexity=149.0), "perplexity"), (dict(clouds=[x, y], metric="l1"), "metric"),
        (dict(clouds=[torch.zeros(100, 6), torch.zeros(50, 6)]), "multiple of 4"),
        (dict(clouds=[x, y]), "device"), (dict(clouds={"pert_emb": x, "cell_emb": y}), "device"),
    ]
    for kw, word in bad:
        with pytest.raises((ValueError, TypeError), match=word):
            mixing.integration_scores(**kw)


def test_dict_clouds_go_in_the_reference_order():
    from clip_dplm_amd import mixing
    a, b, c, d = (torch.full((2, 4), float(i)) for i in range(4))
    got = mixing._cloud_list({"protein_emb": a, "other": d, "cell_emb": b, "pert_emb": c})
    assert [float(t[0, 0]) for t in got] == [1.0, 2.0, 0.0, 3.0]


def test_ops_argument_errors():
    from clip_dplm_amd import ops
    x, lab, beta = torch.zeros(8, 8), torch.zeros(8, dtype=torch.int32), torch.ones(8)
    for kw, exc in ((dict(n_labels=513), ValueError), (dict(n_labels=0), ValueError), (dict(n_labels=2.0), TypeError),
                    (dict(want_out=False, want_stats=False), ValueError), (dict(diag_offset=-2), ValueError),
                    (dict(beta=None), TypeError), (dict(beta=torch.ones(7)), ValueError),
                    (dict(shift=torch.ones(8, dtype=F64)), TypeError), (dict(labels=lab.long()), TypeError),
                    (dict(), ValueError)):                                # host tensors: no CPU fallback
        args = dict(x=x, y=x, labels=lab, n_labels=3, beta=beta)
        args.update(kw)
        with pytest.raises(exc):
            ops.label_kernel_sums(**args)


# ------------------------------------------------------------------------------------------------ the C entry
def test_entry_point_refuses_without_a_launch():
    from clip_dplm_amd import _ffi
    lib = _ffi.load()
    assert lib.clipk_version() == _ffi.ABI_VERSION                       # entry points were added, no signature changed
    for n, nargs in (("clipk_label_kernel_sums", 20), ("clipk_label_kernel_sums_workspace", 4)):
        assert n in _ffi.SIGNATURES and hasattr(lib, n) and len(_ffi.SIGNATURES[n][1]) == nargs

    def lks(Mx, Ny, P, G, diag=-1):
        return lib.clipk_label_kernel_sums(None, Mx, None, Ny, P, None, G, None, None, None, None, diag, None, None, None,
                                           None, None, None, 0, None)

    for Mx, Ny, P, G in ((0, 8, 8, 1), (8, 0, 8, 1), (8, 8, 0, 1), (8, 8, 8, 0), (-1, 8, 8, 1)):
        assert lks(Mx, Ny, P, G) == -1 and lib.clipk_label_kernel_sums_workspace(Mx, Ny, P, G) == 0
    for Mx, Ny, P, G in ((8, 8, 6, 1), (8, 8, 516, 1), (8, 8, 8, 513)):
        assert lks(Mx, Ny, P, G) == -2 and lib.clipk_label_kernel_sums_workspace(Mx, Ny, P, G) == 0
    # a supported shape with null pointers or an offset below -1: a bad argument, not a launch
    assert lks(100, 100, 8, 10) == -1 and lks(100, 100, 8, 10, diag=-2) == -1
    # the slabs: 130 keys split three ways, the row stride G rounded up to 4; the sizes of clipk_label_dist_sums
    assert lib.clipk_label_kernel_sums_workspace(130, 130, 8, 10) == 3 * 130 * 12 * 4
    assert lib.clipk_label_kernel_sums_workspace(66, 130, 8, 512) == lib.clipk_label_dist_sums_workspace(66, 130, 8, 512)


# ------------------------------------------------------------------------------------------------ scalings on hand cases
def test_scalings_on_hand_cases():
    from clip_dplm_amd import mixing
    # equal masses of two labels: LISI exactly 2, scaled exactly 1 (iLISI) / 0 (cLISI)
    out = torch.tensor([[3.0, 3.0], [0.5, 0.5], [7.0, 7.0]], dtype=F64)
    v = ref.lisi_from_sums(out)
    assert torch.equal(v, torch.full((3,), 2.0, dtype=F64))
    assert mixing.median_score(v) == 2.0 == ref.median(v)
    assert mixing.scale_ilisi(2.0, 2) == 1.0 == ref.ilisi_scaled(2.0, 2)
    assert mixing.scale_clisi(2.0, 2) == 0.0 == ref.clisi_scaled(2.0, 2)
    assert mixing.scale_ilisi(1.0, 3) == 0.0 and mixing.scale_clisi(1.0, 3) == 1.0 and mixing.scale_ilisi(2.0, 3) == 0.5
    # the median: the two middle values' mean for an even count, NaN rows (no mass) left out; f32 device-style input
    assert mixing.median_score(torch.tensor([4.0, 1.0, 2.0, 3.0])) == 2.5
    assert mixing.median_score(torch.tensor([float("nan"), 1.0, 5.0, 2.0])) == 2.0

    # two perfectly interleaved labels on a line: every neighbourhood holds both alike - iLISI -> 2, scaled -> 1
    N = 400
    x = torch.zeros(N, 4, dtype=F64)
    x[:, 0] = torch.arange(N, dtype=F64)
    lab = torch.arange(N) % 2
    v = ref.lisi(x, lab, 50.0)
    med = mixing.median_score(v)
    print(f"interleaved labels: median LISI {med:.6f}, scaled {mixing.scale_ilisi(med, 2):.6f}, min {float(v.min()):.6f}")
    assert 1.99 < med <= 2.0 and mixing.scale_ilisi(med, 2) > 0.99

    # two far blobs labelled by blob: every cross term underflows - LISI exactly 1, scaled exactly 0 (iLISI) / 1 (cLISI)
    xb, lb = ref.blobs(200, 8, 3, n_blobs=2, spread=0.35)
    xb = xb.double()
    xb[lb == 1] += 1000.0
    v = ref.lisi(xb, lb, 30.0)
    assert torch.equal(v, torch.ones_like(v))
    med = mixing.median_score(v)
    assert mixing.scale_ilisi(med, 2) == 0.0 and mixing.scale_clisi(med, 2) == 1.0
    top, conf = ref.vote(ref.label_sums_exact(xb, lb, 30.0))
    assert torch.equal(top, lb) and torch.equal(conf, torch.ones_like(conf))


# ------------------------------------------------------------------------------------------------ truncation
def test_knn_truncation_at_all_neighbours_is_the_exact_definition():
    x, lab = ref.vote_case(300, 16, 4, 5)
    exact, knn = ref.lisi(x, lab, 30.0), ref.lisi_knn(x, lab, 30.0, 299)
    dev = float((exact - knn).abs().max())
    print(f"k = N - 1 against the exact restatement: {dev:.3e}")
    assert dev <= 1e-9 * float(exact.max())


def test_record_of_the_3x_perplexity_truncation():
    """A record, not an assertion: how far truncating every neighbourhood to k = 3 x perplexity - the
    published implementation's choice - moves the median on the test blobs."""
    for N, P, G in VOTE_CASES:
        x, lab = ref.vote_case(N, P, G, 100 + G)
        perplexity = ref.case_perplexity(N)
        k = min(N - 1, int(3 * perplexity))
        exact, knn = ref.lisi(x, lab, perplexity), ref.lisi_knn(x, lab, perplexity, k)
        print(f"N={N} P={P} G={G} perplexity={perplexity:g} k={k}: median exact {ref.median(exact):.6f}  truncated "
              f"{ref.median(knn):.6f}  difference {ref.median(knn) - ref.median(exact):+.3e}  per point up to "
              f"{float((exact - knn).abs().max()):.3e}")
        assert bool(torch.isfinite(knn).all())


# ------------------------------------------------------------------------------------------------ more than 512 labels
def test_merge_of_label_blocks():
    from clip_dplm_amd import mixing
    N, G = 300, 600
    x = ref.cloud(N, 16, 9)
    lab = torch.randint(0, G, (N,), generator=torch.Generator().manual_seed(4))
    out = ref.label_sums_exact(x, lab, 30.0, G=G)
    out[5, 3] = out[5, 580] = out[5].max() + 1.0                         # equal maxima in two blocks: the lower label
    out[6, 590] = out[6].max() + 1.0                                     # the maximum in the second block
    mass, sumsq, top, best = ref.stats(out)
    parts = []
    for g0 in (0, 512):
        m, q, t, b = ref.stats(out[:, g0:g0 + 512])
        parts.append((m, q, b, t + g0))
    m, q, b, t = mixing.merge_label_blocks(parts)
    assert torch.equal(t, top) and torch.equal(b, best) and int(t[5]) == 3 and int(t[6]) == 590
    assert float((m - mass).abs().max()) <= 4 * 2.0 ** -52 * float(mass.max())
    assert float((q - sumsq).abs().max()) <= 4 * 2.0 ** -52 * float(sumsq.max())
    one = mixing.merge_label_blocks(parts[:1])
    assert all(a is c for a, c in zip(one, parts[0]))


# ------------------------------------------------------------------------------------------------ the GPU test's inputs
@pytest.mark.parametrize("N,P,G", VOTE_CASES)
def test_vote_cases_stay_under_the_near_tie_cap(N, P, G):
    """tests/test_gpu_lisi.py::test_top allows at most 1 % of a case's rows to be near-ties (the two largest f64 masses
    within twice the bound): the restatement alone stays under it, checked here without a device."""
    x, lab = ref.vote_case(N, P, G, 100 + G)
    d64, d32 = ref.sq_dists(x.double()), ref.sq_dists(x)
    beta, dmin = ref.calibrated(x, ref.case_perplexity(N), d64)
    o64 = ref.label_sums(ref.weights(d64, beta.double(), dmin.double()), lab, G)
    o32 = ref.label_sums(ref.weights(d32, beta, dmin), lab, G)
    near = int((~ref.decided_rows(o64, o32)).sum())
    agree = float((ref.stats(o64)[2] == lab).double().mean())
    print(f"N={N} P={P} G={G}: {near} near-ties of {N} rows; the f64 vote agrees with the labels on {agree:.3f}")
    assert near <= N // 100
