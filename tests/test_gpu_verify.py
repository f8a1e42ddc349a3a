"""fr_verify_pairs and facerecognition_amd.verification on the GPU against tests/verify_ref.py (float64).

Exact-grid inputs (entries multiples of 1/8, normalize = 0: every score is a multiple of 1/64 and every sum of scores is
exact in float32) must equal the oracle in every output, ties included.  Float inputs are judged with
delta = (D + 8) 2^-24 (derivation in tests/verify_ref.py): counts between the oracle's at t + delta and t - delta,
histograms equal up to pairs within delta of an edge, scores within delta, indices equal where the runner-up is more
than 2 delta away, row sums within (N - 1) delta.

Shapes: N = 130 is three row tiles with a tail of 2; D = 64 is one whole D chunk and D = 20 a ragged one; N = 1100
crosses the 1024-column chunk over which row partials are kept (two chunks, 18 row tiles); N = 2 is the smallest call.
"""
import functools

import numpy as np
import pytest

from tests import verify_ref as R

pytestmark = pytest.mark.gpu

KEYS = ("totals", "counts", "hist", "row_score", "row_idx", "row_sum")
CHUNK = 1024


def min_ws(n):
    return 4 * 64 * ((n + 63) // 64) + 2048 * ((n + CHUNK - 1) // CHUNK)


def run(gpu, E, labels, thr=(), nbins=0, rng=(-1.0, 1.0), normalize=True, rows=True, **kw):
    import torch

    from facerecognition_amd import verification as V

    out = V.verify_pairs(torch.from_numpy(E).to(gpu), torch.from_numpy(np.asarray(labels, np.int32)).to(gpu), thr, nbins,
                         rng, normalize, rows, **kw)
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def attained_thresholds(S):
    """Thresholds exactly ON attained scores (five of them, the extremes included) and midway between grid values."""
    vals = np.unique(S[np.triu_indices(len(S), 1)])
    on = vals[[0, len(vals) // 4, len(vals) // 2, 3 * len(vals) // 4, -1]]
    return np.r_[on, on[1:4] + 1.0 / 128, 0.0, 1.0 / 128].astype(np.float32)


@functools.lru_cache(maxsize=None)
def grid_ref(N, D):
    E, labels = R.grid_case(N, D, seed=3)
    S = R.scores(E, False)
    thr = attained_thresholds(S)
    return E, labels, thr, R.all_pairs(S, labels, thr, 512, -64.0, 64.0)


def assert_equal(got, ref, keys=KEYS):
    for k in keys:
        assert np.array_equal(np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)), k


@pytest.mark.parametrize("N,D", [(130, 64), (130, 20), (1100, 16)])
def test_exact_grid_equals_the_float64_oracle(gpu, N, D):
    """(1100, 16): the 1024-column chunk is crossed, row sums and counts stay exact."""
    E, labels, thr, ref = grid_ref(N, D)
    assert sorted(np.bincount(labels)[[7, 3]]) == [1, 2] and np.bincount(labels)[0] > N // 4
    ties = np.sum(ref["runner_up"] == ref["row_score"])
    assert ties > N // 4  # the grid produces equal scores in quantity: the lowest-index rule is exercised
    assert ref["totals"].sum() == N * (N - 1) // 2 and ref["counts"][:5, :].sum() > 0
    got = run(gpu, E, labels, thr, 512, (-64.0, 64.0), normalize=False)
    assert_equal(got, ref)
    # the same without row outputs: only the upper triangle is swept
    got = run(gpu, E, labels, thr, 512, (-64.0, 64.0), normalize=False, rows=False)
    assert_equal(got, ref, ("totals", "counts", "hist"))
    assert got["row_score"] is None and got["row_idx"] is None and got["row_sum"] is None


@pytest.mark.parametrize("N", [2, 70])
def test_one_label_and_all_distinct_labels(gpu, N):
    E = R.grid_case(N, 16, seed=5)[0]
    S = R.scores(E, False)
    for labels in (np.full(N, 5, np.int32), np.arange(N, dtype=np.int32) - 3):
        ref = R.all_pairs(S, labels, [0.0, -0.25], 64, -16.0, 16.0)
        got = run(gpu, E, labels, [0.0, -0.25], 64, (-16.0, 16.0), normalize=False)
        assert_equal(got, ref)
    assert np.all(got["row_idx"][:, :2] == -1) and np.all(got["row_score"][:, 0] == -np.inf)  # all distinct: no mate
    assert np.all(got["row_score"][:, 1] == np.inf) and got["totals"].tolist() == [0, N * (N - 1) // 2]
    got = run(gpu, E, np.full(N, 5, np.int32), normalize=False)
    assert np.all(got["row_idx"][:, 2] == -1) and np.all(got["row_score"][:, 2] == -np.inf)  # one label: no impostor
    assert got["counts"].shape == (0, 2) and got["hist"] is None


def test_optional_outputs_are_left_alone(gpu):
    """hist, the row pair and row_sum NULL in turn: the others are as before, and the slices of one sentinel-filled
    allocation that were not passed keep the sentinel (they sit between the ones that were)."""
    import torch

    from facerecognition_amd import verification as V

    N, D, nb = 130, 20, 512
    E, labels, thr, ref = grid_ref(N, D)
    e, y = torch.from_numpy(E).to(gpu), torch.from_numpy(labels).to(gpu)
    sizes = dict(counts=2 * len(thr), hist=2 * nb, row_score=3 * N, row_idx=3 * N, row_sum=2 * N, totals=2)
    SENT = 0x5A5A5A5A5A5A5A5A
    for skip in ((), ("hist",), ("row_score", "row_idx"), ("row_sum",), ("hist", "row_score", "row_idx", "row_sum")):
        buf = torch.full((sum(sizes.values()),), SENT, dtype=torch.int64, device=gpu)
        views, at = {}, 0
        for k, n in sizes.items():
            views[k] = buf[at:at + n]
            at += n
        arg = {k: (None if k in skip else v) for k, v in views.items()}
        as_f32 = lambda t: None if t is None else t.view(torch.float32)  # noqa: E731  (the first half of the slice)
        as_i32 = lambda t: None if t is None else t.view(torch.int32)  # noqa: E731
        if "hist" not in skip:
            views["hist"].zero_()  # hist is added to
        V._call(e, y, thr, arg["counts"], arg["totals"], arg["hist"], nb, -64.0, 64.0, as_f32(arg["row_score"]),
                as_i32(arg["row_idx"]), as_f32(arg["row_sum"]), False)
        host = {k: v.cpu() for k, v in views.items()}
        for k in skip:
            assert torch.all(host[k] == SENT), (skip, k)
        assert np.array_equal(host["totals"].numpy(), ref["totals"]) and np.array_equal(host["counts"].numpy().reshape(-1, 2), ref["counts"])
        if "hist" not in skip:
            assert np.array_equal(host["hist"].numpy().reshape(2, nb), ref["hist"])
        if "row_score" not in skip:
            assert np.array_equal(host["row_score"].view(torch.float32)[:3 * N].numpy().reshape(N, 3), ref["row_score"])
            assert np.array_equal(host["row_idx"].view(torch.int32)[:3 * N].numpy().reshape(N, 3), ref["row_idx"])
            assert torch.all(host["row_score"].view(torch.int32)[3 * N:] == 0x5A5A5A5A)  # written no further than [N][3]
        if "row_sum" not in skip:
            assert np.array_equal(host["row_sum"].view(torch.float32)[:2 * N].numpy().reshape(N, 2), ref["row_sum"])


FLOAT_N, FLOAT_D, FLOAT_SEED, FLOAT_BINS = 300, 64, 1, 32
FLOAT_THR = R.SWEEP.astype(np.float32)


@functools.lru_cache(maxsize=None)
def float_ref():
    E, labels = R.float_case(FLOAT_N, FLOAT_D, FLOAT_SEED)
    return E, labels, R.scores(E, True)


def test_float_rows_within_the_derived_bounds(gpu):
    E, labels, S = float_ref()
    N, d = FLOAT_N, R.delta(FLOAT_D)
    norms = np.linalg.norm(E, axis=1)
    assert norms.min() < 0.9 and norms.max() > 3.0  # rows not of unit length
    # the condition on the seed: at most 0.1 % of the pairs within delta of a threshold or an edge
    near = R.near_fraction(S, labels, FLOAT_THR, FLOAT_BINS, -1.0, 1.0, d)
    print(f"  pairs within delta of a threshold or edge: {100 * near:.4f} %")
    assert near <= 1e-3
    ref = R.all_pairs(S, labels, FLOAT_THR, FLOAT_BINS, -1.0, 1.0)
    got = run(gpu, E, labels, FLOAT_THR, FLOAT_BINS, (-1.0, 1.0), normalize=True)
    assert np.array_equal(got["totals"], ref["totals"])
    hi = R.all_pairs(S - d, labels, FLOAT_THR)["counts"]  # s > t + delta
    lo = R.all_pairs(S + d, labels, FLOAT_THR)["counts"]  # s > t - delta
    assert np.all(hi <= got["counts"]) and np.all(got["counts"] <= lo)
    assert hi.sum() > 0
    # histograms: a pair whose bin is the same at s - delta and s + delta must be in it, the others in either
    iu = np.triu_indices(N, 1)
    s, gen = S[iu], (labels[:, None] == labels[None, :])[iu]
    b0, b1 = R.bins(s - d, FLOAT_BINS, -1.0, 1.0), R.bins(s + d, FLOAT_BINS, -1.0, 1.0)
    for c, mask in enumerate((gen, ~gen)):
        sure = np.bincount(b0[mask & (b0 == b1)], minlength=FLOAT_BINS)
        amb = mask & (b0 != b1)
        may = np.bincount(b0[amb], minlength=FLOAT_BINS) + np.bincount(b1[amb], minlength=FLOAT_BINS)
        assert np.all(sure <= got["hist"][c]) and np.all(got["hist"][c] <= sure + may)
        assert got["hist"][c].sum() == ref["totals"][c]
    err = np.abs(got["row_score"].astype(np.float64) - ref["row_score"])
    print(f"  row_score: largest error / delta = {err.max() / d:.3g}")
    assert np.all(err <= d)
    clear = ~(np.abs(ref["row_score"] - ref["runner_up"]) <= 2 * d)  # (no runner-up: nan, clear)
    assert clear.mean() > 0.99
    assert np.array_equal(got["row_idx"][clear], ref["row_idx"][clear])
    assert np.all((got["row_idx"] >= -1) & (got["row_idx"] < N))
    err = np.abs(got["row_sum"].astype(np.float64) - ref["row_sum"])
    print(f"  row_sum: largest error / ((N - 1) delta) = {err.max() / ((N - 1) * d):.3g}")
    assert np.all(err <= (N - 1) * d)


def test_repeatable_and_independent_of_the_workspace(gpu):
    """Two runs give equal bits; the minimum workspace (64-row bands), twice that and the recommended one give the
    same bits.  N = 1100 is 18 bands at the minimum and two column chunks."""
    E, labels = R.float_case(1100, 16, seed=4, classes=30)
    runs = [run(gpu, E, labels, FLOAT_THR, 2048, (-1.0, 1.0), ws_bytes=ws)
            for ws in (None, None, min_ws(1100), 2 * min_ws(1100))]
    for other in runs[1:]:
        for k in KEYS:
            assert np.array_equal(runs[0][k].view(np.uint8), other[k].view(np.uint8)), k
    assert runs[0]["totals"].sum() == 1100 * 1099 // 2 and runs[0]["hist"].sum() == 1100 * 1099 // 2


def test_hist_accumulates_counts_and_totals_are_overwritten(gpu):
    import torch

    E, labels, thr, ref = grid_ref(130, 20)
    hist = torch.zeros((2, 512), dtype=torch.int64, device=gpu)
    for k in (1, 2, 3):
        got = run(gpu, E, labels, thr, 512, (-64.0, 64.0), normalize=False, hist=hist)
        assert np.array_equal(got["hist"], k * ref["hist"])
        assert np.array_equal(got["counts"], ref["counts"]) and np.array_equal(got["totals"], ref["totals"])


# ---- the host layer on a planted set: 20 tight clusters of 8 rows, two rows deliberately mislabelled ----
PLANT_CLASSES, PLANT_PER, PLANT_D, PLANT_SEED, PLANT_BINS = 20, 8, 32, 10, 64
PLANT_FARS = (1e-1, 1e-2, 1e-3, 1e-6)
MISLABELLED = (3, 45)  # row 3 (cluster 0) carries cluster 1's label, row 45 (cluster 5) cluster 9's


@functools.lru_cache(maxsize=None)
def planted():
    rng = np.random.default_rng(PLANT_SEED)
    cluster = np.repeat(np.arange(PLANT_CLASSES), PLANT_PER)
    E = rng.standard_normal((PLANT_CLASSES, PLANT_D))[cluster] + 0.25 * rng.standard_normal((len(cluster), PLANT_D))
    E *= rng.uniform(0.5, 2.0, size=(len(cluster), 1))
    labels = cluster * 7 + 1000
    labels[MISLABELLED[0]] = 1 * 7 + 1000
    labels[MISLABELLED[1]] = 9 * 7 + 1000
    E = E.astype(np.float32)
    return E, labels, R.scores(E, True)


def test_compute_verification_accuracy_on_a_planted_set(gpu):
    import torch

    from facerecognition_amd import verification as V

    E, labels, S = planted()
    d = R.delta(PLANT_D)
    assert R.near_fraction(S, labels, FLOAT_THR, 0, -1, 1, d) == 0.0  # no pair within delta of a sweep threshold
    ref = R.verification_accuracy_all_pairs(E, labels)
    for emb, lab in ((torch.from_numpy(E).to(gpu), labels), (E, labels.tolist()),
                     (torch.from_numpy(E).to(gpu), torch.from_numpy(labels).to(gpu))):
        acc, thr, m = V.compute_verification_accuracy(emb, lab)
        assert acc == pytest.approx(ref[0], abs=1e-12) and thr == ref[1] and m["threshold"] == ref[1]
        assert m["accuracy"] == acc and 0.9 < acc < 1.0  # the mislabelled rows cost accuracy
        assert (m["num_pos_pairs"], m["num_neg_pairs"]) == (ref[2]["num_pos_pairs"], ref[2]["num_neg_pairs"])
        assert abs(m["pos_sim_mean"] - ref[2]["pos_sim_mean"]) <= d and abs(m["neg_sim_mean"] - ref[2]["neg_sim_mean"]) <= d
    # a singleton row is dropped first; num_pairs is accepted and ignored
    acc2, thr2, m2 = V.compute_verification_accuracy(np.r_[E, 2 * E[:1]], np.r_[labels, 5], 10000, 0.5)
    assert (acc2, thr2, m2["num_pos_pairs"], m2["num_neg_pairs"]) == (acc, thr, m["num_pos_pairs"], m["num_neg_pairs"])


def test_verification_report_on_a_planted_set(gpu):
    import torch

    from facerecognition_amd import verification as V

    E, labels, S = planted()
    n, d = len(labels), R.delta(PLANT_D)
    e = torch.from_numpy(E).to(gpu)
    _, inv = np.unique(labels, return_inverse=True)
    n_gen, n_imp = (int(v) for v in R.all_pairs(S, inv)["totals"])

    # 64 bins: no pair lies within delta of an edge, so the histograms and all that is read from them are the oracle's
    ref = R.all_pairs(S, inv, (), PLANT_BINS, -1.0, 1.0)
    assert R.near_fraction(S, inv, (), PLANT_BINS, -1.0, 1.0, d) == 0.0
    rep = V.verification_report(e, labels, fars=PLANT_FARS, hist_bins=PLANT_BINS)
    assert (rep["genuine_pairs"], rep["impostor_pairs"]) == (n_gen, n_imp)
    assert np.array_equal(rep["hist"], ref["hist"])
    roc = V.roc_from_histograms(ref["hist"], (-1.0, 1.0))
    assert rep["roc"]["eer_bin"] == roc["eer_bin"] and rep["eer"] == roc["eer"] and rep["auc"] == roc["auc"]
    assert 0.95 < rep["auc"] <= 1.0 and 0 < rep["eer"] < 0.05 and rep["dprime"] > 3

    # TAR at FAR with the default 2048 bins: the rule replayed on the float64 scores, and the exact quantile
    rep = V.verification_report(e, labels, fars=PLANT_FARS)
    assert rep["hist"].shape == (2, 2048) and rep["hist"].sum(1).tolist() == [n_gen, n_imp]
    ks, thr = V.far_candidates(rep["hist"][1], n_imp, PLANT_FARS, (-1.0, 1.0))
    assert R.near_fraction(S, inv, thr.reshape(-1), 0, -1, 1, d) == 0.0  # no pair within delta of a candidate threshold
    c = R.all_pairs(S, inv, thr.reshape(-1))["counts"].reshape(len(PLANT_FARS), -1, 2)
    iu = np.triu_indices(n, 1)
    genuine = S[iu][(inv[:, None] == inv[None, :])[iu]]
    impostor = np.sort(S[iu][(inv[:, None] != inv[None, :])[iu]])[::-1]
    for f, entry in enumerate(rep["tar_at_far"]):
        m = int(np.argmax(c[f, :, 1] <= ks[f]))
        assert entry["threshold"] == float(thr[f, m]) and entry["false_accepts"] == c[f, m, 1] <= ks[f]
        assert entry["tar"] == c[f, m, 0] / n_gen and entry["far"] == c[f, m, 1] / n_imp
        k, tar = R.tar_at_far(S, inv, PLANT_FARS[f])
        assert k == ks[f] == int(PLANT_FARS[f] * n_imp)
        # the reported threshold is less than one sub-step (2 / 2048 / 16) above the exact quantile, the (k + 1)-th
        # highest impostor score; the two TARs differ by the genuine pairs in between, of which this set has none
        assert 0 <= entry["threshold"] - impostor[k] < 2 / 2048 / 16 + d
        assert not np.any((genuine > impostor[k] - d) & (genuine <= entry["threshold"] + d))
        assert entry["tar"] == tar
        assert (entry["note"] != "") == (k == 0)
    assert ks[-1] == 0 and "zero false accepts" in rep["tar_at_far"][-1]["note"]  # 1e-6 < 1 / impostor pairs

    # leave-one-out rank-1: no row's best mate is within 2 delta of its best impostor, so the decisions are the oracle's
    full = R.all_pairs(S, inv)
    assert np.abs(full["row_score"][:, 0] - full["row_score"][:, 2]).min() > 2 * d
    rank1, rows_with_mate = R.loo_rank1(full)
    assert (rep["rank1"], rep["rank1_rows"]) == (rank1, rows_with_mate) and rows_with_mate == n
    assert 0.9 < rank1 <= (n - 2) / n  # the two mislabelled rows lose to their own cluster

    # label noise: every pair listed first involves a mislabelled row, and both rows show up
    hard = rep.hardest_impostors(2 * (PLANT_PER - 1))
    assert all(a in MISLABELLED or b in MISLABELLED for a, b, _ in hard), hard
    assert {x for a, b, _ in hard for x in (a, b)} >= set(MISLABELLED)
    assert all(s > 0.7 for _, _, s in hard) and [s for _, _, s in hard] == sorted((s for _, _, s in hard), reverse=True)
    assert len({(min(a, b), max(a, b)) for a, b, _ in hard}) == len(hard)  # each unordered pair once
    assert rep["hardest_impostors"] == rep.hardest_impostors(10)
    easy = rep.hardest_genuines(2)
    assert all(a in MISLABELLED or b in MISLABELLED for a, b, _ in easy) and all(s < 0.5 for _, _, s in easy)
