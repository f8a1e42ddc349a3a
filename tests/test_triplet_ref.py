"""tests/triplet_ref.py against the reference's own output (tests/golden/triplet_golden.npz, written by
tools/gen_triplet_golden.py from the reference's three mining functions and nn.TripletMarginLoss in float64), and the
judge of the GPU tests against planted wrong answers, without a GPU."""
import os

import numpy as np
import pytest

from tests import triplet_ref as R

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "triplet_golden.npz"))
MODES = (("semi", R.SEMI_HARD), ("hard", R.BATCH_HARD), ("first", R.FIRST))


def _gold(key):
    return tuple(GOLD[f"{key}_{k}"] for k in "apn")


@pytest.mark.parametrize("key,mode", MODES)
def test_both_parts_reproduce_the_reference_indices(key, mode):
    E, labels, margin = GOLD["E"], GOLD["labels"], float(GOLD["margin"])
    a, p, n = _gold(key)
    for dist in (R.gram_dist_f32(E), R.dist_f64(E)[0]):
        lims, ra, rp, rn, semi = R.mine(dist, labels, mode, margin)
        assert np.array_equal(ra, a) and np.array_equal(rp, p) and np.array_equal(rn, n), (key, dist.dtype)
        assert lims[-1] == len(a) and np.array_equal(np.diff(lims), np.bincount(a, minlength=len(labels)))
        if key == "semi":
            assert np.array_equal(semi, GOLD["semi_took"])


@pytest.mark.parametrize("key,mode", MODES)
def test_loss_and_gradient_reproduce_torch(key, mode):
    a, p, n = _gold(key)
    r = R.loss_ref(GOLD["E"], a, p, n, float(GOLD["margin"]), float(GOLD["u"]))
    assert not r["unsure"].any()
    assert abs(r["loss"] - GOLD[f"{key}_loss"]) <= 1e-12 * abs(GOLD[f"{key}_loss"])
    ref = GOLD[f"{key}_dE"]
    assert np.abs(r["dE"] - ref).max() <= 1e-12 * np.abs(ref).max()


def test_fixture_contains_every_branch():
    E, labels, margin = GOLD["E"], GOLD["labels"], float(GOLD["margin"])
    assert np.array_equal(E, E.astype(np.float32))  # float32 values: both parts see the same rows
    assert (np.bincount(labels) == 1).any()  # a singleton label
    a, p, n = _gold("semi")
    d = R.dist_f64(E)[0]
    assert (d[a, p] == 0).any() and np.array_equal(E[0], E[1])  # an exact duplicate as positive
    took = GOLD["semi_took"]
    assert took.any() and not took.all()  # both branches
    r = R.loss_ref(E, a, p, n, margin)
    assert (r["x"] < 0).any() and (r["x"] > 0).any()  # an inactive and an active triplet
    assert len(set(a) & set(p) & set(n)) > 0  # a row in all three roles
    assert set(labels[a]) == {0, 1, 2, 3}  # the singletons are never anchors
    # the two fallbacks differ: nearest for the semi-hard rule, farthest for the first-index rule
    fa, fp, fn = _gold("first")
    assert np.array_equal(fa, a) and np.array_equal(fp, p)
    fb = took == 0
    assert (d[a[fb], fn[fb]] > d[a[fb], n[fb]]).all()
    assert (fn[took == 1] <= n[took == 1]).all() and (fn[took == 1] < n[took == 1]).any()


def test_valid_choice_accepts_the_reference_and_rejects_planted_errors():
    E, labels, margin = GOLD["E"], GOLD["labels"], float(GOLD["margin"])
    d, db = R.dist_f64(E)
    for key, mode in MODES:
        for t in zip(*_gold(key)):
            ok, case = R.valid_choice(d, db, labels, mode, margin, *t)
            assert ok and case != "either", (key, t, case)
    a, p, n = _gold("semi")
    took = GOLD["semi_took"]
    rejected = {"second": 0, "not_semi": 0, "labels": 0}
    for ai, pi, ni, tk in zip(a, p, n, took):
        neg, certain, possible = R.pair_case(d, db, labels, margin, ai, pi)
        pool = neg[certain] if tk else neg
        second = pool[np.argsort(d[ai, pool], kind="stable")]
        second = [j for j in second if d[ai, j] > d[ai, ni]]
        if second:  # the second-nearest candidate, across the planted gap
            assert not R.valid_choice(d, db, labels, R.SEMI_HARD, margin, ai, pi, second[0])[0]
            rejected["second"] += 1
        if tk and (~possible).any():  # a negative that is not semi-hard although a certain one exists
            wrong = neg[~possible][np.argmin(d[ai, neg[~possible]])]
            assert not R.valid_choice(d, db, labels, R.SEMI_HARD, margin, ai, pi, wrong)[0]
            assert not R.valid_choice(d, db, labels, R.FIRST, margin, ai, pi, wrong)[0]
            rejected["not_semi"] += 1
        assert not R.valid_choice(d, db, labels, R.SEMI_HARD, margin, ai, pi, pi)[0]  # a positive as negative
        rejected["labels"] += 1
    assert all(v > 0 for v in rejected.values()), rejected
    a, p, n = _gold("hard")
    for ai, pi, ni in zip(a, p, n):
        others = [j for j in np.flatnonzero(labels != labels[ai]) if d[ai, j] > d[ai, ni]]
        assert not R.valid_choice(d, db, labels, R.BATCH_HARD, margin, ai, pi, others[0])[0]
    # the first-index rule: a later semi-hard negative is rejected, the farthest-negative fallback must be the farthest
    a, p, n = _gold("first")
    later = 0
    for ai, pi, ni in zip(a, p, n):
        neg, certain, possible = R.pair_case(d, db, labels, margin, ai, pi)
        if certain.any():
            for j in neg[certain][1:]:
                assert not R.valid_choice(d, db, labels, R.FIRST, margin, ai, pi, j)[0]
                later += 1
        else:
            nearest = neg[np.argmin(d[ai, neg])]
            assert not R.valid_choice(d, db, labels, R.FIRST, margin, ai, pi, nearest)[0]
    assert later > 0


@pytest.mark.parametrize("N,D", R.FLOAT_SHAPES)
def test_gpu_float_inputs_exercise_both_branches(N, D):
    """From float64 alone: the float inputs the GPU tests judge with valid_choice take the semi-hard branch for 20 % to
    80 % of the pairs, and at most 5 % of the pairs are undecided within the bounds."""
    E, labels = R.float_case(N, D, seed=7)
    d, db = R.dist_f64(E)
    lims, a, p, n, semi = R.mine(d, labels, R.SEMI_HARD, R.FLOAT_MARGIN)
    assert len(a) > 4 * N
    assert 0.2 <= semi.mean() <= 0.8, semi.mean()
    for mode in (R.SEMI_HARD, R.FIRST):
        _, a, p, n, _ = R.mine(d, labels, mode, R.FLOAT_MARGIN)
        cases = [R.valid_choice(d, db, labels, mode, R.FLOAT_MARGIN, *t) for t in zip(a, p, n)]
        assert all(ok for ok, _ in cases)
        assert np.mean([c == "either" for _, c in cases]) <= 0.05


def test_grid_inputs_are_exact_and_have_ties():
    for N, D in ((70, 16), (130, 512)):
        E, labels = R.grid_case(N, D, seed=3)
        assert np.array_equal(E * 8, np.round(E * 8)) and np.abs(E).max() <= 2
        sizes = np.bincount(np.unique(labels, return_inverse=True)[1])
        assert {1, 2, 4} <= set(sizes) and sizes.max() >= 20
        d32 = R.gram_dist_f32(E)
        d64 = R.dist_f64(E)[0]
        assert np.array_equal(d32.astype(np.float64) ** 2 > 0, d64 > 0)
        assert np.array_equal(d32, np.sqrt((d64 ** 2).astype(np.float32)))  # the Gram form is exact on the grid
        # deliberate ties: some anchor has two different negatives at exactly its smallest negative distance
        ties = 0
        for i in range(N):
            dn = d32[i, labels != labels[i]]
            ties += (dn == dn.min()).sum() > 1
        assert ties > 0
        for mode in (R.SEMI_HARD, R.BATCH_HARD, R.FIRST):
            lims = R.mine(d32, labels, mode, 0.5)[0]
            assert lims[-1] > 0 and np.array_equal(lims, R.counts(labels, mode))
