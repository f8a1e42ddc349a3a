"""tests/verify_ref.py (the float64 checker of the all-pairs verification) on hand-computed cases, against the
reference's own output on one seeded input (tests/golden/verify_golden.npz, made by tools/gen_verify_golden.py), and
the agreement of the all-pairs balanced accuracy with the reference's sampled estimate.  No GPU."""
import os

import numpy as np

from tests import verify_ref as R

INF = np.inf
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "verify_golden.npz")

# four rows, two classes; every score is a multiple of 1/4
E4 = np.array([[1, 0], [0.5, 0.75], [0, 1], [-1, 0]], np.float64)
L4 = np.array([0, 0, 1, 1])


def test_four_rows_by_hand():
    S = R.scores(E4, False)
    assert np.array_equal(S, [[1, 0.5, 0, -1], [0.5, 0.8125, 0.75, -0.5], [0, 0.75, 1, 0], [-1, -0.5, 0, 1]])
    r = R.all_pairs(S, L4, [0.0, 0.5, 0.25], nbins=4, lo=-1, hi=1)
    # genuine pairs (0, 1) = 0.5 and (2, 3) = 0; impostors (0, 2) = 0, (0, 3) = -1, (1, 2) = 0.75, (1, 3) = -0.5
    assert r["totals"].tolist() == [2, 4]
    assert r["counts"].tolist() == [[1, 1], [0, 1], [1, 1]]  # 0.5 > 0.5 is false: the comparison is strict
    assert r["hist"].tolist() == [[0, 0, 1, 1], [1, 1, 1, 1]]  # bin = floor((s + 1) * 2)
    assert r["row_score"].tolist() == [[0.5, 0.5, 0], [0.5, 0.5, 0.75], [0, 0, 0.75], [0, 0, -0.5]]
    assert r["row_idx"].tolist() == [[1, 1, 2], [0, 0, 2], [3, 3, 1], [2, 2, 1]]
    assert r["row_sum"].tolist() == [[0.5, -1], [0.5, 0.25], [0, 0.75], [0, -1.5]]
    assert R.loo_rank1(r) == (0.5, 4)  # rows 0 and 3 win, rows 1 and 2 lose to an impostor at 0.75


def test_ties_go_to_the_lowest_index_and_the_diagonal_is_no_pair():
    S = np.full((5, 5), 0.25)
    np.fill_diagonal(S, 9.0)  # would win every slot if the diagonal counted
    r = R.all_pairs(S, [0, 0, 0, 1, 1])
    assert r["row_idx"].tolist() == [[1, 1, 3], [0, 0, 3], [0, 0, 3], [4, 4, 0], [3, 3, 0]]
    assert np.all(r["row_score"] == 0.25)
    assert r["row_sum"].tolist() == [[0.5, 0.5], [0.5, 0.5], [0.5, 0.5], [0.25, 0.75], [0.25, 0.75]]
    assert r["runner_up"][0].tolist() == [0.25, 0.25, 0.25] and np.isnan(r["runner_up"][3, 0])


def test_singleton_class_and_single_class():
    S = R.scores(np.array([[1.0, 0], [0.5, 0.5], [0, 2.0]]), False)
    r = R.all_pairs(S, [4, 4, -9], [0.25])
    assert r["totals"].tolist() == [1, 2] and r["counts"].tolist() == [[1, 1]]  # (0, 1) = 0.5, (1, 2) = 1, (0, 2) = 0
    assert r["row_score"][2].tolist() == [-INF, INF, 1.0] and r["row_idx"][2].tolist() == [-1, -1, 1]
    assert r["row_sum"][2].tolist() == [0, 1.0]
    r = R.all_pairs(S, [1, 1, 1])
    assert r["totals"].tolist() == [3, 0]
    assert np.all(r["row_score"][:, 2] == -INF) and np.all(r["row_idx"][:, 2] == -1)
    assert R.loo_rank1(r) == (1.0, 3)
    r = R.all_pairs(S, [1, 2, 3])
    assert r["totals"].tolist() == [0, 3] and np.all(r["row_idx"][:, :2] == -1)
    assert np.all(r["row_score"][:, 0] == -INF) and np.all(r["row_score"][:, 1] == INF)


def test_normalisation_is_the_references_and_bins_clamp():
    S = R.scores(np.array([[3.0, 4.0], [0.0, 2.0]]), True)
    assert S[0, 1] == (8.0 * (1 / (5 + 1e-8))) * (1 / (2 + 1e-8)) and abs(S[0, 1] - 0.8) < 1e-8
    assert S[0, 0] < 1.0  # (|a| / (|a| + 1e-8))^2
    assert R.bins([-70, -64, -63.75, 0, 63.9, 64, 1e9], 512, -64, 64).tolist() == [0, 0, 1, 256, 511, 511, 511]
    assert R.bins([0.1], 3, 0, 1).tolist() == [0]  # inv_w is float32(3) / float32(1)
    assert R.delta(64) == 72 * 2.0 ** -24


def test_tar_at_far_by_hand():
    # impostor scores of E4: 0.75, 0, -0.5, -1; genuine 0.5, 0
    S = R.scores(E4, False)
    assert R.tar_at_far(S, L4, 0.2) == (0, 0.0)   # no false accept allowed: threshold 0.75, no genuine above
    assert R.tar_at_far(S, L4, 0.25) == (1, 0.5)  # one allowed: threshold 0, and the genuine 0 is not above it (strict)
    assert R.tar_at_far(S, L4, 0.5) == (2, 1.0)


def _clusters(classes, per, D, spread, seed):
    rng = np.random.default_rng(seed)
    labels = np.repeat(np.arange(classes), per)
    E = rng.standard_normal((classes, D))[labels] + spread * rng.standard_normal((classes * per, D))
    return E.astype(np.float32), labels


def test_all_pairs_function_drops_singletons_and_returns_early_like_the_reference():
    E, labels = _clusters(6, 4, 8, 0.8, seed=1)
    full = R.verification_accuracy_all_pairs(E, labels)
    extra = R.verification_accuracy_all_pairs(np.r_[E, E[:2] * 3], np.r_[labels, [77, 78]])
    assert full[:2] == extra[:2] and full[2] == extra[2]
    assert set(full[2]) == {"accuracy", "threshold", "pos_sim_mean", "neg_sim_mean", "num_pos_pairs", "num_neg_pairs"}
    assert full[2]["num_pos_pairs"] == 6 * 6 and full[2]["num_neg_pairs"] == 24 * 23 // 2 - 36
    for fn in (R.verification_accuracy_all_pairs, lambda e, y: R.verification_accuracy_sampled(e, y, np.random.RandomState(0))):
        assert fn(E[:1], labels[:1]) == (0.0, 0.5, {})
        assert fn(E[:5], [0, 0, 0, 1, 2]) == (0.0, 0.5, {"error": "Not enough valid labels"})


def test_balanced_accuracy_over_all_pairs_agrees_with_the_sampled_estimate():
    """Equal class sizes: the reference's half-genuine, half-impostor sample estimates the balanced accuracy.  Each
    half is a mean of 5000 Bernoulli draws, so the sampled accuracy at a fixed threshold has sigma <= 0.5 / sqrt(10000);
    the margin is 5 sigma = 0.025 (derived, not measured)."""
    E, labels = _clusters(40, 10, 32, 1.4, seed=2)
    acc_all, thr_all, m_all = R.verification_accuracy_all_pairs(E, labels)
    acc_s, thr_s, m_s = R.verification_accuracy_sampled(E, labels, np.random.RandomState(12345), num_pairs=10000)
    print(f"all pairs {acc_all:.4f} at {thr_all:.2f}; sampled {acc_s:.4f} at {thr_s:.2f}")
    assert 0.6 < acc_all < 0.99  # the classes overlap: the comparison is not 1 against 1
    assert abs(acc_all - acc_s) <= 0.025
    assert m_s["num_pos_pairs"] == m_s["num_neg_pairs"] == 5000
    # a mean of 5000 cosines, each in [-1, 1]: sigma <= 1 / sqrt(5000), 5 sigma = 0.071
    assert abs(m_all["pos_sim_mean"] - m_s["pos_sim_mean"]) <= 0.071
    assert abs(m_all["neg_sim_mean"] - m_s["neg_sim_mean"]) <= 0.071


def test_restatement_reproduces_the_references_own_output():
    g = np.load(GOLDEN)
    acc, thr, m = R.verification_accuracy_sampled(g["E"], g["labels"], np.random.RandomState(int(g["seed"])),
                                                  num_pairs=int(g["num_pairs"]))
    assert acc == float(g["accuracy"]) and thr == float(g["best_threshold"])
    assert float(m["pos_sim_mean"]) == float(g["pos_sim_mean"]) and float(m["neg_sim_mean"]) == float(g["neg_sim_mean"])
    assert m["num_pos_pairs"] == int(g["num_pos_pairs"]) and m["num_neg_pairs"] == int(g["num_neg_pairs"])
    assert 0.5 < acc < 1.0 and 0.1 < thr < 0.85  # an informative case: not saturated, not at the sweep's ends
