"""facerecognition_amd.evaluate on the CPU: the metric / sweep / ROC / report functions against what the
reference's inference/evaluate.py returned for the same seeded inputs (tests/golden/evaluate_golden.npz,
written by tools/gen_eval_golden.py), and closed_set_report against a brute-force restatement of the
reference notebook's cells 16-19 on a full score matrix."""
import os

import numpy as np
import pytest

from facerecognition_amd import evaluate as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evaluate_golden.npz")
CASES = ["rounded", "continuous"]
RTOL = 1e-12


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def close(a, b):
    return np.allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=RTOL, atol=0.0)


def inputs(gold, case):
    return gold[case + "_y_true"], gold[case + "_y_pred"], gold[case + "_scores"]


@pytest.mark.parametrize("case", CASES)
def test_compute_metrics_matches_reference(gold, case):
    y_true, y_pred, _ = inputs(gold, case)
    m = E.compute_metrics(y_true, y_pred)
    keys = [str(k) for k in gold[case + "_metric_keys"]]
    assert list(m.keys()) == keys and len(keys) == 10
    for k, want in zip(keys, gold[case + "_metric_values"]):
        if k in ("total_samples", "correct", "wrong"):
            assert m[k] == int(want) and isinstance(m[k], int), k
        else:
            assert close(m[k], want), (k, m[k], want)


@pytest.mark.parametrize("case", CASES)
def test_threshold_sweep_matches_reference(gold, case):
    y_true, y_pred, scores = inputs(gold, case)
    s = E.threshold_sweep(scores, y_true, y_pred)
    keys = [str(k) for k in gold[case + "_sweep_keys"]]
    want = gold[case + "_sweep_rows"]
    assert len(s["results"]) == len(want) == len(np.arange(0.3, 0.95, 0.05))
    for row, w in zip(s["results"], want):
        assert list(row.keys()) == keys
        for k, v in zip(keys, w):
            if k.startswith("num_"):
                assert row[k] == int(v), (k, row)
            elif k == "threshold":
                assert row[k] == v
            else:
                assert close(row[k], v), (k, row[k], v)
    best = gold[case + "_sweep_best"]
    assert s["best_f1_threshold"] == best[0] and s["best_accuracy_threshold"] == best[2]  # first maxima
    assert close(s["best_f1_score"], best[1]) and close(s["best_accuracy_score"], best[3])


@pytest.mark.parametrize("case", CASES)
def test_roc_analysis_matches_reference(gold, case):
    y_true, y_pred, scores = inputs(gold, case)
    r = E.roc_analysis((y_true == y_pred).astype(int), scores)
    assert sorted(r.keys()) == ["auc", "eer", "eer_threshold", "fpr", "thresholds", "tpr"]
    for k in ("fpr", "tpr", "thresholds"):
        assert len(r[k]) == len(gold[case + "_" + k]), k  # the same points dropped
    if case == "continuous":
        assert len(r["fpr"]) < len(np.unique(scores)) + 1  # collinear points really were dropped
    assert close(r["fpr"], gold[case + "_fpr"]) and close(r["tpr"], gold[case + "_tpr"])
    assert np.isinf(r["thresholds"][0])
    assert np.array_equal(r["thresholds"][1:], gold[case + "_thresholds"][1:])
    auc, eer, eer_thr = gold[case + "_auc_eer"]
    assert close(r["auc"], auc) and close(r["eer"], eer) and r["eer_threshold"] == eer_thr


@pytest.mark.parametrize("case", CASES)
def test_generate_report_matches_reference(gold, case, tmp_path):
    y_true, y_pred, scores = inputs(gold, case)
    m = E.compute_metrics(y_true, y_pred)
    roc = E.roc_analysis((y_true == y_pred).astype(int), scores)
    sweep = E.threshold_sweep(scores, y_true, y_pred)
    text = E.generate_report(m, roc, sweep, str(tmp_path / "out"))
    assert text == str(gold[case + "_report"])
    assert (tmp_path / "out" / "evaluation_report.md").read_text(encoding="utf-8") == text


def test_confusion_matrix_and_string_labels():
    y_true = np.array(["b", "a", "c", "a", "b"])
    y_pred = np.array(["b", "c", "c", "a", "Unknown"])
    cm = E.confusion_matrix(y_true, y_pred)  # labels: Unknown, a, b, c
    assert cm.dtype == np.int64 and cm.shape == (4, 4) and cm.sum() == 5
    assert cm[1, 1] == 1 and cm[1, 3] == 1 and cm[2, 2] == 1 and cm[2, 0] == 1 and cm[3, 3] == 1
    m = E.compute_metrics(y_true, y_pred)
    assert m["correct"] == 3 and m["wrong"] == 2 and m["accuracy"] == 0.6
    # macro over the 4 labels present, zero_division=0: precision Unknown 0, a 1, b 1, c 1/2
    assert close(m["precision_macro"], (0 + 1 + 1 + 0.5) / 4)
    assert close(m["recall_weighted"], 0.6)


def test_closed_set_report_matches_notebook_bruteforce():
    """Cells 16-19 restated on the full [200, 50] matrix.  The notebook's argsort leaves the order of
    equal scores open; the restatement fixes it to the match order (score descending, lower index
    first), which is also what its argmax does."""
    rng = np.random.default_rng(5)
    n, g = 200, 50
    sims = np.round(rng.uniform(-0.2, 0.6, (n, g)), 2).astype(np.float32)  # 81 levels: many ties
    labels = rng.integers(0, g, n)
    for i in range(0, n, 2):  # half the probes: a strong true score
        sims[i, labels[i]] = np.float32(0.55 + 0.05 * (i % 10))
    for i in range(0, n, 5):  # planted ties with the true score, below and above the true index
        sims[i, (labels[i] + 7) % g] = sims[i, labels[i]]
        sims[i, (labels[i] - 3) % g] = sims[i, labels[i]]

    # --- the notebook, on the matrix
    preds = np.argmax(sims, axis=1)
    top1 = (preds == labels).mean() * 100
    top5_preds = np.argsort(-sims, axis=1, kind="stable")[:, :5]
    top5 = np.mean([t in p for t, p in zip(labels, top5_preds)]) * 100
    y_bin = (labels == preds).astype(int)
    y_sc = np.array([sims[i, t] for i, t in enumerate(labels)])
    max_sims = sims.max(axis=1)
    thresholds = np.arange(0.0, 1.0, 0.05)
    accs, covs = [], []
    for t in thresholds:
        m = max_sims >= t
        covs.append(m.mean() * 100)
        accs.append(y_bin[m].mean() * 100 if m.sum() > 0 else 0)

    # --- the device outputs such a matrix stands for
    order = np.argsort(-sims, axis=1, kind="stable")
    rank = np.array([int(np.where(order[i] == labels[i])[0][0]) for i in range(n)])
    hist = np.zeros(400, np.int64)
    mask = np.ones_like(sims, dtype=bool)
    mask[np.arange(n), labels] = False
    bins = np.clip(np.floor((sims[mask].astype(np.float64) + 1.0) * 200.0).astype(int), 0, 399)
    np.add.at(hist, bins, 1)

    rep = E.closed_set_report(y_sc, rank, max_sims, hist=hist, hist_range=(-1.0, 1.0), max_rank=g)
    assert rep["top1_acc"] * 100 == top1 and rep["top5_acc"] * 100 == top5
    assert 0 < rep["top1_acc"] < rep["top5_acc"] < 1
    assert np.array_equal(rep["thresholds"], thresholds)
    assert np.array_equal(rep["accuracy"], np.array(accs, dtype=np.float64))
    assert np.array_equal(rep["coverage"], np.array(covs, dtype=np.float64))
    want_roc = E.roc_analysis(y_bin, y_sc)  # identical ROC inputs -> identical curve
    assert np.array_equal((rank == 0).astype(int), y_bin)
    for k in ("fpr", "tpr", "thresholds"):
        assert np.array_equal(rep["roc"][k], want_roc[k])
    assert rep["roc"]["auc"] == want_roc["auc"] and rep["roc"]["eer"] == want_roc["eer"]
    cmc = rep["cmc"]
    assert cmc[0] == rep["top1_acc"] and cmc[4] == rep["top5_acc"] and cmc[-1] == 1.0 and np.all(np.diff(cmc) >= 0)
    # false-accept rate at an edge = share of impostor scores in the bins from that edge up
    assert rep["impostor_pairs"] == n * (g - 1) and rep["far"][0] == 1.0 and rep["far"][-1] == 0.0
    for e in (200, 240, 300, 330):
        assert abs(rep["far_edges"][e] - (-1.0 + e / 200.0)) < 1e-12
        assert rep["far"][e] == np.mean(bins >= e)


def test_evaluate_recognition_engine_with_a_stub_engine(tmp_path):
    """One recognize_batch call; the reference's result keys, the confusion matrix as an integer array."""
    labels = ["ann", "bob", "cy", "ann", "bob", "cy", "ann", "bob"]
    preds = ["ann", "bob", "ann", "ann", "Unknown", "cy", "bob", "bob"]
    confs = [0.9, 0.8, 0.45, 0.7, 0.2, 0.65, 0.5, 0.85]

    class Engine:
        calls = 0

        def recognize_batch(self, imgs):
            Engine.calls += 1
            return [{"identity": p, "confidence": c} for p, c in zip(preds, confs)]

    out = E.evaluate_recognition_engine(Engine(), [f"img{i}.jpg" for i in range(8)], labels, str(tmp_path))
    assert Engine.calls == 1
    assert sorted(out) == ["confidences", "confusion_matrix", "metrics", "predictions", "roc", "threshold_sweep"]
    assert out["predictions"] == preds and out["confidences"] == confs
    assert out["metrics"]["correct"] == 5 and out["metrics"]["total_samples"] == 8
    cm = out["confusion_matrix"]  # labels: Unknown, ann, bob, cy
    assert cm.dtype == np.int64 and cm.shape == (4, 4) and int(np.trace(cm)) == 5 and cm[2, 0] == 1
    # the sweep treats 'Unknown' (not a test label) as unknown at every threshold
    row = out["threshold_sweep"]["results"][0]  # threshold 0.3: everything but the 0.2 prediction is known
    assert row["num_known"] == 7 and row["num_unknown"] == 1 and close(row["precision"], 5 / 7)
    assert (tmp_path / "evaluation_report.md").exists()
    import facerecognition_amd

    assert facerecognition_amd.evaluate_recognition_engine is E.evaluate_recognition_engine
    assert facerecognition_amd.closed_set_report is E.closed_set_report
