#!/usr/bin/env python3
"""Generate tests/golden/evaluate_golden.npz (run in the survey container, where /root/reference exists;
the GPU box never runs this).

It loads the reference's OWN inference/evaluate.py by file path -- with an empty ``seaborn`` module
stubbed in (not installed here; only the confusion-matrix plot uses it) and the Agg matplotlib backend --
feeds it seeded label and score arrays and records what it returns: compute_metrics, every
threshold_sweep row and the chosen thresholds, the ROC arrays / AUC / EER of plot_roc_curve, and the
text of generate_report up to its list of plot files.  Two cases: scores rounded to 2 decimals (ties,
and scores exactly at a sweep threshold) and continuous scores (roc_curve drops collinear points).

Output: data only (inputs and expected outputs), plus the sklearn version that produced it.
"""
import importlib.util
import os
import sys
import tempfile
import types

import numpy as np

os.environ.setdefault("MPLBACKEND", "Agg")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"


def load_reference():
    sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))
    spec = importlib.util.spec_from_file_location("ref_evaluate", os.path.join(REF, "inference", "evaluate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_case(seed: int, n: int, n_classes: int, rounded: bool):
    """Labels with ~25 % errors (some predictions of a class that never occurs as a true label, some
    'unknown' -1), scores higher for correct predictions."""
    rng = np.random.default_rng(seed)
    y_true = rng.integers(0, n_classes, n)
    y_pred = y_true.copy()
    wrong = rng.choice(n, size=n // 4, replace=False)
    y_pred[wrong] = rng.integers(0, n_classes + 2, wrong.size)  # n_classes, n_classes + 1: predicted only
    y_pred[rng.choice(n, size=n // 20, replace=False)] = -1
    scores = rng.uniform(0.2, 0.9, n) + 0.15 * (y_pred == y_true)
    scores = np.clip(scores, 0.0, 1.0)
    if rounded:
        scores = np.round(scores, 2)
    return y_true.astype(np.int64), y_pred.astype(np.int64), scores.astype(np.float64)


def main():
    import sklearn

    ref = load_reference()
    out = {"sklearn_version": np.array(sklearn.__version__), "cases": np.array(["rounded", "continuous"])}
    for name, (seed, n, ncls, rounded) in {"rounded": (11, 400, 12, True), "continuous": (12, 600, 20, False)}.items():
        y_true, y_pred, scores = make_case(seed, n, ncls, rounded)
        m = ref.compute_metrics(y_true, y_pred)
        sweep = ref.threshold_sweep(scores, y_true, y_pred)
        roc = ref.plot_roc_curve((y_true == y_pred).astype(int), scores, output_path=None, show=False)
        with tempfile.TemporaryDirectory() as d:
            report = ref.generate_report(m, roc, sweep, d)
        cut = report.index("## Visualizations")
        p = name + "_"
        out[p + "y_true"], out[p + "y_pred"], out[p + "scores"] = y_true, y_pred, scores
        out[p + "metric_keys"] = np.array(list(m.keys()))
        out[p + "metric_values"] = np.array([float(v) for v in m.values()], dtype=np.float64)
        rows = sweep["results"]
        out[p + "sweep_keys"] = np.array(list(rows[0].keys()))
        out[p + "sweep_rows"] = np.array([[float(r[k]) for k in rows[0]] for r in rows], dtype=np.float64)
        out[p + "sweep_best"] = np.array([sweep["best_f1_threshold"], sweep["best_f1_score"],
                                          sweep["best_accuracy_threshold"], sweep["best_accuracy_score"]], np.float64)
        for k in ("fpr", "tpr", "thresholds"):
            out[p + k] = np.asarray(roc[k], dtype=np.float64)
        out[p + "auc_eer"] = np.array([roc["auc"], roc["eer"], roc["eer_threshold"]], dtype=np.float64)
        out[p + "report"] = np.array(report[:cut].rstrip("\n") + "\n")
        print(f"{name}: n={n} roc points={len(roc['fpr'])} auc={roc['auc']:.4f} eer={roc['eer']:.4f} "
              f"best_f1_thr={sweep['best_f1_threshold']:.2f}")
    path = os.path.join(ROOT, "tests", "golden", "evaluate_golden.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
