"""Evaluation: metrics, threshold sweep, ROC / AUC / EER, report, closed-set gallery evaluation.

Drop-in for the reference's ``inference/evaluate.py`` (``compute_metrics``, ``threshold_sweep``, the ROC
analysis inside ``plot_roc_curve``, ``evaluate_recognition_engine``, ``generate_report``: names, arguments
and result keys kept) and for cells 15-19 of its ``evaluate_arcface_kaggle.ipynb`` (top-1 / top-5, ROC of
the true-class score, accuracy against coverage).  numpy only: the sklearn calls the reference makes
(``precision_score`` ... with ``zero_division=0``, ``roc_curve`` with its defaults, ``auc``,
``confusion_matrix``) are restated here, and plots are left out.

The closed-set part needs no probes x gallery score matrix: ``DeviceGallery.evaluate`` (fr_match_eval)
returns per probe the score of its true row, the rank of that row and the top-k, plus a histogram of
all impostor scores; ``closed_set_report`` derives everything the notebook reads from its 760 MB matrix
(``argmax``, ``argsort[:, -5:]``, ``sims[i, true_idx]``, ``max(axis=1)``) from those.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np


def _prf(y_true: np.ndarray, y_pred: np.ndarray):
    """Per-label precision / recall / F1 / support over the sorted union of the labels present
    (precision_recall_fscore_support with zero_division=0)."""
    labels = np.unique(np.concatenate([y_true, y_pred]))
    t = np.searchsorted(labels, y_true)
    p = np.searchsorted(labels, y_pred)
    n = len(labels)
    tp = np.bincount(t[t == p], minlength=n).astype(np.float64)
    pred = np.bincount(p, minlength=n).astype(np.float64)
    true = np.bincount(t, minlength=n).astype(np.float64)

    def div(a, b):
        out = np.zeros_like(a)
        np.divide(a, b, out=out, where=b != 0)
        return out

    return div(tp, pred), div(tp, true), div(2 * tp, true + pred), true


def _averages(x: np.ndarray, support: np.ndarray) -> Tuple[float, float]:
    weighted = float(np.sum(x * support) / np.sum(support)) if np.sum(support) > 0 else 0.0
    return weighted, float(np.mean(x)) if len(x) else 0.0


def compute_metrics(y_true: np.ndarray, y_pred: np.ndarray, labels: List[str] = None) -> Dict:
    """Accuracy, weighted and macro precision / recall / F1, and the counts (``labels`` is accepted and
    unused, as in the reference)."""
    y_true = np.asarray(y_true)
    y_pred = np.asarray(y_pred)
    prec, rec, f1, support = _prf(y_true, y_pred)
    pw, pm = _averages(prec, support)
    rw, rm = _averages(rec, support)
    fw, fm = _averages(f1, support)
    return {
        "accuracy": float(np.mean(y_true == y_pred)),
        "precision_weighted": pw,
        "recall_weighted": rw,
        "f1_weighted": fw,
        "precision_macro": pm,
        "recall_macro": rm,
        "f1_macro": fm,
        "total_samples": len(y_true),
        "correct": int(np.sum(y_true == y_pred)),
        "wrong": int(np.sum(y_true != y_pred)),
    }


def threshold_sweep(similarities: np.ndarray, y_true: np.ndarray, y_pred_identities: np.ndarray,
                    thresholds: List[float] = None) -> Dict:
    """Accuracy / precision / recall / F1 / known ratio when predictions scoring below each threshold
    become unknown (-1); the best-F1 and best-accuracy thresholds are the first maxima."""
    if thresholds is None:
        thresholds = np.arange(0.3, 0.95, 0.05)
    similarities = np.asarray(similarities)
    y_true = np.asarray(y_true)
    y_pred_identities = np.asarray(y_pred_identities)
    n = len(y_true)
    results = []
    for thresh in thresholds:
        y_pred = np.where(similarities >= thresh, y_pred_identities, -1)
        known = y_pred != -1
        num_known = int(np.sum(known))
        accuracy = precision = recall = f1 = 0.0
        if num_known:
            correct = np.sum((y_pred == y_true) & known)
            accuracy = recall = correct / n if n > 0 else 0
            precision = correct / num_known
            f1 = 2 * precision * recall / (precision + recall) if (precision + recall) > 0 else 0
        results.append({
            "threshold": float(thresh),
            "accuracy": float(accuracy),
            "precision": float(precision),
            "recall": float(recall),
            "f1": float(f1),
            "known_ratio": float(num_known / n if n > 0 else 0),
            "num_known": num_known,
            "num_unknown": int(np.sum(~known)),
        })
    best_f1 = results[int(np.argmax([r["f1"] for r in results]))]
    best_acc = results[int(np.argmax([r["accuracy"] for r in results]))]
    return {
        "results": results,
        "best_f1_threshold": best_f1["threshold"],
        "best_f1_score": best_f1["f1"],
        "best_accuracy_threshold": best_acc["threshold"],
        "best_accuracy_score": best_acc["accuracy"],
    }


def _roc_curve(y_true: np.ndarray, y_scores: np.ndarray):
    """sklearn.metrics.roc_curve with its defaults (positive label 1, drop_intermediate=True): one
    point per distinct score in descending order, points collinear with both neighbours dropped, a
    leading (0, 0) at threshold inf."""
    pos = np.asarray(y_true) == 1
    score = np.asarray(y_scores, dtype=np.float64)
    order = np.argsort(score, kind="mergesort")[::-1]
    score = score[order]
    pos = pos[order]
    idx = np.r_[np.where(np.diff(score))[0], pos.size - 1]
    tps = np.cumsum(pos, dtype=np.float64)[idx]
    fps = 1 + idx - tps
    thr = score[idx]
    if len(fps) > 2:
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        fps, tps, thr = fps[keep], tps[keep], thr[keep]
    tps = np.r_[0, tps]
    fps = np.r_[0, fps]
    thr = np.r_[np.inf, thr]
    with np.errstate(divide="ignore", invalid="ignore"):
        fpr = fps / fps[-1] if fps[-1] > 0 else np.full(fps.shape, np.nan)
        tpr = tps / tps[-1] if tps[-1] > 0 else np.full(tps.shape, np.nan)
    return fpr, tpr, thr


def roc_analysis(y_true: np.ndarray, y_scores: np.ndarray) -> Dict:
    """ROC of binary labels (1 = correct prediction) against scores: fpr, tpr, thresholds (the first is
    inf), trapezoidal AUC, and the equal-error point, the curve point where |fpr - (1 - tpr)| is least
    (first minimum).  The dict the reference's ``plot_roc_curve`` returns, without the plot."""
    fpr, tpr, thresholds = _roc_curve(y_true, y_scores)
    roc_auc = float(np.sum(np.diff(fpr) * (tpr[1:] + tpr[:-1]) / 2.0))
    eer_idx = int(np.argmin(np.abs(fpr - (1 - tpr))))
    return {"fpr": fpr, "tpr": tpr, "thresholds": thresholds, "auc": roc_auc, "eer": fpr[eer_idx],
            "eer_threshold": thresholds[eer_idx]}


def confusion_matrix(y_true: np.ndarray, y_pred: np.ndarray) -> np.ndarray:
    """cm[i, j] = samples of true label i predicted as j, over the sorted union of the labels (int64)."""
    y_true = np.asarray(y_true)
    y_pred = np.asarray(y_pred)
    labels = np.unique(np.concatenate([y_true, y_pred]))
    n = len(labels)
    flat = np.searchsorted(labels, y_true) * n + np.searchsorted(labels, y_pred)
    return np.bincount(flat, minlength=n * n).reshape(n, n).astype(np.int64)


def _table(head: Sequence[str], rule: Sequence[str], rows: Sequence[Sequence[str]]) -> str:
    lines = ["| " + " | ".join(head) + " |", "|" + "|".join(rule) + "|"]
    lines += ["| " + " | ".join(r) + " |" for r in rows]
    return "\n".join(lines) + "\n"


def generate_report(metrics: Dict, roc_results: Dict, sweep_results: Dict, output_dir: str) -> str:
    """Markdown report (summary metrics, ROC analysis, threshold recommendation), also written to
    ``output_dir/evaluation_report.md``.  The reference's report up to its list of plot files, which
    are not produced here."""
    m, r, s = metrics, roc_results, sweep_results
    two = ("Metric", "Value"), ("-" * 8, "-" * 7)
    report = "# Evaluation Report\n\n## Summary Metrics\n\n" + _table(*two, [
        ("Accuracy", f"{m['accuracy']:.4f}"),
        ("Precision (weighted)", f"{m['precision_weighted']:.4f}"),
        ("Recall (weighted)", f"{m['recall_weighted']:.4f}"),
        ("F1 Score (weighted)", f"{m['f1_weighted']:.4f}"),
        ("Total Samples", f"{m['total_samples']}"),
        ("Correct", f"{m['correct']}"),
        ("Wrong", f"{m['wrong']}"),
    ]) + "\n## ROC Analysis\n\n" + _table(*two, [
        ("AUC", f"{r['auc']:.4f}"),
        ("EER", f"{r['eer']:.4f}"),
        ("EER Threshold", f"{r['eer_threshold']:.4f}"),
    ]) + "\n## Threshold Tuning\n\n" + _table(("Recommendation", "Threshold", "Score"), ("-" * 16, "-" * 11, "-" * 7), [
        ("Best F1", f"{s['best_f1_threshold']:.2f}", f"{s['best_f1_score']:.4f}"),
        ("Best Accuracy", f"{s['best_accuracy_threshold']:.2f}", f"{s['best_accuracy_score']:.4f}"),
    ])
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, "evaluation_report.md")
    with open(path, "w", encoding="utf-8") as f:
        f.write(report)
    print(f"Saved report: {path}")
    return report


def evaluate_recognition_engine(engine, test_images: List[str], test_labels: List[str],
                                output_dir: str = "results/evaluation") -> Dict:
    """Evaluate a RecognitionEngine on labelled images: one ``recognize_batch`` call (the reference loops
    ``recognize`` per image), then metrics, ROC of (prediction correct, confidence), the confusion
    matrix (an integer array, not a plot), the threshold sweep and the report.  Labels are numbered in
    sorted order for the sweep (the reference numbers them in set order; the sweep only asks whether
    two numbers are equal, and predictions outside the test labels count as unknown either way)."""
    os.makedirs(output_dir, exist_ok=True)
    print(f"Evaluating {len(test_images)} images...")
    results = engine.recognize_batch(list(test_images))
    predictions = [r["identity"] for r in results]
    confidences = [r["confidence"] for r in results]

    y_true = np.array(test_labels)
    y_pred = np.array(predictions)
    y_scores = np.array(confidences)
    unique_labels = sorted(set(test_labels))
    label_to_id = {label: i for i, label in enumerate(unique_labels)}
    y_true_ids = np.array([label_to_id.get(l, -1) for l in test_labels])
    y_pred_ids = np.array([label_to_id.get(p, -1) for p in predictions])

    metrics = compute_metrics(y_true, y_pred, unique_labels)
    roc_results = roc_analysis((y_true == y_pred).astype(int), y_scores)
    cm = confusion_matrix(y_true, y_pred)
    sweep_results = threshold_sweep(y_scores, y_true_ids, y_pred_ids)
    generate_report(metrics, roc_results, sweep_results, output_dir)
    return {"metrics": metrics, "roc": roc_results, "threshold_sweep": sweep_results, "confusion_matrix": cm,
            "predictions": predictions, "confidences": confidences}


def closed_set_report(true_score: np.ndarray, true_rank: np.ndarray, top1_score: np.ndarray,
                      hist: Optional[np.ndarray] = None, hist_range: Optional[Tuple[float, float]] = None,
                      max_rank: int = 20) -> Dict:
    """Notebook cells 16-19 from the device outputs of ``DeviceGallery.evaluate``.

    ``true_rank`` is the 0-based position of a probe's true row in the match order (score descending,
    lower index first on ties: ``np.argmax``'s rule), ``true_score`` its score (``sims[i, true_idx]``),
    ``top1_score`` the best score (``sims.max(axis=1)``).  Returns

    * ``top1_acc`` = mean(rank == 0) and ``top5_acc`` = mean(rank < 5), as fractions;
    * ``cmc``: cmc[r] = fraction of probes with rank <= r, r < ``max_rank``;
    * ``roc``: ``roc_analysis`` of (rank == 0, true_score);
    * ``thresholds`` = np.arange(0, 1, 0.05) with ``accuracy`` (top-1 accuracy among the probes whose
      best score reaches the threshold, 0 where none does) and ``coverage`` (their share), in percent
      as the notebook plots them;
    * with a histogram of impostor scores over ``hist_range``: ``far_edges`` (the nbins + 1 bin edges)
      and ``far`` (the share of impostor scores in or above the bin starting at each edge: the reverse
      cumulative sum over the total, 0 at the last edge), the false-accept rate against threshold.

    All probes are used: the notebook draws an unseeded 5000-probe subsample for its ROC, which is not
    reproduced.  Probes whose true row is outside the gallery (rank -1) count as misses.
    """
    true_score = np.asarray(true_score)
    rank = np.asarray(true_rank).astype(np.int64)
    top1_score = np.asarray(top1_score)
    found = rank >= 0
    hit1 = found & (rank == 0)
    out = {
        "total": int(rank.size),
        "top1_acc": float(np.mean(hit1)),
        "top5_acc": float(np.mean(found & (rank < 5))),
        "cmc": np.array([np.mean(found & (rank <= r)) for r in range(max_rank)], dtype=np.float64),
        "roc": roc_analysis(hit1.astype(int), true_score),
    }
    thresholds = np.arange(0.0, 1.0, 0.05)
    is_correct = hit1.astype(int)
    accs, covs = [], []
    for t in thresholds:
        m = top1_score >= t
        covs.append(m.mean() * 100)
        accs.append(is_correct[m].mean() * 100 if m.sum() > 0 else 0)
    out.update(thresholds=thresholds, accuracy=np.array(accs, dtype=np.float64),
               coverage=np.array(covs, dtype=np.float64))
    if hist is not None:
        h = np.asarray(hist).astype(np.int64)
        lo, hi = hist_range if hist_range is not None else (-1.0, 1.0)
        total = int(h.sum())
        tail = np.r_[np.cumsum(h[::-1])[::-1], 0]
        out.update(far_edges=np.linspace(lo, hi, h.size + 1),
                   far=tail / total if total else np.zeros(h.size + 1), impostor_pairs=total)
    return out


def evaluate_closed_set(gallery, probes, true_idx, hist_bins: int = 512,
                        hist_range: Tuple[float, float] = (-1.0, 1.0), max_rank: int = 20, k: int = 5) -> Dict:
    """``gallery.evaluate(probes, true_idx)`` (a DeviceGallery; true_idx = each probe's true gallery
    row) followed by ``closed_set_report``.  The device outputs are returned under ``device``."""
    r = gallery.evaluate(probes, true_idx, k=max(int(k), 1), hist_bins=hist_bins, hist_range=hist_range)
    rep = closed_set_report(r["true_score"], r["true_rank"], r["scores"][:, 0], r["hist"],
                            hist_range if hist_bins else None, max_rank)
    rep["device"] = r
    return rep
