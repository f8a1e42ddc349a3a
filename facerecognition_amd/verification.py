"""All-pairs 1:1 verification on the device (libfrhip's fr_verify_pairs).

Drop-in for the reference's ``compute_verification_accuracy`` (models/arcface/train_arcface.py:114-210 and
models/facenet/train_facenet.py:64-160), the metric its ``validate()`` reports every epoch and its early stopping
watches.  The reference estimates it from 10 000 randomly drawn pairs, one ``np.dot`` per pair, unseeded; here EVERY
pair of the set is scored exactly in one Gram sweep on the GPU, no N x N matrix is stored and the result is bitwise
repeatable.  ``verification_report`` adds what a 1:1 protocol reads from the two score distributions: ROC, AUC, EER,
d', TAR at fixed FAR, leave-one-out rank-1 and the pairs most likely to be label noise.  The definitions (score,
normalisation, strict ``>``, histogram bins, tie rule) are in include/frhip.h "All-pairs verification".

There is no CPU or PyTorch fallback: the scores are computed on the GPU, float32.  At most 2^22 rows per call.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native as N

MAX_THRESHOLDS = 64  # FR_VERIFY_MAX_THRESHOLDS


def _check(embeddings):
    if not (isinstance(embeddings, torch.Tensor) and embeddings.is_cuda):
        raise RuntimeError("verification needs ROCm GPU tensors; there is deliberately no CPU fallback")
    if embeddings.dim() != 2:
        raise ValueError(f"verification: embeddings [N, D] expected, got {tuple(embeddings.shape)}")
    if embeddings.dtype != torch.float32:
        raise TypeError("verification: float32 embeddings expected (the scores are exact float32)")


def _call(e, y, thresholds, counts, totals, hist, nbins, lo, hi, row_score, row_idx, row_sum, normalize, ws_bytes=None):
    """fr_verify_pairs on caller-made buffers (None = NULL).  thresholds: host float32 array."""
    n_rows, dim = e.shape
    L = N.lib()
    if ws_bytes is None:
        ws_bytes = L.fr_verify_workspace(n_rows, dim)
        if ws_bytes == 0:
            N.check(-1, "fr_verify_workspace")
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=e.device)
    thr = np.ascontiguousarray(thresholds, dtype=np.float32)
    N.check(L.fr_verify_pairs(N.ptr(e), n_rows, dim, N.ptr(y), int(normalize), thr.ctypes.data if thr.size else None,
                              int(thr.size), N.ptr(counts), N.ptr(totals), N.ptr(hist), int(nbins), float(lo), float(hi),
                              N.ptr(row_score), N.ptr(row_idx), N.ptr(row_sum), N.ptr(ws), ws_bytes,
                              N.stream_ptr(e.device)), "fr_verify_pairs")


def verify_pairs(embeddings, labels, thresholds=(), hist_bins=0, hist_range=(-1, 1), normalize=True, rows=True, *,
                 hist=None, ws_bytes=None):
    """One exact pass over all pairs of ``embeddings`` [N, D] (GPU, float32) with ``labels`` [N] (any integers).

    Returns a dict of device tensors (counts are int64): ``totals`` [2] = genuine and impostor pairs (i < j);
    ``counts`` [T, 2] = of those, the pairs scoring strictly above each threshold; ``hist`` [2, hist_bins] (None when
    ``hist_bins`` is 0) over ``hist_range``; with ``rows``: ``row_score`` / ``row_idx`` [N, 3] = each row's best genuine
    mate, worst genuine mate and best impostor over all j != i (ties to the lowest j; -inf, +inf, -inf and -1 where
    there is none) and ``row_sum`` [N, 2] = the sums of its genuine and impostor scores.  ``normalize``: score the rows
    divided by (norm + 1e-8) as the reference does; False: the rows as given.  ``hist``: an int64 [2, hist_bins] tensor
    to add into instead of a new one; ``ws_bytes``: the workspace to use instead of the recommended one (neither the
    results nor their bits depend on it).  Stream-ordered; nothing is read back."""
    _check(embeddings)
    e = embeddings.detach().contiguous()
    n_rows = e.shape[0]
    dev = e.device
    y = torch.as_tensor(labels, device=dev).reshape(-1).to(torch.int32).contiguous()
    if y.numel() != n_rows:
        raise ValueError(f"verification: {n_rows} labels expected, got {y.numel()}")
    thr = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    hist_bins = int(hist_bins)
    if hist is not None:
        if not (hist.is_cuda and hist.dtype == torch.int64 and hist.is_contiguous() and hist_bins > 0
                and tuple(hist.shape) == (2, hist_bins)):
            raise ValueError("verification: hist must be a contiguous int64 GPU tensor [2, hist_bins]")
    elif hist_bins:
        hist = torch.zeros((2, hist_bins), dtype=torch.int64, device=dev)
    counts = torch.empty((thr.size, 2), dtype=torch.int64, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    row_score = torch.empty((n_rows, 3), dtype=torch.float32, device=dev) if rows else None
    row_idx = torch.empty((n_rows, 3), dtype=torch.int32, device=dev) if rows else None
    row_sum = torch.empty((n_rows, 2), dtype=torch.float32, device=dev) if rows else None
    lo, hi = hist_range
    _call(e, y, thr, counts if thr.size else None, totals, hist, hist_bins, lo, hi, row_score, row_idx, row_sum,
          bool(normalize), ws_bytes)
    return {"totals": totals, "counts": counts, "hist": hist, "row_score": row_score, "row_idx": row_idx,
            "row_sum": row_sum}


def _to_device(embeddings):
    """numpy arrays (what the reference's validate() passes) are uploaded; CPU tensors are refused like everywhere."""
    if isinstance(embeddings, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError("verification needs a ROCm GPU; there is deliberately no CPU fallback")
        return torch.from_numpy(np.ascontiguousarray(embeddings, dtype=np.float32)).cuda()
    _check(embeddings)
    return embeddings


def _host_labels(labels):
    if isinstance(labels, torch.Tensor):
        labels = labels.detach().cpu().numpy()
    return np.asarray(labels).reshape(-1)


SWEEP = np.arange(0.1, 0.9, 0.05)  # the reference's threshold grid


def compute_verification_accuracy(embeddings, labels, num_pairs=None, threshold=0.5):
    """The reference's verification accuracy over ALL pairs: ``(accuracy, best_threshold, metrics)`` with the
    reference's metrics keys (``accuracy``, ``threshold``, ``pos_sim_mean``, ``neg_sim_mean``, ``num_pos_pairs``,
    ``num_neg_pairs``) and its early returns (``(0.0, threshold, {})`` for fewer than two rows, ``{'error': ...}`` for
    fewer than two labels with two rows).  Rows whose label occurs once are dropped first, as the reference's
    ``valid_labels`` does; scores are cosine similarities with the reference's ``a / (|a| + 1e-8)``; a pair is accepted
    when its score is strictly above the threshold; thresholds are ``np.arange(0.1, 0.9, 0.05)`` (compared as
    float32) and the best is the first with the strictly highest accuracy.

    Departure from the reference: it samples ``num_pairs // 2`` genuine and as many impostor pairs; here every pair is
    used and ``accuracy`` is the balanced accuracy 0.5 (genuine accepted / genuine + impostor rejected / impostor),
    which is what its half-and-half sample estimates when classes have equal sizes (it draws labels, not pairs,
    uniformly).  ``num_pairs`` is accepted for the signature's sake and ignored.  The two means come from the
    per-row score sums, added in float64 on the host.  ``embeddings``: a GPU float32 tensor or a numpy array."""
    n = len(embeddings)
    if n < 2:
        return 0.0, threshold, {}
    lab = _host_labels(labels)
    _, inv, cnt = np.unique(lab, return_inverse=True, return_counts=True)
    if int(np.sum(cnt >= 2)) < 2:
        return 0.0, threshold, {"error": "Not enough valid labels"}
    keep = cnt[inv] >= 2
    e = _to_device(embeddings)
    if not keep.all():
        e = e[torch.from_numpy(np.flatnonzero(keep)).to(e.device)]
    r = verify_pairs(e, inv[keep].astype(np.int32), SWEEP.astype(np.float32))
    n_pos, n_neg = (int(v) for v in r["totals"].tolist())
    counts = r["counts"].cpu().numpy().astype(np.float64)
    acc = 0.5 * (counts[:, 0] / n_pos + (n_neg - counts[:, 1]) / n_neg)
    best_acc, best_thresh = 0, threshold
    for a, t in zip(acc, SWEEP):
        if a > best_acc:
            best_acc, best_thresh = a, t
    sums = r["row_sum"].double().sum(0).tolist()  # every pair is in two rows' sums
    accuracy = float(best_acc)
    metrics = {"accuracy": accuracy, "threshold": best_thresh, "pos_sim_mean": sums[0] / (2 * n_pos),
               "neg_sim_mean": sums[1] / (2 * n_neg), "num_pos_pairs": n_pos, "num_neg_pairs": n_neg}
    return accuracy, best_thresh, metrics


def roc_from_histograms(hist, hist_range=(-1.0, 1.0)):
    """ROC of a genuine / impostor histogram pair [2, nbins] at the nbins + 1 bin edges: ``edges``, ``tar`` and ``far``
    (the share of genuine / impostor pairs in or above the bin starting at each edge, 0 at the last edge: evaluate.py's
    ``closed_set_report`` far rule), trapezoidal ``auc``, and the equal-error point, the edge where |far - (1 - tar)| is
    least (first minimum, as ``roc_analysis``): ``eer`` = (far + 1 - tar) / 2 there, ``eer_threshold``, ``eer_bin``.
    ``dprime`` = (mean_g - mean_i) / sqrt((var_g + var_i) / 2) from the bin centres."""
    h = np.asarray(hist).astype(np.int64)
    nb = h.shape[1]
    lo, hi = hist_range
    edges = np.linspace(lo, hi, nb + 1)
    tot = h.sum(1).astype(np.float64)
    tail = np.concatenate([np.cumsum(h[:, ::-1], axis=1)[:, ::-1], np.zeros((2, 1), np.int64)], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        tar, far = tail[0] / tot[0], tail[1] / tot[1]
    x, yv = far[::-1], tar[::-1]  # ascending far
    auc = float(np.sum(np.diff(x) * (yv[1:] + yv[:-1]) / 2.0))
    k = int(np.argmin(np.abs(far - (1 - tar))))
    centre = (edges[:-1] + edges[1:]) / 2
    mean = (h * centre).sum(1) / tot
    var = (h * (centre[None, :] - mean[:, None]) ** 2).sum(1) / tot
    spread = np.sqrt((var[0] + var[1]) / 2)
    return {"edges": edges, "tar": tar, "far": far, "auc": auc, "eer": float((far[k] + 1 - tar[k]) / 2),
            "eer_threshold": float(edges[k]), "eer_bin": k,
            "dprime": float((mean[0] - mean[1]) / spread) if spread > 0 else float("inf")}


def far_candidates(imp_hist, n_imp, fars, hist_range, shift=0):
    """The thresholds of the refining call: for each requested FAR the allowed false accepts k = floor(far n_imp) and
    the bin b that holds the quantile (the lowest bin with at most k impostors in the bins above it, moved up by
    ``shift``), then P = 64 // len(fars) float32 thresholds lo + (b + m / P) w, m = 1 .. P, the last one bin b's upper
    edge.  Returns (k [F], thresholds [F, P])."""
    h = np.asarray(imp_hist).astype(np.int64)
    nb = h.size
    lo, hi = hist_range
    w = (hi - lo) / nb
    per = MAX_THRESHOLDS // len(fars)
    above = np.concatenate([np.cumsum(h[::-1])[::-1][1:], [0]])  # impostors in the bins above b
    ks, thr = [], []
    for f in fars:
        k = int(np.floor(float(f) * n_imp + 1e-9))
        b = int(np.argmax(above <= k)) + shift
        ks.append(k)
        thr.append(lo + (b + np.arange(1, per + 1) / per) * w)
    return np.array(ks, np.int64), np.array(thr, np.float64).astype(np.float32)


class VerificationReport(dict):
    """``verification_report``'s result: a dict, plus the two label-noise lists at any length."""

    def hardest_impostors(self, k=10):
        """The k impostor pairs of highest score among every row's best impostor: ``(row, other row, score)``, each
        unordered pair once, highest first (then lower row).  Rows of one person under two labels come first."""
        return _pairs(self["row_score"][:, 2], self["row_idx"][:, 2], k, descending=True)

    def hardest_genuines(self, k=10):
        """The k genuine pairs of lowest score among every row's worst mate, lowest first: a row carrying another
        person's label comes first."""
        return _pairs(self["row_score"][:, 1], self["row_idx"][:, 1], k, descending=False)


def _pairs(score, other, k, descending):
    has = np.flatnonzero(other >= 0)
    key = -score[has] if descending else score[has]
    out, seen = [], set()
    for r in has[np.argsort(key, kind="mergesort")]:
        pair = (min(int(r), int(other[r])), max(int(r), int(other[r])))
        if pair in seen:
            continue
        seen.add(pair)
        out.append((int(r), int(other[r]), float(score[r])))
        if len(out) >= k:
            break
    return out


def verification_report(embeddings, labels, fars=(1e-1, 1e-2, 1e-3, 1e-4), hist_bins=2048):
    """A 1:1 verification report over ALL pairs of a labelled set (cosine scores, the reference's normalisation).

    From the genuine and impostor histograms (``hist_bins`` bins over [-1, 1]): ``roc`` (``roc_from_histograms``: tar
    and far at every bin edge), ``auc``, ``eer``, ``eer_threshold``, ``dprime``.  ``tar_at_far``: one dict per
    requested FAR with the EXACT counts at a stated threshold: a second device pass counts both classes strictly above
    64 // len(fars) thresholds that subdivide the histogram bin holding the FAR quantile (``far_candidates``); reported
    is the lowest of them with at most floor(far x impostor pairs) false accepts: ``threshold``, ``false_accepts``,
    ``far`` (false accepts / impostor pairs), ``tar`` (genuine pairs above it / genuine pairs).  The counts are exact;
    the threshold is within one sub-step, (2 / hist_bins) / (64 // len(fars)) (6.1e-5 for the defaults), of the lowest
    threshold that meets the FAR.  A FAR below 1 / impostor pairs allows no false accept: the entry is the TAR at zero
    false accepts and its ``note`` says so.  ``rank1``: leave-one-out rank-1 accuracy over the ``rank1_rows`` rows that
    have a mate: a row is correct when its best genuine mate beats its best impostor (at an equal score, when the mate
    has the lower index).  ``hardest_impostors(k)`` / ``hardest_genuines(k)`` list (row, other row, score) for hunting
    label noise; the first ten of each are also stored under those keys.  ``embeddings``: a GPU float32 tensor or a
    numpy array; every row is used (a singleton only has impostors)."""
    fars = [float(f) for f in fars]
    if not 1 <= len(fars) <= MAX_THRESHOLDS:
        raise ValueError(f"verification_report: 1 to {MAX_THRESHOLDS} FAR values expected")
    if any(not (0 < f < 1) for f in fars):
        raise ValueError("verification_report: every FAR must lie in (0, 1)")
    e = _to_device(embeddings)
    _, inv = np.unique(_host_labels(labels), return_inverse=True)
    y = torch.from_numpy(inv.astype(np.int32)).to(e.device)
    rng = (-1.0, 1.0)
    r = verify_pairs(e, y, (), hist_bins, rng)
    hist = r["hist"].cpu().numpy()
    n_gen, n_imp = (int(v) for v in r["totals"].tolist())
    if n_gen == 0 or n_imp == 0:
        raise ValueError("verification_report: the set needs at least one genuine and one impostor pair")
    score, idx = r["row_score"].cpu().numpy(), r["row_idx"].cpu().numpy()
    rep = VerificationReport(genuine_pairs=n_gen, impostor_pairs=n_imp, hist=hist, hist_range=rng, row_score=score,
                             row_idx=idx)
    roc = roc_from_histograms(hist, rng)
    rep.update(roc=roc, auc=roc["auc"], eer=roc["eer"], eer_threshold=roc["eer_threshold"], dprime=roc["dprime"])

    tar_at_far = []
    for shift in range(4):  # (a bin further up only if float32 edge rounding left no candidate within the bin)
        ks, thr = far_candidates(hist[1], n_imp, fars, rng, shift)
        c = verify_pairs(e, y, thr.reshape(-1), rows=False)["counts"].cpu().numpy().reshape(len(fars), -1, 2)
        if all((c[f, :, 1] <= ks[f]).any() for f in range(len(fars))):
            break
    else:
        raise RuntimeError("verification_report: no threshold met a requested FAR")
    for f, far in enumerate(fars):
        m = int(np.argmax(c[f, :, 1] <= ks[f]))
        entry = {"far_target": far, "threshold": float(thr[f, m]), "false_accepts": int(c[f, m, 1]),
                 "far": int(c[f, m, 1]) / n_imp, "tar": int(c[f, m, 0]) / n_gen, "note": ""}
        if ks[f] == 0:
            entry["note"] = "FAR below 1 / impostor pairs: the TAR at zero false accepts"
        tar_at_far.append(entry)
    rep["tar_at_far"] = tar_at_far

    mate = idx[:, 0] >= 0
    win = (idx[:, 2] < 0) | (score[:, 0] > score[:, 2]) | ((score[:, 0] == score[:, 2]) & (idx[:, 0] < idx[:, 2]))
    rep.update(rank1=float(np.mean(win[mate])) if mate.any() else 0.0, rank1_rows=int(mate.sum()),
               pos_sim_mean=float(r["row_sum"][:, 0].double().sum().item()) / (2 * n_gen),
               neg_sim_mean=float(r["row_sum"][:, 1].double().sum().item()) / (2 * n_imp))
    rep["hardest_impostors"] = rep.hardest_impostors(10)
    rep["hardest_genuines"] = rep.hardest_genuines(10)
    return rep
