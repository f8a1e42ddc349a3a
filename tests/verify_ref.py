"""Float64 numpy restatement of the all-pairs verification (include/frhip.h "All-pairs verification") and of what
facerecognition_amd.verification derives from it, plus our own restatement of the reference's sampled
``compute_verification_accuracy`` with the random generator passed in.  The checker of tests/test_gpu_verify.py; itself
checked on hand-computed cases by tests/test_verify_ref.py.  No GPU, no torch.

``delta(D)`` = (D + 8) u, u = 2^-24, bounds the device's float32 score against the float64 one in units of the
cosine: D u |a| |b| is the first-order worst case of a D-term float32 dot product (one rounding per product and per
sum) and |a| |b| r_a r_b <= 1; the 8 u cover the normalisation's own roundings (per row a square root, the + 1e-8 and
a division, then two products).  The rounding inside the two square sums (positive terms: about D u / 4 relative each
after the square root, worst case) is left to the slack of the dot product's worst case, which sums of mixed signs
never approach.  Derived, not measured.
"""
import numpy as np

U = 2.0 ** -24
SWEEP = np.arange(0.1, 0.9, 0.05)


def delta(D):
    return (D + 8) * U


def grid_case(N, D, seed):
    """Rows whose entries are multiples of 1/8 in [-1, 1]: every dot product is a multiple of 1/64 of magnitude at most
    D, exact in float32 in any summation order.  A quarter of the rows are copies of four others, spread over the
    tiles and the labels, so that equal scores, also among a row's best and worst, come in quantity.  Labels: one
    singleton (7), one class of two (3), one large class (0) and the rest over four more."""
    rng = np.random.default_rng(seed)
    E = (rng.integers(-8, 9, size=(N, D)) / 8.0).astype(np.float32)
    order = rng.permutation(N)
    for k, dst in enumerate(order[4:4 + N // 4]):
        E[dst] = E[order[k % 4]]
    labels = np.zeros(N, np.int32)
    if N > 8:
        labels[:] = rng.integers(10, 14, size=N)
        labels[rng.permutation(N)[: N // 3]] = 0
        labels[N // 2] = 7
        labels[[1, N - 2]] = 3
    return E, labels


def float_case(N, D, seed, classes=12):
    """Gaussian clusters, rows NOT of unit length (norms spread over about [0.8, 4])."""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, classes, size=N).astype(np.int32)
    centres = rng.standard_normal((classes, D))
    E = centres[labels] + 1.5 * rng.standard_normal((N, D))
    E *= rng.uniform(0.5, 2.0, size=(N, 1)) / np.sqrt(D)
    return E.astype(np.float32), labels


def scores(E, normalize):
    """s_ij in float64: the Gram matrix, with normalize scaled by r_i r_j, r = 1 / (|e| + 1e-8)."""
    E = np.asarray(E, np.float64)
    S = E @ E.T
    if normalize:
        r = 1.0 / (np.sqrt((E * E).sum(1)) + 1e-8)
        S = (S * r[:, None]) * r[None, :]
    return S


def bins(s, nbins, lo, hi):
    """fr_match_eval's bin rule with the float32 constants the ABI uses: inv_w = f32(nbins) / f32(hi - lo)."""
    lo32, hi32 = np.float32(lo), np.float32(hi)
    inv_w = np.float64(np.float32(nbins) / np.float32(hi32 - lo32))
    return np.clip(np.floor((np.asarray(s, np.float64) - np.float64(lo32)) * inv_w), 0, nbins - 1).astype(np.int64)


def all_pairs(S, labels, thresholds=(), nbins=0, lo=-1.0, hi=1.0):
    """Everything fr_verify_pairs returns, from a score matrix S [N, N]: dict of totals [2], counts [T, 2],
    hist [2, nbins] (None without bins), row_score / row_idx [N, 3], row_sum [N, 2]; also runner_up [N, 3], the score
    of the best candidate other than the chosen one (nan where there is none)."""
    S = np.asarray(S, np.float64)
    labels = np.asarray(labels)
    n = len(labels)
    gen = labels[:, None] == labels[None, :]
    off = ~np.eye(n, dtype=bool)
    up = np.triu(np.ones((n, n), bool), 1)
    out = {"totals": np.array([(gen & up).sum(), (~gen & up).sum()], np.int64)}
    thr = np.asarray(thresholds, np.float32).astype(np.float64)
    out["counts"] = np.array([[(gen & up & (S > t)).sum(), (~gen & up & (S > t)).sum()] for t in thr],
                             np.int64).reshape(len(thr), 2)
    out["hist"] = None
    if nbins:
        b = bins(S, nbins, lo, hi)
        out["hist"] = np.stack([np.bincount(b[gen & up], minlength=nbins), np.bincount(b[~gen & up], minlength=nbins)])
    score = np.empty((n, 3))
    idx = np.empty((n, 3), np.int32)
    runner = np.full((n, 3), np.nan)
    for slot, (mask, sign) in enumerate(((gen & off, 1.0), (gen & off, -1.0), (~gen & off, 1.0))):
        key = np.where(mask, sign * S, -np.inf)
        j = np.argmax(key, axis=1)  # the first maximum: ties to the lowest j
        has = mask.any(1)
        idx[:, slot] = np.where(has, j, -1)
        score[:, slot] = np.where(has, S[np.arange(n), j], -sign * np.inf)
        key[np.arange(n), j] = -np.inf
        second = key.max(1)
        runner[:, slot] = np.where(np.isfinite(second), sign * second, np.nan)
    out.update(row_score=score, row_idx=idx, runner_up=runner,
               row_sum=np.stack([np.where(gen & off, S, 0.0).sum(1), np.where(~gen & off, S, 0.0).sum(1)], axis=1))
    return out


def near_fraction(S, labels, thresholds, nbins, lo, hi, d):
    """The share of pairs i < j whose float64 score lies within d of a threshold or of a histogram edge."""
    S = np.asarray(S, np.float64)
    s = S[np.triu_indices(len(labels), 1)]
    near = np.zeros(s.shape, bool)
    for t in np.asarray(thresholds, np.float32).astype(np.float64):
        near |= np.abs(s - t) <= d
    if nbins:
        near |= bins(s - d, nbins, lo, hi) != bins(s + d, nbins, lo, hi)
    return float(near.mean())


def balanced_accuracy(counts, totals):
    c = np.asarray(counts, np.float64)
    g, i = (float(v) for v in totals)
    return 0.5 * (c[:, 0] / g + (i - c[:, 1]) / i)


def first_best(acc, thresholds, threshold=0.5):
    """The reference's loop: the first threshold with the strictly highest accuracy (its default where none is > 0)."""
    best_acc, best = 0, threshold
    for a, t in zip(acc, thresholds):
        if a > best_acc:
            best_acc, best = a, t
    return float(best_acc), best


def verification_accuracy_all_pairs(embeddings, labels, threshold=0.5):
    """facerecognition_amd.verification.compute_verification_accuracy in float64 on the host."""
    n = len(embeddings)
    if n < 2:
        return 0.0, threshold, {}
    labels = np.asarray(labels)
    _, inv, cnt = np.unique(labels, return_inverse=True, return_counts=True)
    if int(np.sum(cnt >= 2)) < 2:
        return 0.0, threshold, {"error": "Not enough valid labels"}
    keep = cnt[inv] >= 2
    S = scores(np.asarray(embeddings)[keep], True)
    r = all_pairs(S, inv[keep], SWEEP.astype(np.float32))
    acc, best = first_best(balanced_accuracy(r["counts"], r["totals"]), SWEEP, threshold)
    g, i = (int(v) for v in r["totals"])
    return acc, best, {"accuracy": acc, "threshold": best, "pos_sim_mean": r["row_sum"][:, 0].sum() / (2 * g),
                       "neg_sim_mean": r["row_sum"][:, 1].sum() / (2 * i), "num_pos_pairs": g, "num_neg_pairs": i}


def verification_accuracy_sampled(embeddings, labels, rng, num_pairs=10000, threshold=0.5):
    """Our restatement of the reference's sampled function.  rng: anything with numpy's legacy ``choice`` and
    ``shuffle`` (``np.random.RandomState(seed)`` draws what the reference draws after ``np.random.seed(seed)``):
    num_pairs // 2 times a label among those with two rows, then two of its rows without replacement; num_pairs // 2
    times two distinct such labels, then a row of each; the pairs shuffled; cosine of a / (|a| + 1e-8); accuracy of
    ``similarity > t`` over np.arange(0.1, 0.9, 0.05), the first strictly best."""
    embeddings = np.asarray(embeddings)
    labels = np.asarray(labels)
    n = len(embeddings)
    if n < 2:
        return 0.0, threshold, {}
    unique_labels = np.unique(labels)
    rows_of = {l: np.where(labels == l)[0] for l in unique_labels}
    valid = [l for l in unique_labels if len(rows_of[l]) >= 2]
    if len(valid) < 2:
        return 0.0, threshold, {"error": "Not enough valid labels"}
    pos, neg = [], []
    for _ in range(num_pairs // 2):
        rows = rows_of[rng.choice(valid)]
        i, j = rng.choice(rows, 2, replace=False)
        pos.append((i, j, 1))
    for _ in range(num_pairs // 2):
        l1, l2 = rng.choice(valid, 2, replace=False)
        neg.append((rng.choice(rows_of[l1]), rng.choice(rows_of[l2]), 0))
    pairs = pos + neg
    rng.shuffle(pairs)

    def cos(a, b):
        return np.dot(a / (np.linalg.norm(a) + 1e-8), b / (np.linalg.norm(b) + 1e-8))

    sims = np.array([cos(embeddings[i], embeddings[j]) for i, j, _ in pairs])
    same = np.array([s for _, _, s in pairs])
    best_acc, best = 0, threshold
    for t in SWEEP:
        acc = ((sims > t).astype(int) == same).mean()
        if acc > best_acc:
            best_acc, best = acc, t
    accuracy = ((sims > best).astype(int) == same).mean()
    return accuracy, best, {"accuracy": accuracy, "threshold": best, "pos_sim_mean": sims[same == 1].mean(),
                            "neg_sim_mean": sims[same == 0].mean(), "num_pos_pairs": len(pos), "num_neg_pairs": len(neg)}


def tar_at_far(S, labels, far):
    """(k, tar): k = floor(far x impostor pairs) false accepts allowed, and the share of genuine pairs strictly above
    the lowest score threshold that lets at most k impostor pairs through (the (k + 1)-th highest impostor score)."""
    S = np.asarray(S, np.float64)
    labels = np.asarray(labels)
    iu = np.triu_indices(len(labels), 1)
    s, gen = S[iu], (labels[:, None] == labels[None, :])[iu]
    imp = np.sort(s[~gen])[::-1]
    k = int(np.floor(far * imp.size + 1e-9))
    t = imp[k] if k < imp.size else -np.inf
    return k, float((s[gen] > t).mean())


def loo_rank1(r):
    """Leave-one-out rank-1 from all_pairs' row outputs: over the rows with a mate, the share whose best mate beats
    the best impostor (equal scores: the lower index wins)."""
    score, idx = r["row_score"], r["row_idx"]
    mate = idx[:, 0] >= 0
    win = (idx[:, 2] < 0) | (score[:, 0] > score[:, 2]) | ((score[:, 0] == score[:, 2]) & (idx[:, 0] < idx[:, 2]))
    return float(win[mate].mean()), int(mate.sum())
