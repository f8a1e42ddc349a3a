"""Triplet mining and the triplet margin loss restated in numpy (a test helper, like arcmargin_ref.py): the rules of
include/frhip.h "Triplet mining and loss".

Part (a), ``gram_dist_f32`` + ``mine``: the device's own arithmetic in float32 (Gram form, IEEE sqrt, float32
comparisons).  Bitwise the device's only where every product and partial sum is exact in float32 (the exact-grid tests:
multiples of 1/8 in [-2, 2]); there the order of the sums does not matter.

Part (b), ``dist_f64`` + ``valid_choice`` + ``loss_ref``: float64, with bounds computed from float64 values alone, never
from a device output.  With eps = 2^-24 (float32's unit roundoff), s_i = |e_i|^2, A_ij = sum_k |e_ik e_jk|:

  d2      |d d2_ij| <= (D + 16) eps (s_i + s_j + 2 A_ij) =: q_ij
          (D squares and D products summed in any order, the two additions of the Gram form, 16 for slack)
  d       |d d_ij| <= min(sqrt(q_ij), q_ij / d_ij) + 2 eps d_ij =: db_ij
          (|sqrt(x~) - sqrt(x)| = |x~ - x| / (sqrt(x~) + sqrt(x)) is at most both; the square root's rounding)
  tests   d_an > d_ap is decided up to t1 = db_an + db_ap; d_an < fl(d_ap + m) up to t2 = t1 + 2 eps (d_ap + m).
          A negative is CERTAINLY semi-hard when both hold with these margins, POSSIBLY when neither fails by more.
  choice  an argmin over a set S picks c with d32_c <= d32_j for all j in S, so d_c - db_c <= min_j (d_j + db_j);
          argmax likewise with the signs exchanged.
  delta   z_k = x_k - y_k + 1e-6, w_k = |x_k - y_k| + 1e-6 >= |z_k|:  |d z_k| <= 2 eps w_k, the sum of squares
          errs by at most (D + 16) eps sum w_k^2 =: Q, so |d delta| <= min(sqrt(Q), Q / delta) + 2 eps delta =: eb
          (the plain distance |x - y| likewise with w_k = |x_k - y_k|)
  hinge   x = fl(fl(m + delta_ap) - delta_an): |dx| <= eb_ap + eb_an + 2 eps (m + delta_ap + |x|) =: xb; max(., 0) is
          1-Lipschitz
  mean    thread i of 1024 adds the terms i, i + 1024, ... in order, then a 10-level tree and one division:
          (ceil(T / 1024) + 16) eps mean |term| on top of the mean of the terms' bounds
  dE      a triplet with |x| <= xb may count as active or not: its whole contribution goes into the bound (unless rows
          p and n are equal: then delta_ap and delta_an are the same float and fl(m + delta) - delta >= 0 by the
          monotonicity of rounding: certainly active).  Otherwise w = (u / T) / delta has relative error
          eb / delta + 4 eps, the term w z_k errs by |w| 2 eps w_k + |w z_k| (eb / delta + 6 eps), and a row's M terms
          are summed in some order: (M + 16) eps sum |terms|.
"""
import numpy as np

EPS = 2.0 ** -24
PAIR_EPS = 1e-6
SEMI_HARD, BATCH_HARD, FIRST = 0, 1, 2


def make_labels(N, rng):
    """Classes of about 20, 4, 2 and 1 rows (then 4s up to N), shuffled so that no class is contiguous."""
    sizes = [s for s in (20, 4, 2, 1, 4, 2, 1, 1) if s <= max(N // 3, 1)]
    lab = []
    for s in sizes:
        if len(lab) + s <= N:
            lab += [len(set(lab)) * 3 - 7] * s  # arbitrary values, negative ones included
    while len(lab) < N:
        lab += [len(set(lab)) * 3 - 7] * min(4, N - len(lab))
    return rng.permutation(np.array(lab, np.int32))


def grid_case(N, D, seed):
    """Exact-grid inputs: multiples of 1/8 in [-2, 2] (every product and partial sum is exact in float32), clustered by
    class, with duplicated rows (within a class and across classes) and deliberate ties: rows c + v and c - v are
    equally far from every row equal to c."""
    rng = np.random.default_rng(seed)
    labels = make_labels(N, rng)
    classes = np.unique(labels)
    centres = {c: rng.integers(-10, 11, D) for c in classes}
    E = np.zeros((N, D), np.int64)
    for i in range(N):
        v = np.zeros(D, np.int64)
        k = rng.integers(0, 4)  # 0: the centre itself (duplicates within the class)
        v[rng.integers(0, D, k)] = rng.integers(-3, 4, k)
        E[i] = centres[labels[i]] + v
    if N >= 8:
        order = rng.permutation(N)
        E[order[0]] = 2 * centres[labels[order[1]]] - E[order[1]]  # the mirror image of a row about its centre
        E[order[2]] = E[order[3]]                                   # a duplicate, most likely across classes
        near = [c for c in classes if c != labels[order[4]]][0]
        centres[near] = centres[labels[order[4]]].copy()            # two classes on one centre: many exact ties
        centres[near][0] += 1
        for i in np.flatnonzero(labels == near):
            E[i] = centres[near]
    return (np.clip(E, -16, 16) / 8.0).astype(np.float32), labels


SPREAD = {16: 0.8, 128: 1.0, 512: 0.8}  # tuned per D at margin 0.2: test_triplet_ref.py checks the semi-hard share
FLOAT_SHAPES = ((70, 16), (130, 128), (257, 512))
FLOAT_MARGIN = 0.2


def float_case(N, D, seed):
    """Float inputs of the GPU tests: unit-norm rows, class centres from a 4-dimensional latent (so that the distances
    between classes vary widely), a spread per class."""
    rng = np.random.default_rng(seed)
    labels = make_labels(N, rng)
    classes = np.unique(labels)
    proj = np.linalg.qr(rng.standard_normal((D, 4)))[0].T
    E = np.zeros((N, D))
    for c in classes:
        centre = rng.standard_normal(4) @ proj
        rows = np.flatnonzero(labels == c)
        sigma = SPREAD[D] * rng.uniform(0.2, 1.0)
        E[rows] = centre + sigma * rng.standard_normal((len(rows), D)) / np.sqrt(D)
    E /= np.linalg.norm(E, axis=1, keepdims=True)
    return E.astype(np.float32), labels


def counts(labels, mode):
    """lims [N + 1] from the labels alone."""
    labels = np.asarray(labels)
    N = len(labels)
    same = (labels[:, None] == labels[None, :]).sum(1)
    c = np.where((same > 1) & (same < N), 1 if mode == BATCH_HARD else same - 1, 0)
    return np.concatenate([[0], np.cumsum(c)]).astype(np.int64)


def gram_dist_f32(E):
    """Part (a): d = sqrt(max(s_i + s_j - 2 g_ij, 0)) in float32."""
    E = np.asarray(E, np.float32)
    g = (E.astype(np.float64) @ E.astype(np.float64).T).astype(np.float32)
    s = (E.astype(np.float64) ** 2).sum(1).astype(np.float32)
    d2 = np.maximum((s[:, None] + s[None, :]) - np.float32(2) * g, np.float32(0))
    assert d2.dtype == np.float32
    return np.sqrt(d2)


def mine(dist, labels, mode, margin):
    """The reference's loops over a distance matrix, in the matrix's own precision; np.argmin / argmax take the
    lowest index of equal values.  Returns (lims, a, p, n, semi)."""
    labels = np.asarray(labels)
    N = len(labels)
    m = dist.dtype.type(np.float32(margin))
    idx = np.arange(N)
    a_, p_, n_, s_ = [], [], [], []
    for i in range(N):
        pos = idx[(labels == labels[i]) & (idx != i)]
        neg = idx[labels != labels[i]]
        if len(pos) == 0 or len(neg) == 0:
            continue
        dn = dist[i, neg]
        if mode == BATCH_HARD:
            a_.append(i); p_.append(pos[np.argmax(dist[i, pos])]); n_.append(neg[np.argmin(dn)]); s_.append(0)
            continue
        for p in pos:
            dap = dist[i, p]
            thr = dap + m
            mask = (dn > dap) & (dn < thr)
            if mask.any():
                n = neg[mask][0] if mode == FIRST else neg[mask][np.argmin(dn[mask])]
            else:
                n = neg[np.argmax(dn)] if mode == FIRST else neg[np.argmin(dn)]
            a_.append(i); p_.append(p); n_.append(n); s_.append(int(mask.any()))
    return (counts(labels, mode), np.array(a_, np.int64), np.array(p_, np.int64), np.array(n_, np.int64),
            np.array(s_, np.uint8))


def dist_f64(E):
    """Part (b): the true distances of the float32 rows and the bound db on the device's Gram-form error."""
    E = np.asarray(E, np.float64)
    D = E.shape[1]
    s = (E * E).sum(1)
    d = np.sqrt(np.maximum(((E[:, None, :] - E[None, :, :]) ** 2).sum(2), 0.0))
    q = (D + 16) * EPS * (s[:, None] + s[None, :] + 2 * (np.abs(E) @ np.abs(E).T))
    with np.errstate(divide="ignore", invalid="ignore"):
        db = np.minimum(np.sqrt(q), np.where(d > 0, q / d, np.inf)) + 2 * EPS * d
    return d, db


def pair_case(d, db, labels, margin, a, p):
    """The negatives of anchor a and, for the pair (a, p), which of them are certainly / possibly semi-hard."""
    labels = np.asarray(labels)
    neg = np.flatnonzero(labels != labels[a])
    m = float(np.float32(margin))
    t1 = db[a, neg] + db[a, p]
    t2 = t1 + 2 * EPS * (d[a, p] + m)
    lo, hi = d[a, neg] - d[a, p], d[a, p] + m - d[a, neg]
    return neg, (lo > t1) & (hi > t2), (lo > -t1) & (hi > -t2)


def _argmin_ok(d, db, a, c, cand):
    return d[a, c] - db[a, c] <= (d[a, cand] + db[a, cand]).min()


def _argmax_ok(d, db, a, c, cand):
    return d[a, c] + db[a, c] >= (d[a, cand] - db[a, cand]).max()


def valid_choice(d, db, labels, mode, margin, a, p, n):
    """Whether the device's triplet (a, p, n) is a choice float32 arithmetic within the bounds can make.  Returns
    (ok, case) with case in 'semi' (a certainly semi-hard negative exists), 'fallback' (none is possibly semi-hard),
    'either' (undecided within the bounds: either rule's outcome is accepted) or 'hard'."""
    labels = np.asarray(labels)
    if not (labels[p] == labels[a] and p != a and labels[n] != labels[a]):
        return False, "labels"
    if mode == BATCH_HARD:
        pos = np.flatnonzero((labels == labels[a]) & (np.arange(len(labels)) != a))
        neg = np.flatnonzero(labels != labels[a])
        return bool(_argmax_ok(d, db, a, p, pos) and _argmin_ok(d, db, a, n, neg)), "hard"
    neg, certain, possible = pair_case(d, db, labels, margin, a, p)
    is_possible = bool(possible[neg == n][0])
    fallback_ok = bool(_argmax_ok(d, db, a, n, neg) if mode == FIRST else _argmin_ok(d, db, a, n, neg))
    if certain.any():
        if mode == FIRST:
            return is_possible and n <= neg[certain][0], "semi"
        return is_possible and bool(_argmin_ok(d, db, a, n, neg[certain])), "semi"
    if not possible.any():
        return fallback_ok, "fallback"
    return is_possible or fallback_ok, "either"


def _delta(x, y, shift):
    """|x - y + shift| per row and the bound on the float32 result."""
    D = x.shape[1]
    z = x - y + shift
    w = np.abs(x - y) + shift
    dl = np.sqrt((z * z).sum(1))
    Q = (D + 16) * EPS * (w * w).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        eb = np.minimum(np.sqrt(Q), np.where(dl > 0, Q / dl, np.inf)) + 2 * EPS * dl
    return z, w, dl, eb


def loss_ref(E, a, p, n, margin, u=1.0):
    """nn.TripletMarginLoss(margin, p=2) of E[a], E[p], E[n] in float64, the gradient of u loss by E, the metrics of
    compute_triplet_metrics, and the bounds on the float32 results (module docstring)."""
    E = np.asarray(E, np.float64)
    a, p, n = (np.asarray(v, np.int64) for v in (a, p, n))
    N, D = E.shape
    T = len(a)
    m = float(np.float32(margin))
    zp, wp, dap, ebp = _delta(E[a], E[p], PAIR_EPS)
    zn, wn, dan, ebn = _delta(E[a], E[n], PAIR_EPS)
    _, _, pd, pdb = _delta(E[a], E[p], 0.0)
    _, _, nd, ndb = _delta(E[a], E[n], 0.0)
    x = m + dap - dan
    xb = ebp + ebn + 2 * EPS * (m + dap + np.abs(x))
    h = np.maximum(x, 0.0)
    red = (-(-T // 1024) + 16) * EPS

    def mean(v, vb):
        return v.mean(), vb.mean() + red * np.abs(v).mean()

    loss, loss_b = mean(h, xb)
    pos_dist, pos_b = mean(pd, pdb)
    neg_dist, neg_b = mean(nd, ndb)
    gap_b = pdb + ndb
    acc_lo, acc_hi = (nd - pd > gap_b).mean(), (nd - pd >= -gap_b).mean()

    same_pn = np.array([np.array_equal(E[pi], E[ni]) for pi, ni in zip(p, n)])
    active = (x >= 0) | same_pn
    unsure = (np.abs(x) <= xb) & ~same_pn
    s = float(u) / T
    with np.errstate(divide="ignore", invalid="ignore"):
        cp = np.where(dap > 0, s / dap, 0.0)
        cn = np.where(dan > 0, s / dan, 0.0)
        rp = np.where(dap > 0, ebp / dap, 0.0) + 6 * EPS
        rn = np.where(dan > 0, ebn / dan, 0.0) + 6 * EPS
    tp, tn = cp[:, None] * zp, cn[:, None] * zn                                    # [T, D] terms
    tpb = np.abs(cp)[:, None] * 2 * EPS * wp + np.abs(tp) * rp[:, None]
    tnb = np.abs(cn)[:, None] * 2 * EPS * wn + np.abs(tn) * rn[:, None]
    dE, bound, mag, cnt = np.zeros((N, D)), np.zeros((N, D)), np.zeros((N, D)), np.zeros(N)
    for t in range(T):
        for row, term, tb in ((a[t], tp[t], tpb[t]), (a[t], -tn[t], tnb[t]), (p[t], -tp[t], tpb[t]),
                              (n[t], tn[t], tnb[t])):
            if unsure[t]:
                bound[row] += np.abs(term) + tb
                cnt[row] += 1
                if active[t]:
                    dE[row] += term
            elif active[t]:
                dE[row] += term
                bound[row] += tb
                mag[row] += np.abs(term)
                cnt[row] += 1
    bound += (cnt[:, None] + 16) * EPS * mag
    return dict(loss=loss, loss_bound=loss_b, hinge=h, hinge_bound=xb, x=x, active=active, unsure=unsure,
                pos_dist=pos_dist, pos_dist_bound=pos_b, neg_dist=neg_dist, neg_dist_bound=neg_b, pd=pd, nd=nd,
                accuracy=(nd > pd).mean(), accuracy_lo=acc_lo, accuracy_hi=acc_hi, dE=dE, dE_bound=bound,
                delta_ap=dap, delta_an=dan)
