"""Float64 numpy restatement of the t-SNE the device runs (facerecognition_amd/csrc/tsne.hip): sklearn.manifold.TSNE's
default algorithm with the repulsive term summed exactly.  Our own code, written from the published algorithm (van
der Maaten & Hinton 2008; sklearn's documented _binary_search_perplexity / _gradient_descent rules); test_tsne_ref.py
pins it against sklearn where sklearn imports.  Dense O(N^2) arrays: for test sizes only."""
import numpy as np

EPS32 = 2.0 ** -24


def planted_clusters(n_clusters, per, dim, noise, seed, centre_norms=None, normalise=True):
    """Rows around unit centres: centre + noise * N(0, 1) / sqrt(dim), renormalised (or scaled to centre_norms)."""
    rng = np.random.RandomState(seed)
    c = rng.standard_normal((n_clusters, dim))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    if centre_norms is not None:
        c *= np.asarray(centre_norms, np.float64)[:, None]
    x = np.repeat(c, per, axis=0) + noise * rng.standard_normal((n_clusters * per, dim)) / np.sqrt(dim)
    if normalise:
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float32), np.repeat(np.arange(n_clusters), per)


def knn_bruteforce(x, k):
    """(idx [N, k], d2 [N, k]) by squared Euclidean distance in float64, self excluded, ties by index."""
    x = np.asarray(x, np.float64)
    d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    idx = np.argsort(d, axis=1, kind="stable")[:, :k]
    return idx.astype(np.int32), np.take_along_axis(d, idx, axis=1)


def sqdist(x, idx):
    x = np.asarray(x, np.float64)
    return ((x[:, None, :] - x[idx]) ** 2).sum(-1)


def p_from_beta(d2, beta):
    """p_j|i for the given bandwidths; each row's smallest distance is subtracted first (p is unchanged by it)."""
    d = np.asarray(d2, np.float64)
    d = d - d.min(axis=1, keepdims=True)
    p = np.exp(-d * np.asarray(beta, np.float64)[:, None])
    s = p.sum(axis=1, keepdims=True)
    s[s == 0.0] = 1e-8
    return p / s


def entropy(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(p > 0, p * np.log(p), 0.0)
    return -t.sum(axis=1)


def binary_search_perplexity(d2, perplexity):
    """sklearn's rule: beta from 1, doubled / halved while unbounded, else bisected; at most 100 steps; stop at
    |H - log perplexity| <= 1e-5.  Returns (beta [N], p [N, k])."""
    d2 = np.asarray(d2, np.float64)
    target = np.log(perplexity)
    betas = np.empty(d2.shape[0])
    for i, row in enumerate(d2):
        d = row - row.min()
        beta, lo, hi = 1.0, -np.inf, np.inf
        for _ in range(100):
            p = np.exp(-d * beta)
            sp = p.sum()
            if sp == 0.0:
                sp = 1e-8
            diff = np.log(sp) + beta * (d * p).sum() / sp - target
            if abs(diff) <= 1e-5:
                break
            if diff > 0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
        betas[i] = beta
    return betas, p_from_beta(d2, betas)


def joint_csr(idx, p_cond):
    """P_ij = (p_j|i + p_i|j) / (2 N) as CSR (indptr, col, val) with ascending columns."""
    idx = np.asarray(idx, np.int64)
    n, k = idx.shape
    r = np.repeat(np.arange(n, dtype=np.int64), k)
    c = idx.ravel()
    v = np.asarray(p_cond, np.float64).ravel()
    key = np.concatenate([r * n + c, c * n + r])
    uniq, inv = np.unique(key, return_inverse=True)
    val = np.zeros(uniq.size)
    np.add.at(val, inv, np.concatenate([v, v]))
    rows = uniq // n
    indptr = np.zeros(n + 1, np.int64)
    np.add.at(indptr, rows + 1, 1)
    return np.cumsum(indptr).astype(np.int32), (uniq % n).astype(np.int32), val / (2.0 * n)


def csr_to_dense(indptr, col, val, n):
    p = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(indptr))
    p[rows, col[:indptr[n]]] = val[:indptr[n]]
    return p


def gradient(p_dense, y, exaggeration=1.0):
    """Returns dict(grad [N, 2], kl, z, gnorm, bound [N, 2], z_abs, kl_abs): bound = the per-component sum of absolute
    terms S_i of the gradient (the summation-error yardstick), z_abs / kl_abs the same for Z and KL."""
    y = np.asarray(y, np.float64)
    n = y.shape[0]
    diff = y[:, None, :] - y[None, :, :]
    d = 1.0 + (diff ** 2).sum(-1)
    w = 1.0 / d
    np.fill_diagonal(w, 0.0)
    z = w.sum()
    pw = p_dense * w
    attr = (pw[:, :, None] * diff).sum(1)
    rep = ((w * w)[:, :, None] * diff).sum(1)
    grad = 4.0 * (exaggeration * attr - rep / z)
    bound = 4.0 * (exaggeration * (pw[:, :, None] * np.abs(diff)).sum(1) + ((w * w)[:, :, None] * np.abs(diff)).sum(1) / z)
    nz = p_dense > 0
    terms = p_dense[nz] * (np.log(p_dense[nz]) + np.log(d[nz]))
    return dict(grad=grad, kl=terms.sum() + np.log(z), z=z, gnorm=np.sqrt((grad ** 2).sum()), bound=bound,
                z_abs=z, kl_abs=np.abs(terms).sum() + abs(np.log(z)))


def step(grad, y, update, gains, momentum, learning_rate):
    """One step of sklearn's _gradient_descent; returns new (y, update, gains)."""
    inc = update * grad < 0.0
    gains = np.where(inc, gains + 0.2, gains * 0.8)
    gains = np.maximum(gains, 0.01)
    update = momentum * update - learning_rate * (gains * grad)
    return y + update, update, gains


def fit(p_dense, y0, max_iter=1000, early_exaggeration=12.0, learning_rate=None, n_iter_without_progress=300,
        min_grad_norm=1e-7):
    """sklearn's TSNE._tsne schedule; returns (y, kl, last iteration)."""
    n = y0.shape[0]
    lr = max(n / early_exaggeration / 4.0, 50.0) if learning_rate is None else learning_rate
    y = np.asarray(y0, np.float64).copy()
    kl, it = np.nan, -1
    stages = [(min(250, max_iter), early_exaggeration, 0.5, 250)]
    if max_iter > 250:
        stages.append((max_iter, 1.0, 0.8, n_iter_without_progress))
    for stop, e, momentum, patience in stages:
        update, gains = np.zeros_like(y), np.ones_like(y)
        best, best_it = np.finfo(np.float64).max, it + 1
        for i in range(it + 1, stop):
            it = i
            g = gradient(p_dense, y, e)
            kl = g["kl"]
            y, update, gains = step(g["grad"], y, update, gains, momentum, lr)
            if (i + 1) % 50 == 0:
                if kl < best:
                    best, best_it = kl, i
                elif i - best_it > patience:
                    break
                if g["gnorm"] <= min_grad_norm:
                    break
    return y, kl, it


def nearest_neighbour_purity(y, labels):
    """Share of points whose nearest 2-D neighbour has their label."""
    y = np.asarray(y, np.float64)
    d = ((y[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    return float(np.mean(labels[np.argmin(d, axis=1)] == labels))
