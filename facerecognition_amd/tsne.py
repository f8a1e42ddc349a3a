"""t-SNE of embeddings on the device (libfrhip fr_tsne_*; DESIGN.md §4 "t-SNE").

``TSNE`` follows ``sklearn.manifold.TSNE``'s defaults -- sparse kNN input affinities at 3 * perplexity neighbours,
early exaggeration, the gains / momentum optimiser and its stopping rules -- with the repulsive term summed exactly
over all pairs instead of Barnes-Hut's approximation.  It replaces the sklearn call in the reference's
``visualize_tsne`` (inference/extract_embeddings.py:648-711), which subsamples to 2000 rows because the host run is
slow.  Two components only.  There is no CPU fallback: without a GPU ``fit`` raises ``RuntimeError``.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _native as N

N_ITER_CHECK = 50          # sklearn's _N_ITER_CHECK: steps per fr_tsne_run call, one stats read-back each
EXPLORATION_ITERS = 250    # sklearn's _EXPLORATION_MAX_ITER (= its n_iter_without_progress for that stage)
SEARCH_CHUNK = 4096        # probes per fr_match_topk call of the neighbour search
UNIT_NORM_TOL = 1e-3       # the gallery's rule: rows within this of unit norm are matched as they are


def auto_learning_rate(n_samples: int, early_exaggeration: float) -> float:
    """sklearn's learning_rate='auto'."""
    return max(n_samples / early_exaggeration / 4.0, 50.0)


def n_neighbors(n_samples: int, perplexity: float) -> int:
    return min(n_samples - 1, int(3.0 * perplexity + 1))


def augmented_rows(X: np.ndarray):
    """Rows whose inner product ranks by Euclidean distance: gallery [x, |x|^2, r] / M and probes [x, -1/2, 0],
    zero-padded to a multiple of 4 columns.  probe . gallery = (|x_i|^2 - |x_i - x_j|^2) / (2 M); r = sqrt(M^2 - |x|^2
    - |x|^4) gives every gallery row unit norm, so the gallery's normalisation rule leaves them as they are."""
    X = np.asarray(X, np.float64)
    n, d = X.shape
    sq = np.einsum("ij,ij->i", X, X)
    m2 = float(np.max(sq + sq * sq)) or 1.0
    da = (d + 2 + 3) // 4 * 4
    g = np.zeros((n, da), np.float64)
    p = np.zeros((n, da), np.float64)
    g[:, :d] = X
    g[:, d] = sq
    g[:, d + 1] = np.sqrt(np.maximum(m2 - sq - sq * sq, 0.0))
    g /= np.sqrt(m2)
    p[:, :d] = X
    p[:, d] = -0.5
    return g.astype(np.float32), p.astype(np.float32)


def pca_init(X_dev):
    """The top two principal axes' scores, scaled so the first has standard deviation 1e-4 (sklearn's init='pca');
    X^T X on the device, eigh on the host.  Each axis is signed so that its largest component is positive."""
    import torch

    xc = X_dev.double() - X_dev.double().mean(dim=0, keepdim=True)
    cov = (xc.T @ xc).cpu().numpy()
    _, vec = np.linalg.eigh(cov)
    axes = vec[:, ::-1][:, :2].copy()
    for c in range(axes.shape[1]):
        if axes[np.argmax(np.abs(axes[:, c])), c] < 0:
            axes[:, c] = -axes[:, c]
    y = (xc @ torch.from_numpy(axes).to(xc.device)).cpu().numpy()
    sd = float(np.std(y[:, 0]))
    return (y / (sd if sd > 0 else 1.0) * 1e-4).astype(np.float32)


class TSNE:
    def __init__(self, n_components: int = 2, perplexity: float = 30.0, early_exaggeration: float = 12.0,
                 learning_rate="auto", max_iter: int = 1000, n_iter_without_progress: int = 300,
                 min_grad_norm: float = 1e-7, init="pca", random_state=None, device: int = 0,
                 n_iter: Optional[int] = None):
        self.n_components = n_components
        self.perplexity = perplexity
        self.early_exaggeration = early_exaggeration
        self.learning_rate = learning_rate
        self.max_iter = int(n_iter) if n_iter is not None else int(max_iter)  # n_iter: sklearn < 1.5's name
        self.n_iter_without_progress = n_iter_without_progress
        self.min_grad_norm = min_grad_norm
        self.init = init
        self.random_state = random_state
        self.device = device

    # ---- host-side argument handling (no GPU needed) ----
    def _check(self, X: np.ndarray):
        if self.n_components != 2:
            raise ValueError(f"TSNE: n_components must be 2 (got {self.n_components})")
        if X.ndim != 2 or X.shape[0] < 2 or X.shape[1] < 1:
            raise ValueError(f"TSNE: X must be (n_samples >= 2, n_features >= 1), got {X.shape}")
        n = X.shape[0]
        if not np.isfinite(self.perplexity) or self.perplexity <= 0 or self.perplexity >= n:
            raise ValueError(f"TSNE: perplexity must be positive and less than n_samples ({n}), got {self.perplexity}")
        if self.max_iter < 1:
            raise ValueError(f"TSNE: max_iter must be at least 1, got {self.max_iter}")
        if isinstance(self.init, str):
            if self.init not in ("pca", "random"):
                raise ValueError(f"TSNE: init must be 'pca', 'random' or an (n_samples, 2) array, got {self.init!r}")
        elif np.asarray(self.init).shape != (n, 2):
            raise ValueError(f"TSNE: init array must have shape ({n}, 2), got {np.asarray(self.init).shape}")
        if self.learning_rate == "auto":
            self.learning_rate_ = auto_learning_rate(n, self.early_exaggeration)
        else:
            self.learning_rate_ = float(self.learning_rate)
        for name, v in (("early_exaggeration", self.early_exaggeration), ("learning_rate", self.learning_rate_)):
            if not np.isfinite(v) or v <= 0:
                raise ValueError(f"TSNE: {name} must be finite and positive, got {v}")

    def _init_host(self, n: int):
        """init='random' or an array; None for 'pca' (computed from the device rows)."""
        if isinstance(self.init, str):
            if self.init == "pca":
                return None
            rs = self.random_state if isinstance(self.random_state, np.random.RandomState) \
                else np.random.RandomState(self.random_state)
            return (1e-4 * rs.standard_normal(size=(n, 2))).astype(np.float32)
        return np.ascontiguousarray(np.asarray(self.init, np.float32))

    # ---- device steps ----
    def _neighbors(self, X: np.ndarray, k: int):
        """idx [N, k] int32 on the device: each row's k nearest other rows by the exact top-k of a temporary gallery."""
        import torch

        from .gallery import DeviceGallery

        n, d = X.shape
        norms = np.linalg.norm(X.astype(np.float64), axis=1)
        if d % 4 == 0 and np.all(np.abs(norms - 1.0) < UNIT_NORM_TOL):
            g = p = np.ascontiguousarray(X, np.float32)
        else:
            g, p = augmented_rows(X)
        gal = DeviceGallery(g, dim=g.shape[1], device=self.device)
        dev = gal.device
        idx = torch.empty((n, k), dtype=torch.int32, device=dev)
        try:
            for r0 in range(0, n, SEARCH_CHUNK):
                r1 = min(r0 + SEARCH_CHUNK, n)
                _, cand = gal.search_device(torch.from_numpy(p[r0:r1]).to(dev), k + 1)
                own = torch.arange(r0, r1, dtype=torch.int32, device=dev)[:, None]
                is_own = cand == own
                # drop the row's own index, or the last entry where a duplicate row displaced it
                drop = torch.where(is_own.any(dim=1), is_own.int().argmax(dim=1), torch.full_like(own[:, 0], k).long())
                keep = torch.ones_like(cand, dtype=torch.bool)
                keep[torch.arange(r1 - r0, device=dev), drop] = False
                idx[r0:r1] = cand[keep].reshape(r1 - r0, k)
        finally:
            gal.close()
        return idx

    def _affinities(self, X: np.ndarray, dev):
        """(indptr, col, val) of the joint P as device tensors, and the rows on the device."""
        import torch

        n, d = X.shape
        k = n_neighbors(n, self.perplexity)
        L = N.lib()
        stream = N.stream_ptr(dev)
        idx = self._neighbors(X, k)
        xd = torch.from_numpy(X).to(dev)
        d2 = torch.empty((n, k), dtype=torch.float32, device=dev)
        N.check(L.fr_tsne_knn_sqdist(N.ptr(xd), n, d, N.ptr(idx), k, N.ptr(d2), stream), "fr_tsne_knn_sqdist")
        nws = L.fr_tsne_affinities_workspace(n, k)
        if not nws:
            N.check(-1, "fr_tsne_affinities_workspace")
        ws = torch.empty((nws,), dtype=torch.uint8, device=dev)
        indptr = torch.empty((n + 1,), dtype=torch.int32, device=dev)
        col = torch.empty((2 * n * k,), dtype=torch.int32, device=dev)
        val = torch.empty((2 * n * k,), dtype=torch.float32, device=dev)
        beta = torch.empty((n,), dtype=torch.float32, device=dev)
        N.check(L.fr_tsne_affinities(N.ptr(idx), N.ptr(d2), n, k, float(self.perplexity), N.ptr(indptr), N.ptr(col),
                                     N.ptr(val), N.ptr(beta), N.ptr(ws), nws, stream), "fr_tsne_affinities")
        torch.cuda.synchronize(dev)  # the workspace is freed on return
        return (indptr, col, val), xd

    def fit(self, X, y=None):
        import torch

        X = np.asarray(X)
        self._check(X)
        y0 = self._init_host(X.shape[0])
        if not torch.cuda.is_available():
            raise RuntimeError("TSNE needs a ROCm GPU; there is deliberately no CPU fallback")
        X = np.ascontiguousarray(X, np.float32)
        dev = torch.device("cuda", self.device)
        with torch.cuda.device(dev):
            (indptr, col, val), xd = self._affinities(X, dev)
            if y0 is None:
                y0 = pca_init(xd)
            del xd
            Y = torch.from_numpy(y0).to(dev).contiguous()
            self._optimise(N.lib(), indptr, col, val, X.shape[0], Y, N.stream_ptr(dev), dev)
            self.embedding_ = Y.cpu().numpy()
        return self

    def _optimise(self, L, indptr, col, val, n, Y, stream, dev):
        import torch

        gws = L.fr_tsne_gradient_workspace(n)
        if not gws:
            N.check(-1, "fr_tsne_gradient_workspace")
        ws = torch.empty((gws,), dtype=torch.uint8, device=dev)
        grad = torch.empty((n, 2), dtype=torch.float32, device=dev)
        stats = torch.zeros((3,), dtype=torch.float64, device=dev)
        update = torch.zeros((n, 2), dtype=torch.float32, device=dev)
        gains = torch.ones((n, 2), dtype=torch.float32, device=dev)
        explore = min(EXPLORATION_ITERS, self.max_iter)
        stages = [(explore, float(self.early_exaggeration), 0.5, EXPLORATION_ITERS)]
        if self.max_iter > explore:
            stages.append((self.max_iter, 1.0, 0.8, int(self.n_iter_without_progress)))
        kl, it = float("nan"), -1
        for stop, exaggeration, momentum, patience in stages:
            update.zero_()   # sklearn starts each _gradient_descent call from zero update and unit gains
            gains.fill_(1.0)
            i = it + 1       # ... and the second stage where the first one stopped
            best, best_it = np.finfo(np.float64).max, i
            while i < stop:
                steps = min(N_ITER_CHECK - i % N_ITER_CHECK, stop - i)
                N.check(L.fr_tsne_run(N.ptr(indptr), N.ptr(col), N.ptr(val), n, N.ptr(Y), N.ptr(update), N.ptr(gains),
                                      exaggeration, momentum, float(self.learning_rate_), steps, N.ptr(grad),
                                      N.ptr(stats), N.ptr(ws), gws, stream), "fr_tsne_run")
                i += steps
                it = i - 1
                kl, _, gnorm = stats.cpu().tolist()
                if i % N_ITER_CHECK == 0:
                    if kl < best:
                        best, best_it = kl, it
                    elif it - best_it > patience:
                        break
                    if gnorm <= self.min_grad_norm:
                        break
        self.kl_divergence_ = float(kl)
        self.n_iter_ = int(it)

    def fit_transform(self, X, y=None):
        return self.fit(X).embedding_
