"""tests/tsne_ref.py (the float64 restatement the GPU tests compare with) pinned against sklearn, where sklearn
imports: gradient and KL against sklearn.manifold._t_sne._kl_divergence on a dense P, the bandwidth search against
sklearn.manifold._utils._binary_search_perplexity.  No GPU."""
import numpy as np
import pytest

from tests import tsne_ref as R

pytest.importorskip("sklearn")


def _dense_p(n, seed):
    rng = np.random.RandomState(seed)
    p = rng.uniform(0.1, 1.0, (n, n))
    p = p + p.T
    np.fill_diagonal(p, 0.0)
    return p / p.sum()


@pytest.mark.parametrize("n,scale,e", [(7, 1.0, 1.0), (40, 1e-4, 12.0), (65, 30.0, 1.0), (33, 1.0, 12.0)])
def test_gradient_and_kl_match_sklearn(n, scale, e):
    from scipy.spatial.distance import squareform
    from sklearn.manifold._t_sne import _kl_divergence

    p = _dense_p(n, n)
    y = scale * np.random.RandomState(n + 1).standard_normal((n, 2))
    kl_sk, g_sk = _kl_divergence(y.ravel(), squareform(e * p, checks=False), 1.0, n, 2)
    g = R.gradient(p, y, e)
    assert np.abs(g["grad"].ravel() - g_sk).max() <= 1e-10 * np.abs(g_sk).max()
    if e == 1.0:  # sklearn's error is of the P it is given; ours is always of the unexaggerated P
        assert abs(g["kl"] - kl_sk) <= 1e-10 * abs(kl_sk)


@pytest.mark.parametrize("n,k,perplexity,seed", [(60, 31, 10.0, 0), (120, 91, 30.0, 1), (40, 16, 5.0, 2)])
def test_bandwidth_search_matches_sklearn(n, k, perplexity, seed):
    from sklearn.manifold._utils import _binary_search_perplexity

    x, _ = R.planted_clusters(4, n // 4, 32, 0.6, seed)
    idx, d2 = R.knn_bruteforce(x, k)
    d2 = d2.astype(np.float32)
    p_sk = np.asarray(_binary_search_perplexity(d2, perplexity, 0), np.float64)
    _, p = R.binary_search_perplexity(d2, perplexity)
    h_sk, h = R.entropy(p_sk), R.entropy(p)
    print("entropy error: sklearn %.3g, restatement %.3g; max |P - P_sklearn| %.3g" % (
        np.abs(h_sk - np.log(perplexity)).max(), np.abs(h - np.log(perplexity)).max(), np.abs(p - p_sk).max()))
    assert np.abs(h - np.log(perplexity)).max() <= 1e-5
    assert np.abs(h_sk - np.log(perplexity)).max() <= 1e-5
    np.testing.assert_allclose(p.sum(axis=1), 1.0, rtol=0, atol=1e-12)


def test_joint_csr_is_the_symmetrised_dense_matrix():
    x, _ = R.planted_clusters(3, 10, 16, 0.6, 5)
    idx, d2 = R.knn_bruteforce(x, 7)
    _, p = R.binary_search_perplexity(d2, 3.0)
    n = x.shape[0]
    dense = np.zeros((n, n))
    dense[np.repeat(np.arange(n), 7), idx.ravel()] = p.ravel()
    indptr, col, val = R.joint_csr(idx, p)
    np.testing.assert_allclose(R.csr_to_dense(indptr, col, val, n), (dense + dense.T) / (2 * n), rtol=0, atol=1e-18)
    for i in range(n):
        assert np.all(np.diff(col[indptr[i]:indptr[i + 1]]) > 0)
    assert abs(val.sum() - 1.0) < 1e-12
