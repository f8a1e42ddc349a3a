#!/usr/bin/env python3
"""Writes tests/golden/tsne_golden.npz: the float64 restatement's (tests/tsne_ref.py) KL divergence, trustworthiness
and nearest-neighbour purity on the end-to-end test's input -- 256 rows in 8 planted clusters, D = 512, perplexity
10, 500 iterations -- from 8 seeded random inits.  tests/test_gpu_tsne.py reads the file instead of rerunning the
float64 loop; the device run is one more draw from the same set of local optima.  No GPU.

    python tools/gen_tsne_golden.py [--out tests/golden/tsne_golden.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import tsne_ref as R  # noqa: E402

CLUSTERS, PER, DIM, NOISE, DATA_SEED = 8, 32, 512, 0.6, 0
PERPLEXITY, MAX_ITER = 10.0, 500
INIT_SEEDS = list(range(8))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "tsne_golden.npz"))
    a = ap.parse_args(argv)
    try:
        from sklearn.manifold import trustworthiness
    except ImportError:
        trustworthiness = None
    x, labels = R.planted_clusters(CLUSTERS, PER, DIM, NOISE, DATA_SEED)
    n = x.shape[0]
    k = min(n - 1, int(3 * PERPLEXITY + 1))
    idx, d2 = R.knn_bruteforce(x, k)
    _, p = R.binary_search_perplexity(d2, PERPLEXITY)
    dense = R.csr_to_dense(*R.joint_csr(idx, p), n)
    kl, trust, purity = [], [], []
    for seed in INIT_SEEDS:
        y0 = 1e-4 * np.random.RandomState(seed).standard_normal((n, 2))
        y, e, _ = R.fit(dense, y0, max_iter=MAX_ITER)
        kl.append(e)
        purity.append(R.nearest_neighbour_purity(y, labels))
        trust.append(trustworthiness(x, y, n_neighbors=5) if trustworthiness else np.nan)
        print(f"seed {seed}: KL {kl[-1]:.4f} trustworthiness {trust[-1]:.4f} purity {purity[-1]:.3f}")
    np.savez(a.out, clusters=CLUSTERS, per=PER, dim=DIM, noise=NOISE, data_seed=DATA_SEED, perplexity=PERPLEXITY,
             max_iter=MAX_ITER, init_seeds=np.array(INIT_SEEDS), kl=np.array(kl), trustworthiness=np.array(trust),
             purity=np.array(purity))
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
