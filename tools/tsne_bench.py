#!/usr/bin/env python3
"""Time the device t-SNE (DESIGN.md §4 t-SNE): ``TSNE.fit_transform`` on N rows of planted unit clusters, D = 512,
perplexity 30, 1000 iterations; default N = 2000 and N = 46715 (the gallery the reference's notebooks evaluate).

Per N one JSON line with
  fit_ms            fit_transform end to end (events on the launching stream; median of --runs after one warm-up),
  affinities_ms     neighbour search + distances + bandwidth search + symmetrisation (one run),
  step_ms           one optimiser iteration = fr_tsne_run(50) / 50 on the final layout,
  repulsion_ms      the repulsion launch alone (fr_op_tsne_repulsion; 20 back-to-back launches per timing),
  pairs_per_s       N^2 / repulsion_ms,
and, where sklearn imports (and --sklearn-max-n allows), sklearn_fit_s: sklearn.manifold.TSNE's Barnes-Hut run with
the same arguments on the same rows and this host's CPUs, once, for context.
Reads nothing outside the repository.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rows(n, dim, seed):
    """Unit rows around n / 20 planted unit centres (noise 0.6 / sqrt(dim) per component)."""
    rng = np.random.RandomState(seed)
    c = rng.standard_normal((max(n // 20, 1), dim))
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    x = c[np.arange(n) % len(c)] + 0.6 * rng.standard_normal((n, dim)) / np.sqrt(dim)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def event_ms(fn, runs):
    import torch
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), [round(min(ms), 4), round(max(ms), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[2000, 46715])
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--perplexity", type=float, default=30.0)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--sklearn-max-n", type=int, default=46715, help="largest N sklearn is timed at (0: never)")
    a = ap.parse_args()

    import torch

    from facerecognition_amd import _native as NL
    from facerecognition_amd.tsne import TSNE

    if not torch.cuda.is_available():
        raise SystemExit("tsne_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    L, st = NL.lib(), NL.stream_ptr(dev)
    for n in a.n:
        x = rows(n, a.dim, n)
        kw = dict(n_components=2, perplexity=a.perplexity, max_iter=a.iters, init="pca", random_state=42)
        t = TSNE(**kw)
        t.fit(x)  # warm-up
        fit_ms, fit_spread = event_ms(lambda: t.fit(x), a.runs)
        y = torch.from_numpy(t.embedding_).to(dev)
        aff_ms, _ = event_ms(lambda: t._affinities(x, dev), 1)
        (indptr, col, val), _ = t._affinities(x, dev)
        gws = int(L.fr_tsne_gradient_workspace(n))
        ws = torch.empty((gws,), dtype=torch.uint8, device=dev)
        grad = torch.empty((n, 2), dtype=torch.float32, device=dev)
        stats = torch.empty((3,), dtype=torch.float64, device=dev)
        upd, gains = torch.zeros_like(y), torch.ones_like(y)
        ycopy = y.clone()

        def run50():
            NL.check(L.fr_tsne_run(NL.ptr(indptr), NL.ptr(col), NL.ptr(val), n, NL.ptr(ycopy), NL.ptr(upd),
                                   NL.ptr(gains), 1.0, 0.8, float(t.learning_rate_), 50, NL.ptr(grad), NL.ptr(stats),
                                   NL.ptr(ws), gws, st), "fr_tsne_run")

        run50()
        step_ms, step_spread = event_ms(run50, a.runs)
        def rep20():
            for _ in range(20):
                NL.check(L.fr_op_tsne_repulsion(NL.ptr(y), n, NL.ptr(ws), gws, st), "fr_op_tsne_repulsion")

        rep20()
        rep_ms, rep_spread = event_ms(rep20, a.runs)
        out = {"N": n, "D": a.dim, "perplexity": a.perplexity, "iters": a.iters, "n_iter_": t.n_iter_,
               "kl_divergence": round(t.kl_divergence_, 4), "nnz": int(indptr[n].item()),
               "fit_ms": round(fit_ms, 2), "fit_ms_min_max": fit_spread, "affinities_ms": round(aff_ms, 2),
               "step_ms": round(step_ms / 50, 5), "step_ms_min_max": [round(s / 50, 5) for s in step_spread],
               "repulsion_ms": round(rep_ms / 20, 5), "repulsion_ms_min_max": [round(s / 20, 5) for s in rep_spread],
               "pairs_per_s": round(float(n) * n / (rep_ms / 20 * 1e-3), 0),
               "device": torch.cuda.get_device_name(dev)}
        if a.sklearn_max_n >= n:
            try:
                from sklearn.manifold import TSNE as SkTSNE
            except ImportError:
                SkTSNE = None
            if SkTSNE is not None:
                t0 = time.perf_counter()
                sk = SkTSNE(**kw).fit(x)
                out["sklearn_fit_s"] = round(time.perf_counter() - t0, 2)
                out["sklearn_kl_divergence"] = round(float(sk.kl_divergence_), 4)
                out["host_cpus"] = len(os.sched_getaffinity(0))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
