#!/usr/bin/env python3
"""Time the labelled-evaluation pass (fr_match_eval: true score + rank + 512-bin impostor histogram, no
top-k) against fr_match_topk(k = 5) on the same gallery, and evaluate_closed_set end to end.

Shapes: 2048 probes and the reference notebook's 20387 probes against 9343 prototypes, D = 512.
Device times come from events on the launching stream around ``--iters`` back-to-back calls, the two
entry points alternating in ``--rounds`` rounds (median over rounds reported, with min / max); the
end-to-end figure is a host clock around evaluate_closed_set (numpy in, report out), ending after the
results are on the host.  One JSON line per shape.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make(B, N, D, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((N, D)).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    true = rng.integers(0, N, B)
    # true score 1 / sqrt(1 + 512 sigma^2): 0.83 down to 0.15, the low end below the best impostor (~0.17)
    sigma = rng.uniform(0.03, 0.3, (B, 1)).astype(np.float32)
    P = G[true] + sigma * rng.standard_normal((B, D)).astype(np.float32)
    P /= np.linalg.norm(P, axis=1, keepdims=True)
    return G, P.astype(np.float32), true.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2048x9343,20387x9343")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bins", type=int, default=512)
    ap.add_argument("--no-e2e", action="store_true")
    a = ap.parse_args()

    import torch

    from facerecognition_amd import evaluate_closed_set
    from facerecognition_amd.gallery import DeviceGallery

    if not torch.cuda.is_available():
        raise SystemExit("eval_timing: needs a GPU")
    for shape in a.shapes.split(","):
        B, N = (int(v) for v in shape.split("x"))
        G, P, true = make(B, N, 512, 3)
        gal = DeviceGallery(G)
        p = torch.from_numpy(P).to(gal.device)
        t = torch.from_numpy(true).to(gal.device)
        s = torch.empty((B, 5), dtype=torch.float32, device=gal.device)
        i = torch.empty((B, 5), dtype=torch.int32, device=gal.device)
        hist = torch.zeros((a.bins,), dtype=torch.int64, device=gal.device)

        def run_eval():
            gal.evaluate_device(p, t, 0, a.bins, (-1.0, 1.0), hist)

        def run_eval_nohist():
            gal.evaluate_device(p, t, 0, 0)

        def run_topk():
            gal.search_device(p, 5, s, i)

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.iters

        fns = {"eval_ms": run_eval, "eval_nohist_ms": run_eval_nohist, "topk5_ms": run_topk}
        for fn in fns.values():  # warm every shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                ms[k].append(timed(fn))
        row = {"B": B, "N": N, "D": 512, "bins": a.bins, "iters": a.iters, "rounds": a.rounds}
        for k, v in ms.items():
            row[k] = round(float(np.median(v)), 4)
            row[k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
        row["eval_over_topk5"] = round(row["eval_ms"] / row["topk5_ms"], 3)
        row["eval_nohist_over_topk5"] = round(row["eval_nohist_ms"] / row["topk5_ms"], 3)
        row["gflops_eval"] = round(2.0 * B * N * 512 / (row["eval_ms"] * 1e-3) / 1e9, 1)
        if not a.no_e2e:
            e2e = []
            for _ in range(3):
                t0 = time.perf_counter()
                rep = evaluate_closed_set(gal, P, true, hist_bins=a.bins)
                e2e.append((time.perf_counter() - t0) * 1e3)
            row["closed_set_e2e_ms"] = round(float(np.median(e2e)), 2)
            row["closed_set_e2e_ms_all"] = [round(v, 2) for v in e2e]
            row["top1_acc"], row["top5_acc"] = rep["top1_acc"], rep["top5_acc"]
            row["auc"], row["eer"] = round(rep["roc"]["auc"], 4), round(float(rep["roc"]["eer"]), 4)
            row["score_matrix_bytes_avoided"] = 4 * B * N
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
