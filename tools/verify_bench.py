#!/usr/bin/env python3
"""Time the all-pairs verification (DESIGN.md §4 "Verification") at (N, D) = (2000, 512), (20387, 512) and
(46715, 512): the reference's t-SNE sample size, the evaluation notebook's probe set and a full validation set.

Every shape runs in a child process of its own under a time limit (--limit seconds); after a child that fails or
runs out of time nothing more is started.  Per shape one JSON line, every device time hipEvent-timed on the launching
stream, the median of --runs after 3 warm-ups with [min, max]:
  accuracy_ms   fr_verify_pairs as compute_verification_accuracy calls it: 16 thresholds and the row outputs
                (every (i, j != i) is swept), on preallocated buffers
  report_ms     as verification_report's first pass: 2048-bin histograms and the row outputs
  counts_ms     16 thresholds and 2048-bin histograms, no row outputs (the upper triangle only): what the comparator
                below computes
  refine_ms     64 thresholds, nothing else (verification_report's second pass)
  torch_ms      THE COMPARATOR: our own restatement in torch ops on the same GPU of the counts_ms call: rows
                normalised, then per 1024-row chunk E[chunk] @ E.T, the genuine and impostor scores above the diagonal
                picked by mask, torch.histc of each and a compare-and-sum per threshold.  float32 matmul as torch runs
                it; same_counts / same_hist say whether its integers equal ours (they may differ where a score is within
                rounding of a threshold or edge).
  host_loop_ms  our restatement of the reference's 10 000-pair function (tests/verify_ref.py's
                verification_accuracy_sampled, numpy on the host, one run): what the reference spends per validation
plus flop (2 N^2 D for the full sweep) and the accuracies of both.  Reads nothing outside the repository.  Needs a GPU:
there is no fallback.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def event_ms(fn, runs, warm=3):
    import torch
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(float(np.median(ms)), 4), [round(min(ms), 4), round(max(ms), 4)]


def torch_counts(e, y, thr, nbins, chunk=1024):
    """counts [T, 2] and hist [2, nbins] over i < j from chunked E @ E.T, torch.histc and compare-and-sum."""
    import torch
    n = e.shape[0]
    en = e / (e.norm(dim=1, keepdim=True) + 1e-8)
    cols = torch.arange(n, device=e.device)
    counts = torch.zeros((thr.numel(), 2), dtype=torch.int64, device=e.device)
    hist = torch.zeros((2, nbins), dtype=torch.float64, device=e.device)
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        s = en[c0:c1] @ en.T
        up = cols[None, :] > cols[c0:c1, None]
        gen = y[c0:c1, None] == y[None, :]
        for k, m in enumerate((gen & up, ~gen & up)):
            v = s[m]
            hist[k] += torch.histc(v, bins=nbins, min=-1.0, max=1.0).double()
            for t0 in range(0, thr.numel(), 4):  # (four thresholds at a time bounds the comparison's temporary)
                counts[t0:t0 + 4, k] += (v[None, :] > thr[t0:t0 + 4, None]).sum(1)
    return counts, hist.long()


def one(N, D, runs):
    import torch

    from facerecognition_amd import _native as NL
    from facerecognition_amd import verification as V
    from tests import verify_ref as R

    if not torch.cuda.is_available():
        raise SystemExit("verify_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    L, st = NL.lib(), NL.stream_ptr(dev)
    per = 5  # rows per identity
    g = torch.Generator(device=dev).manual_seed(N)
    centres = torch.randn(((N + per - 1) // per, D), device=dev, generator=g)
    e = (centres.repeat_interleave(per, 0)[:N] + 1.2 * torch.randn((N, D), device=dev, generator=g)).contiguous()
    y = (torch.arange(N, device=dev) // per).to(torch.int32)
    nbytes = int(L.fr_verify_workspace(N, D))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    nb = 2048
    sweep = V.SWEEP.astype(np.float32)
    fine = np.linspace(0.2, 0.4, 64).astype(np.float32)
    counts = torch.zeros((64, 2), dtype=torch.int64, device=dev)
    totals = torch.zeros(2, dtype=torch.int64, device=dev)
    hist = torch.zeros((2, nb), dtype=torch.int64, device=dev)
    score = torch.empty((N, 3), device=dev)
    idx = torch.empty((N, 3), dtype=torch.int32, device=dev)
    rsum = torch.empty((N, 2), device=dev)

    def call(thr, with_hist, rows):
        NL.check(L.fr_verify_pairs(NL.ptr(e), N, D, NL.ptr(y), 1, thr.ctypes.data if thr.size else None, int(thr.size),
                                   NL.ptr(counts), NL.ptr(totals), NL.ptr(hist) if with_hist else None, nb, -1.0, 1.0,
                                   NL.ptr(score) if rows else None, NL.ptr(idx) if rows else None,
                                   NL.ptr(rsum) if rows else None, NL.ptr(ws), nbytes, st), "fr_verify_pairs")

    none = np.zeros(0, np.float32)
    acc_ms, acc_s = event_ms(lambda: call(sweep, False, True), runs)
    rep_ms, rep_s = event_ms(lambda: call(none, True, True), runs)
    ref_ms, ref_s = event_ms(lambda: call(fine, False, False), runs)
    cnt_ms, cnt_s = event_ms(lambda: call(sweep, True, False), runs)
    hist.zero_()
    call(sweep, True, False)
    torch.cuda.synchronize()
    ours_counts, ours_hist, ours_tot = counts[:16].cpu().numpy(), hist.cpu().numpy(), totals.cpu().numpy()
    acc = R.first_best(R.balanced_accuracy(ours_counts, ours_tot), V.SWEEP)

    thr_t = torch.from_numpy(sweep).to(dev)
    t_ms, t_s = event_ms(lambda: torch_counts(e, y, thr_t, nb), max(3, runs // 3), warm=1)
    tc, th = torch_counts(e, y, thr_t, nb)
    tc, th = tc.cpu().numpy(), th.cpu().numpy()

    eh, yh = e.cpu().numpy(), y.cpu().numpy()
    t0 = time.perf_counter()
    sampled = R.verification_accuracy_sampled(eh, yh, np.random.RandomState(0), num_pairs=10000)
    host_ms = 1e3 * (time.perf_counter() - t0)

    out = {"N": N, "D": D, "runs": runs, "pairs": N * (N - 1) // 2, "flop_full_sweep": 2.0 * N * N * D,
           "workspace_bytes": nbytes,
           "accuracy_ms": acc_ms, "accuracy_ms_min_max": acc_s, "report_ms": rep_ms, "report_ms_min_max": rep_s,
           "counts_ms": cnt_ms, "counts_ms_min_max": cnt_s, "refine_ms": ref_ms, "refine_ms_min_max": ref_s,
           "torch_ms": t_ms, "torch_ms_min_max": t_s, "host_loop_ms": round(host_ms, 1),
           "same_counts": bool(np.array_equal(tc, ours_counts)), "same_hist": bool(np.array_equal(th, ours_hist)),
           "counts_max_abs_diff": int(np.abs(tc - ours_counts).max()), "hist_moved": int(np.abs(th - ours_hist).sum() // 2),
           "accuracy_all_pairs": acc[0], "threshold_all_pairs": float(acc[1]), "accuracy_sampled": float(sampled[0]),
           "threshold_sampled": float(sampled[1]), "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, nargs="+", default=["2000,512", "20387,512", "46715,512"])
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--limit", type=int, default=240, help="seconds per shape")
    ap.add_argument("--one", type=str, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        N, D = (int(v) for v in a.one.split(","))
        one(N, D, a.runs)
        return
    for shape in a.shapes:
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", shape, "--runs", str(a.runs)],
                                timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            raise SystemExit(f"verify_bench: {shape} ran out of its {a.limit} s; nothing more is started")
        if rc != 0:
            raise SystemExit(f"verify_bench: {shape} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
