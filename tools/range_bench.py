#!/usr/bin/env python3
"""Time the two range-search passes (fr_match_range_count incl. its scan, fr_match_range_fill) against
fr_match_eval with k = 0 and no histogram -- the same main loop with a compare-and-count epilogue -- on the
same gallery.

Shape: the reference notebook's 20387 probes x 9343 prototypes, D = 512, eval_timing.py's L2-normalised
random rows with planted matches; thresh 0.5 (the reference's default: about one hit per matched probe) and
0.1 (about 2.3 sigma of an impostor score: millions of hits, the fill pass's stores at work).  Device times
come from events on the launching stream around ``--iters`` back-to-back calls, the three entry points
alternating in ``--rounds`` rounds (median over rounds reported, with min / max as the spread).  One JSON
line per shape and threshold.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from eval_timing import make  # noqa: E402  (tools/ is the script's directory)


def bench(gal, p, t, thresh, iters, rounds):
    import torch

    from facerecognition_amd import _native as NL

    L, dev, B = NL.lib(), gal.device, int(p.shape[0])
    st = NL.stream_ptr(dev)
    ws = torch.empty((L.fr_match_range_workspace(gal._h, B) // 4,), dtype=torch.int32, device=dev)
    lims = torch.empty((B + 1,), dtype=torch.int64, device=dev)

    def run_count():
        NL.check(L.fr_match_range_count(gal._h, NL.ptr(p), B, thresh, None, NL.ptr(ws), NL.ptr(lims), st),
                 "fr_match_range_count")

    run_count()
    total = int(lims[-1].item())
    s = torch.empty((max(total, 1),), dtype=torch.float32, device=dev)
    i = torch.empty((max(total, 1),), dtype=torch.int32, device=dev)

    def run_fill():  # ws / lims of the last count: the same arguments, so the same contents every time
        NL.check(L.fr_match_range_fill(gal._h, NL.ptr(p), B, thresh, None, NL.ptr(ws), NL.ptr(lims), NL.ptr(s),
                                       NL.ptr(i), total, st), "fr_match_range_fill")

    def run_eval():
        gal.evaluate_device(p, t, 0, 0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    fns = {"eval_nohist_ms": run_eval, "range_count_ms": run_count, "range_fill_ms": run_fill}
    for fn in fns.values():  # warm every entry point
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
    # the result is what the top-k path says it is: every kept score >= thresh, the best hit fr_match_topk's
    s1, _ = gal.search_device(p, 1)
    cnt = (lims[1:] - lims[:-1]).cpu().numpy()
    assert int(cnt.sum()) == total and bool((s[:total] >= thresh).all())
    assert np.array_equal(cnt > 0, (s1[:, 0] >= thresh).cpu().numpy())
    row = {"B": B, "N": gal.ntotal, "D": 512, "thresh": thresh, "iters": iters, "rounds": rounds, "hits": total,
           "probes_with_hits": int((cnt > 0).sum()), "n_split": int(L.fr_debug_match_range_splits(gal._h, B)),
           "device": torch.cuda.get_device_name(dev)}
    for k, v in ms.items():
        row[k] = round(float(np.median(v)), 4)
        row[k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
    row["count_over_eval"] = round(row["range_count_ms"] / row["eval_nohist_ms"], 3)
    row["fill_over_eval"] = round(row["range_fill_ms"] / row["eval_nohist_ms"], 3)
    row["gflops_count"] = round(2.0 * B * gal.ntotal * 512 / (row["range_count_ms"] * 1e-3) / 1e9, 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20387x9343")
    ap.add_argument("--thresh", default="0.5,0.1")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()

    import torch

    from facerecognition_amd.gallery import DeviceGallery

    if not torch.cuda.is_available():
        raise SystemExit("range_bench: needs a GPU")
    for shape in a.shapes.split(","):
        B, N = (int(v) for v in shape.split("x"))
        G, P, true = make(B, N, 512, 3)
        gal = DeviceGallery(G)
        p = torch.from_numpy(P).to(gal.device)
        t = torch.from_numpy(true).to(gal.device)
        for thresh in a.thresh.split(","):
            print(json.dumps(bench(gal, p, t, float(thresh), a.iters, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
