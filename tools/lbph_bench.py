#!/usr/bin/env python3
"""Time the two LBPH kernels (DESIGN.md §4 LBPH):

  fr_lbph_hist   B = 256 gray 100x100 images, OpenCV defaults (radius 1, 8 neighbours, 8x8 grid)
                 -> achieved bytes/s, counting the image bytes read plus the u16 counts written
  fr_lbph_match  256 probes x 10000 gallery rows, D = 16384, k = 1 (incl. the merge launch)
                 -> elements/s, one element = one (probe, row, bin)

The images are box-blurred device noise; the gallery rows are their histograms, so the counts have a face
histogram's sparsity.  Device times come from events on the launching stream around ``--iters`` back-to-back
calls after a warm-up, ``--rounds`` rounds (median reported, min / max as the spread).  One JSON line per kernel.
Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def images(n, H, W, seed, dev):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.rand((n, 1, H + 4, W + 4), generator=g, device=dev)
    x = torch.nn.functional.avg_pool2d(torch.nn.functional.avg_pool2d(x, 3, 1), 3, 1)[:, 0]
    lo, hi = x.amin((1, 2), keepdim=True), x.amax((1, 2), keepdim=True)
    return ((x - lo) / (hi - lo) * 255).round().to(torch.uint8).contiguous()


def timed(fn, iters, rounds):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return float(np.median(ms)), [round(min(ms), 4), round(max(ms), 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--size", type=int, default=100)
    ap.add_argument("--k", type=int, default=1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()

    import torch

    from facerecognition_amd import _native as NL
    from facerecognition_amd.lbph import lbph_hist, lbph_match

    if not torch.cuda.is_available():
        raise SystemExit("lbph_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    L, st = NL.lib(), NL.stream_ptr(dev)
    B, n, S, k = a.batch, a.rows, a.size, a.k
    D, P = 8 * 8 * 256, ((S - 2) // 8) ** 2
    name = torch.cuda.get_device_name(dev)

    x = images(B, S, S, 0, dev)
    counts = torch.empty((B, D), dtype=torch.int16, device=dev)

    def run_hist():
        NL.check(L.fr_lbph_hist(NL.ptr(x), B, S, S, 1, 8, 8, 8, NL.ptr(counts), st), "fr_lbph_hist")

    ms, spread = timed(run_hist, a.iters * 10, a.rounds)
    nbytes = B * S * S + B * D * 2
    print(json.dumps({"kernel": "lbph_hist", "B": B, "H": S, "W": S, "D": D, "ms": round(ms, 4), "ms_min_max": spread,
                      "bytes": nbytes, "gbytes_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                      "pixel_neighbour_samples_per_s": round(B * (S - 2) ** 2 * 8 / (ms * 1e-3), 0),
                      "device": name}), flush=True)

    gal = torch.cat([lbph_hist(images(min(2000, n - s), S, S, 1 + s, dev)) for s in range(0, n, 2000)])
    q = lbph_hist(x)
    nws = int(L.fr_lbph_match_workspace(B, n, D, k))
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev)
    dist = torch.empty((B, k), dtype=torch.float64, device=dev)
    idx = torch.empty((B, k), dtype=torch.int32, device=dev)

    def run_match():
        NL.check(L.fr_lbph_match(NL.ptr(q), B, NL.ptr(gal), n, D, P, k, NL.ptr(dist), NL.ptr(idx), NL.ptr(ws), nws, st),
                 "fr_lbph_match")

    ms, spread = timed(run_match, a.iters, a.rounds)
    d2, i2 = lbph_match(q[:1], gal, P, k)  # the result is what one probe alone gives, bitwise
    assert torch.equal(d2[0], dist[0]) and torch.equal(i2[0], idx[0])
    elems = float(B) * n * D
    print(json.dumps({"kernel": "lbph_match", "B": B, "N": n, "D": D, "k": k, "ms": round(ms, 4), "ms_min_max": spread,
                      "elements": elems, "gelements_per_s": round(elems / (ms * 1e-3) / 1e9, 1),
                      "gallery_bytes": n * D * 2, "workspace_bytes": nws, "device": name}), flush=True)


if __name__ == "__main__":
    main()
