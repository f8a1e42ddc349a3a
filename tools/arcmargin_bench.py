#!/usr/bin/env python3
"""Time the fused ArcFace margin loss (DESIGN.md §4 "ArcFace margin loss") against the unfused formulation in
torch-ROCm ops on the same GPU, at (B, C, D) = (256, 9343, 512), the reference's evaluation shape, and
(256, 1000000, 512).

Per shape one JSON line with, for the fused path (fr_arcmargin_forward / fr_arcmargin_backward on preallocated
buffers, dE and dW both) and for the unfused one (F.normalize, F.linear, where, scatter, cross_entropy with label
smoothing, autograd: our own restatement of the reference module's forward),
  *_fwd_ms / *_bwd_ms   hipEvent-timed on the launching stream, median of --runs (>= 50) after 10 warm-ups, and
  *_peak_bytes          torch.cuda.max_memory_allocated over one forward + backward beyond the inputs E and W
plus loss_rel_diff, the relative difference of the two mean losses (a sanity check, not a test).
Reads nothing outside the repository.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCALE, MARGIN, LS = 64.0, 0.5, 0.1


def event_ms(fn, runs, warm=10):
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


def unfused_logits(e, w, y):
    """The reference module's forward, restated with torch ops."""
    import torch
    import torch.nn.functional as F
    cosine = F.linear(F.normalize(e), F.normalize(w))
    sine = torch.sqrt(torch.clamp(1.0 - cosine * cosine, min=1e-7))
    phi = cosine * math.cos(MARGIN) - sine * math.sin(MARGIN)
    phi = torch.where(cosine > math.cos(math.pi - MARGIN), phi, cosine - math.sin(math.pi - MARGIN) * MARGIN)
    one_hot = torch.zeros_like(cosine).scatter_(1, y.view(-1, 1), 1.0)
    return (one_hot * phi + (1.0 - one_hot) * cosine) * SCALE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, nargs="+", default=["256,9343,512", "256,1000000,512"])
    ap.add_argument("--runs", type=int, default=50)
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F

    from facerecognition_amd import _native as NL

    if not torch.cuda.is_available():
        raise SystemExit("arcmargin_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    L, st = NL.lib(), NL.stream_ptr(dev)
    for shape in a.shapes:
        B, C, D = (int(v) for v in shape.split(","))
        g = torch.Generator(device=dev).manual_seed(C)
        e = torch.randn((B, D), device=dev, generator=g)
        w = torch.randn((C, D), device=dev, generator=g) * math.sqrt(2.0 / (C + D))
        y = torch.randint(0, C, (B,), device=dev, generator=g)
        y32 = y.to(torch.int32)
        u = torch.full((B,), 1.0 / B, device=dev)
        torch.cuda.synchronize()

        def fused_peak_and_time():
            base = torch.cuda.memory_allocated(dev)
            torch.cuda.reset_peak_memory_stats(dev)
            nbytes = int(L.fr_arcmargin_workspace(B, C, D))
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
            loss, lse, inv_e = (torch.empty(B, device=dev) for _ in range(3))
            inv_w = torch.empty(C, device=dev)
            dE, dW = torch.empty_like(e), torch.empty_like(w)

            def fwd():
                NL.check(L.fr_arcmargin_forward(NL.ptr(e), B, D, NL.ptr(w), C, NL.ptr(y32), None, 1.0, SCALE, MARGIN, 0,
                                                LS, NL.ptr(loss), NL.ptr(lse), NL.ptr(inv_e), NL.ptr(inv_w), None,
                                                NL.ptr(ws), nbytes, st), "fr_arcmargin_forward")

            def bwd():
                NL.check(L.fr_arcmargin_backward(NL.ptr(e), B, D, NL.ptr(w), C, NL.ptr(y32), None, 1.0, SCALE, MARGIN,
                                                 0, LS, NL.ptr(lse), NL.ptr(inv_e), NL.ptr(inv_w), NL.ptr(u), None,
                                                 NL.ptr(dE), NL.ptr(dW), NL.ptr(ws), nbytes, st),
                         "fr_arcmargin_backward")

            fwd()
            bwd()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated(dev) - base
            f, fs = event_ms(fwd, a.runs)
            b, bs = event_ms(bwd, a.runs)
            return peak, f, fs, b, bs, float(loss.mean()), nbytes

        peak_f, ff, ffs, fb, fbs, loss_f, nbytes = fused_peak_and_time()

        eg, wg = e.clone().requires_grad_(True), w.clone().requires_grad_(True)

        def ufwd():
            return F.cross_entropy(unfused_logits(eg, wg, y), y, label_smoothing=LS)

        held = {}

        def ufwd_keep():
            held["loss"] = ufwd()

        def ubwd():
            eg.grad = wg.grad = None
            held["loss"].backward(retain_graph=True)

        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        ufwd_keep()
        ubwd()
        torch.cuda.synchronize()
        peak_u = torch.cuda.max_memory_allocated(dev) - base
        loss_u = float(held["loss"].detach())
        uf, ufs = event_ms(ufwd_keep, a.runs)
        ub, ubs = event_ms(ubwd, a.runs)
        held.clear()
        out = {"B": B, "C": C, "D": D, "runs": a.runs, "workspace_bytes": nbytes,
               "fused_fwd_ms": ff, "fused_fwd_ms_min_max": ffs, "fused_bwd_ms": fb, "fused_bwd_ms_min_max": fbs,
               "fused_peak_bytes": int(peak_f),
               "unfused_fwd_ms": uf, "unfused_fwd_ms_min_max": ufs, "unfused_bwd_ms": ub, "unfused_bwd_ms_min_max": ubs,
               "unfused_peak_bytes": int(peak_u), "loss_rel_diff": abs(loss_f - loss_u) / abs(loss_u),
               "pass_gflop": round(2.0 * B * C * D / 1e9, 2), "device": torch.cuda.get_device_name(dev)}
        print(json.dumps(out), flush=True)
        del eg, wg


if __name__ == "__main__":
    main()
