#!/usr/bin/env python3
"""Time one training step (forward + backward) of the fused embedding head (DESIGN.md §4 "Head training") against the
same step in unfused torch-ROCm ops (BatchNorm, dropout, linear, BatchNorm, autograd) on the same GPU, at the three
models' head shapes (B, K, N) = (256, 2048, 512), (256, 1792, 512) and (256, 25088, 512).

Per shape one JSON line with the step time of
  fused        fr_head_forward + fr_head_backward on preallocated buffers, every parameter gradient, dX NULL (the
               frozen trunk), and fused_dx the same with dX
  unfused      the torch modules in training mode, loss = (y * dY).sum(), autograd for the parameters only, and
               unfused_dx the same with the input requiring a gradient
hipEvent-timed on the launching stream; the sides alternate run by run after 10 warm-ups each, median of --runs.
step_gflop is the three products' 3 x 2 B K N (two without dX).  Reads nothing outside the repository.  Needs a GPU:
there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (B, K, N): (S, input BN and bias, p)
HEADS = {(256, 2048, 512): (1, True, 0.5), (256, 1792, 512): (1, False, 0.6), (256, 25088, 512): (49, True, 0.0)}


def alternate_ms(fns, runs, warm=10):
    """Median and (min, max) ms of each callable, run in turn."""
    import torch
    for fn in fns:
        for _ in range(warm):
            fn()
    ms = [[] for _ in fns]
    for _ in range(runs):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[i].append(e0.elapsed_time(e1))
    return [(round(float(np.median(m)), 4), [round(min(m), 4), round(max(m), 4)]) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, nargs="+", default=["256,2048,512", "256,1792,512", "256,25088,512"])
    ap.add_argument("--runs", type=int, default=50)
    a = ap.parse_args()

    import torch
    from torch import nn

    from facerecognition_amd import _native as NL

    if not torch.cuda.is_available():
        raise SystemExit("head_train_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    L, st = NL.lib(), NL.stream_ptr(dev)
    for shape in a.shapes:
        B, K, N = (int(v) for v in shape.split(","))
        S, full, p = HEADS.get((B, K, N), (1, True, 0.5))
        Cin = K // S
        g = torch.Generator(device=dev).manual_seed(K)
        new = lambda *s: torch.empty(s, device=dev)
        x = torch.randn((B, K), device=dev, generator=g).relu_()
        dY = torch.randn((B, N), device=dev, generator=g)
        w = torch.randn((N, K), device=dev, generator=g) * (2.0 / (K + N)) ** 0.5
        bias = torch.zeros(N, device=dev) if full else None
        g1, b1, rm1, rv1 = (torch.ones(Cin, device=dev), torch.zeros(Cin, device=dev), torch.zeros(Cin, device=dev),
                            torch.ones(Cin, device=dev)) if full else (None,) * 4
        g2, b2, rm2, rv2 = torch.ones(N, device=dev), torch.zeros(N, device=dev), torch.zeros(N, device=dev), torch.ones(N, device=dev)
        nbytes = int(L.fr_head_workspace(B, K, N))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        Y, Z, mean2, rstd2 = new(B, N), new(B, N), new(N), new(N)
        mean1, rstd1 = (new(Cin), new(Cin)) if full else (None, None)
        dX, dW, dbias = new(B, K), new(N, K), new(N) if full else None
        dg1, db1 = (new(Cin), new(Cin)) if full else (None, None)
        dg2, db2 = new(N), new(N)
        P = NL.ptr
        step = [0]

        def fused(dx):
            step[0] += 1
            NL.check(L.fr_head_forward(P(x), B, K, S, P(w), N, P(bias), P(g1), P(b1), P(rm1), P(rv1), P(g2), P(b2), P(rm2),
                                       P(rv2), 3, p, 1e-5, 0.1, 1, step[0], P(Y), P(Z), P(mean1), P(rstd1), P(mean2),
                                       P(rstd2), None, P(ws), nbytes, st), "fr_head_forward")
            NL.check(L.fr_head_backward(P(x), B, K, S, P(w), N, P(g1), P(b1), P(g2), 3, p, 1, step[0], P(mean1), P(rstd1),
                                        P(mean2), P(rstd2), P(Z), P(dY), P(dX) if dx else None, P(dW), P(dbias), P(dg1),
                                        P(db1), P(dg2), P(db2), P(ws), nbytes, st), "fr_head_backward")

        side = int(round(S ** 0.5))
        bn1 = (nn.BatchNorm2d(Cin) if S > 1 else nn.BatchNorm1d(Cin)).to(dev) if full else None
        drop, fc, bn2 = nn.Dropout(p), nn.Linear(K, N, bias=full).to(dev), nn.BatchNorm1d(N).to(dev)
        with torch.no_grad():
            fc.weight.copy_(w)
            if full:
                fc.bias.zero_()
        mods = [m for m in (bn1, fc, bn2) if m is not None]
        xg = x.clone().requires_grad_(True)

        def unfused(dx):
            for m in mods:
                for prm in m.parameters():
                    prm.grad = None
            xi = xg if dx else x
            xg.grad = None
            h = xi
            if bn1 is not None:
                h = bn1(xi.view(B, Cin, side, side)).flatten(1) if S > 1 else bn1(xi)
            y = bn2(fc(drop(h) if p > 0 else h))
            (y * dY).sum().backward()

        fused(True)
        unfused(True)
        torch.cuda.synchronize()
        y_ref = bn2(fc(bn1(x.view(B, Cin, side, side)).flatten(1) if S > 1 else (bn1(x) if full else x))) if p == 0 else None
        (f, fs), (u, us), (fd, fds), (ud, uds) = alternate_ms(
            [lambda: fused(False), lambda: unfused(False), lambda: fused(True), lambda: unfused(True)], a.runs)
        out = {"B": B, "K": K, "N": N, "S": S, "input_bn": full, "p": p, "runs": a.runs, "workspace_bytes": nbytes,
               "fused_step_ms": f, "fused_step_ms_min_max": fs, "unfused_step_ms": u, "unfused_step_ms_min_max": us,
               "fused_dx_step_ms": fd, "fused_dx_step_ms_min_max": fds, "unfused_dx_step_ms": ud,
               "unfused_dx_step_ms_min_max": uds, "step_gflop": round(2 * 2.0 * B * K * N / 1e9, 2),
               "step_dx_gflop": round(3 * 2.0 * B * K * N / 1e9, 2), "device": torch.cuda.get_device_name(dev)}
        if y_ref is not None:  # without dropout the two sides compute the same Y (a sanity check, not a test)
            fused(False)
            out["y_max_abs_diff"] = float((Y - y_ref.detach()).abs().max())
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
