#!/usr/bin/env python3
"""Time one training step (forward + backward) of ResNet50Layer4 (DESIGN.md §4 "Backbone training: layer4") against the
same three Bottlenecks in torch-ROCm's own float32 ops (nn.Conv2d on channels_last tensors, nn.BatchNorm2d in training
mode, ReLU, autograd) on the same GPU, at B = 256 and B = 32, and each of layer4's six convolution shapes on its own.

Per batch size one JSON line with the step time of both sides (every parameter gradient, no input gradient: the trunk
is frozen), then one line per convolution shape with the device's forward, data-gradient and weight-gradient calls and
torch's forward and backward (both gradients).  hipEvent-timed on the launching stream; the sides alternate run by run
after 10 warm-ups each, median of --runs.  The device side is exact float32 on v_mfma_f32_16x16x4f32, which runs at 1/16
of the bf16 MFMA rate; torch's side is whatever MIOpen picks for float32.  Reads nothing outside the repository.  Needs a
GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, H, Cin, Cout, k, stride, transform): layer4's distinct convolutions
CONVS = [("0.conv1", 7, 1024, 512, 1, 1, False), ("0.conv2", 7, 512, 512, 3, 2, True), ("x.conv3", 4, 512, 2048, 1, 1, True),
         ("0.downsample", 7, 1024, 2048, 1, 2, False), ("1.conv1", 4, 2048, 512, 1, 1, False), ("1.conv2", 4, 512, 512, 3, 1, True)]


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
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 32])
    ap.add_argument("--runs", type=int, default=30)
    a = ap.parse_args()

    import torch
    from torch import nn

    from facerecognition_amd import backbone_train as BT

    if not torch.cuda.is_available():
        raise SystemExit("layer4_train_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    name = torch.cuda.get_device_name(dev)

    class TorchBottleneck(nn.Module):
        def __init__(self, cin, p, stride, down):
            super().__init__()
            self.c1, self.b1 = nn.Conv2d(cin, p, 1, bias=False), nn.BatchNorm2d(p)
            self.c2, self.b2 = nn.Conv2d(p, p, 3, stride, 1, bias=False), nn.BatchNorm2d(p)
            self.c3, self.b3 = nn.Conv2d(p, 4 * p, 1, bias=False), nn.BatchNorm2d(4 * p)
            self.ds = nn.Sequential(nn.Conv2d(cin, 4 * p, 1, stride, bias=False), nn.BatchNorm2d(4 * p)) if down else None

        def forward(self, x):
            h = torch.relu(self.b1(self.c1(x)))
            h = torch.relu(self.b2(self.c2(h)))
            h = self.b3(self.c3(h))
            return torch.relu(h + (x if self.ds is None else self.ds(x)))

    for B in a.batches:
        g = torch.Generator(device=dev).manual_seed(B)
        feat = torch.randn((B, 7, 7, 1024), device=dev, generator=g).relu_()
        dY = torch.randn((B, 2048), device=dev, generator=g)
        mine = BT.ResNet50Layer4().to(dev).train()
        ref = nn.Sequential(TorchBottleneck(1024, 512, 2, True), TorchBottleneck(2048, 512, 1, False),
                            TorchBottleneck(2048, 512, 1, False)).to(dev).to(memory_format=torch.channels_last).train()
        x_nchw = feat.permute(0, 3, 1, 2)  # the same memory, NCHW-shaped and channels_last

        def step_mine():
            for prm in mine.parameters():
                prm.grad = None
            mine(feat).backward(dY)

        def step_ref():
            for prm in ref.parameters():
                prm.grad = None
            ref(x_nchw).mean(dim=(2, 3)).backward(dY)

        (m, ms), (r, rs) = alternate_ms([step_mine, step_ref], a.runs)
        print(json.dumps({"what": "layer4 step", "B": B, "runs": a.runs, "device_step_ms": m, "device_step_ms_min_max": ms,
                          "torch_step_ms": r, "torch_step_ms_min_max": rs, "ratio_device_over_torch": round(m / r, 3),
                          "forward_gflop": round(0.51 * B, 1), "device": name}), flush=True)
        del mine, ref

        for cname, H, Cin, Cout, k, stride, tr in CONVS:
            x = torch.randn((B, H, H, Cin), device=dev, generator=g)
            w = torch.randn((Cout, k, k, Cin), device=dev, generator=g) * (2.0 / (k * k * Cin)) ** 0.5
            sc, sh = (torch.rand(Cin, device=dev, generator=g) + 0.5, torch.randn(Cin, device=dev, generator=g)) if tr else (None, None)
            Z = BT.conv_forward(x, w, k, stride, sc, sh, tr)
            dZ = torch.randn(Z.shape, device=dev, generator=g)
            xt = x.permute(0, 3, 1, 2).detach().requires_grad_(True)
            wt = w.permute(0, 3, 1, 2).detach().requires_grad_(True)
            dZt = dZ.permute(0, 3, 1, 2)
            tfwd = lambda: torch.nn.functional.conv2d(xt, wt, None, stride, k // 2)

            def tboth():
                torch.autograd.grad(tfwd(), (xt, wt), dZt)

            res = alternate_ms([lambda: BT.conv_forward(x, w, k, stride, sc, sh, tr),
                                lambda: BT.conv_backward(x, w, k, stride, dZ, sc, sh, tr, True, False),
                                lambda: BT.conv_backward(x, w, k, stride, dZ, sc, sh, tr, False, True), tfwd, tboth], a.runs)
            Ho = Z.shape[1]
            print(json.dumps({"what": "conv", "conv": cname, "B": B, "H": H, "Cin": Cin, "Cout": Cout, "k": k, "stride": stride,
                              "gflop_each": round(2.0 * B * Ho * Ho * Cout * k * k * Cin / 1e9, 2),
                              "device_fwd_ms": res[0][0], "device_dA_ms": res[1][0], "device_dW_ms": res[2][0],
                              "torch_fwd_ms": res[3][0], "torch_fwd_bwd_ms": res[4][0], "device": name}), flush=True)


if __name__ == "__main__":
    main()
