#!/usr/bin/env python3
"""Time one fused clip + step (facerecognition_amd.optim) against ``clip_grad_norm_`` + ``torch.optim`` on the same GPU.

Two tensor lists, the parameters a freeze_ratio 0.8 fine-tune trains: ResNet-50 layer4 + the embedding head + C class
centres of 512 floats, C = 9343 and C = 10^6.  Two optimisers: SGD with momentum (0.9, weight decay 5e-4) and AdamW,
both clipping at 5.0.  Three sides on the same parameters and gradients: the fused step, ``clip_grad_norm_`` +
``torch.optim`` in its default (foreach) mode, and the same with ``fused=True``.  Each side is timed with device events
on the launching stream around one clip + step, the sides alternating, ``--runs`` times after ``--warmup`` untimed
rounds; the median and the extremes are reported.  One JSON line per (list, optimiser) with
  elements, tensors   of the list,
  bytes_model         what one norm pass and one update pass must move: 4 (g) + 12 (p, g, buf) + 8 (p, buf) = 24 B per
                      element for SGD with momentum, 4 + 16 (p, g, m, v) + 12 (p, m, v) = 32 B for AdamW,
  *_ms                median time of one clip + step, *_ms_min_max its extremes,
  fused_gbps          bytes_model / fused_ms, next to the part's streaming rate (about 6 TB/s measured by others; not
                      measured here).
A machine without a GPU is an error: there is nothing to measure."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tensor_list(classes, dev):
    """Parameters of layer4 + head + class centres (values do not matter to the timing; shapes and layouts do)."""
    import torch

    from facerecognition_amd.backbone_train import ResNet50Layer4
    from facerecognition_amd.head import EmbeddingHead

    mods = [ResNet50Layer4().to(dev), EmbeddingHead.for_arch("resnet50_arcface").to(dev)]
    params = [p.detach().clone().requires_grad_(True) for m in mods for p in m.parameters()]
    params.append((torch.randn(classes, 512, device=dev) * 0.01).requires_grad_(True))
    return params


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--classes", type=int, nargs="+", default=[9343, 1000000])
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.jsonl"))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench: no GPU; nothing to measure")
    from facerecognition_amd import optim as O

    dev = torch.device("cuda", 0)
    cases = [("sgd_momentum", 24, O.SGD, torch.optim.SGD, dict(lr=1e-4, momentum=0.9, weight_decay=5e-4)),
             ("adamw", 32, O.AdamW, torch.optim.AdamW, dict(lr=1e-5, weight_decay=1e-2))]
    lines = []
    for classes in a.classes:
        params = tensor_list(classes, dev)
        n = sum(p.numel() for p in params)
        g = torch.Generator(device=dev).manual_seed(1)
        for p in params:
            p.grad = torch.randn(p.shape, device=dev, generator=g).to(memory_format=torch.preserve_format)
            if p.grad.stride() != p.stride():
                p.grad = torch.empty_like(p).copy_(p.grad)
        for name, bytes_per, mine, theirs, kw in cases:
            ours = mine(params, max_norm=5.0, **kw)
            foreach = theirs(params, foreach=True, **kw)
            fused = theirs(params, fused=True, **kw)

            def torch_side(opt):
                def run():
                    torch.nn.utils.clip_grad_norm_(params, 5.0)
                    opt.step()
                return run

            sides = {"fused": ours.step, "torch_foreach": torch_side(foreach), "torch_fused": torch_side(fused)}
            times = {k: [] for k in sides}
            for r in range(a.warmup + a.runs):
                for k, fn in sides.items():  # alternating sides
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    if r >= a.warmup:
                        times[k].append(e0.elapsed_time(e1))
            line = dict(what="clip + step", optimizer=name, classes=classes, tensors=len(params), elements=n,
                        bytes_per_element=bytes_per, bytes_model=n * bytes_per, runs=a.runs,
                        device=torch.cuda.get_device_name(0))
            for k, v in times.items():
                line[f"{k}_ms"] = round(statistics.median(v), 4)
                line[f"{k}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
            line["fused_gbps"] = round(n * bytes_per / (line["fused_ms"] * 1e-3) / 1e9, 1)
            line["ratio_fused_over_torch_foreach"] = round(line["fused_ms"] / line["torch_foreach_ms"], 3)
            line["ratio_fused_over_torch_fused"] = round(line["fused_ms"] / line["torch_fused_ms"], 3)
            print(json.dumps(line), flush=True)
            lines.append(line)
            del ours, foreach, fused, sides
            torch.cuda.empty_cache()
        del params
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
