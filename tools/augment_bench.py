#!/usr/bin/env python3
"""Time the device augmentation (fr_augment) per preset at B = 256, S = 112 and S = 160.

For every preset one JSON line with
  device_ms     device time of one fr_augment call of the batch (device events around ``--steps`` calls after
                ``--warmup``; includes the staging copy of the op lists, not the host sampler),
  sample_ms     host time of ``DeviceTransform.sample`` for the batch (numpy, single thread),
  host_ms       the same programs on the same images through the Pillow / torch reference pipeline on this machine's
                host, single-threaded (measured on ``--host-images`` images and scaled to the batch), for scale,
  features_ms   one ``FRModel.features`` pass of the same batch on the model of that input size,
  ratio         device_ms / features_ms: whether augmentation can starve the trunk.
A machine without a GPU is an error: there is nothing to measure."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_ms(fn, warmup, steps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--sizes", type=int, nargs="+", default=[112, 160])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-images", type=int, default=32)
    ap.add_argument("--no-features", action="store_true")
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench: no GPU; nothing to measure")
    torch.set_num_threads(1)
    from facerecognition_amd import augment as A
    from facerecognition_amd.model import FRModel
    from facerecognition_amd.synthetic import synthetic_crops
    from tests import augment_pil as P

    B = a.batch
    for S in a.sizes:
        u8 = synthetic_crops(B, S, seed=0)
        x = torch.from_numpy(u8).cuda()
        feat_ms = None
        if not a.no_features:
            arch = "irv1_facenet" if S == 160 else "iresnet100"
            model = FRModel.synthetic(arch, max_batch=B)
            f32 = A.get_val_transforms(S)(x)
            feat_ms = device_ms(lambda: model.features(f32), 3, 10)
            del model
        presets = [(n, A.get_train_transforms(S, augment_strength=n)) for n in ("light", "normal", "strong", "heavy")]
        presets += [("facenet", A.facenet_train_transforms(S)), ("facenet_online", A.facenet_train_transforms(S, True)),
                    ("val", A.get_val_transforms(S))]
        for name, t in presets:
            t0 = time.perf_counter()
            ops, args = t.sample(B, np.random.default_rng(0))
            sample_ms = (time.perf_counter() - t0) * 1e3
            dev = device_ms(lambda: t.apply(x, ops, args), a.warmup, a.steps)
            n = min(a.host_images, B)
            t0 = time.perf_counter()
            for b in range(n):
                P.run_program(u8[b], ops[b], args[b])
            host_ms = (time.perf_counter() - t0) * 1e3 * B / n
            row = {"preset": name, "B": B, "S": S, "mean_ops": round(float((ops != 0).sum(1).mean()), 2),
                   "device_ms": round(dev, 4), "sample_ms": round(sample_ms, 2), "host_ms": round(host_ms, 1),
                   "features_ms": None if feat_ms is None else round(feat_ms, 3),
                   "ratio": None if feat_ms is None else round(dev / feat_ms, 4)}
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
