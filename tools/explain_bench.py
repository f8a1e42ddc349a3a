#!/usr/bin/env python3
"""Device time of fr_explain minus fr_embed (the cost of an explanation on top of its forward).

Per batch size: both calls warmed (tuning pass, graph capture), then timed alternately with device events on
the launching stream, fixed buffers; the median of each and their difference.  Beside it the bytes the explain
launches need: the head's weight image once per tile of 8 images (the head-gradient pass), the explained
tensor, the gradient written and read back, the map written, read and rewritten.

    python tools/explain_bench.py [--arch iresnet100] [--dtype bf16] [--batches 1,256] [--iters 30]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="iresnet100")
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--batches", default="1,256")
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    import torch

    from facerecognition_amd import _native as N
    from facerecognition_amd.model import FRModel
    from facerecognition_amd.synthetic import synthetic_crops
    from facerecognition_amd.weights import INPUT_SIZE

    if not torch.cuda.is_available():
        raise SystemExit("explain_bench: needs the GPU (no CPU timing is meaningful)")
    batches = [int(b) for b in a.batches.split(",")]
    S = INPUT_SIZE[a.arch]
    m = FRModel.synthetic(a.arch, dtype=a.dtype, max_batch=max(batches))
    L, s = N.lib(), N.stream_ptr()
    h, w, C = m.explain_shape()
    D = m.embedding_size
    K = C if a.arch == "resnet50_arcface" else h * w * C
    for B in batches:
        u8 = torch.from_numpy(synthetic_crops(min(B, 16), S, seed=0)).repeat((B + 15) // 16, 1, 1, 1)[:B].cuda().contiguous()
        emb = torch.empty((B, D), dtype=torch.float32, device="cuda")
        cam = torch.empty((B, S, S), dtype=torch.float32, device="cuda")

        def embed():
            N.check(L.fr_embed(m.handle, u8.data_ptr(), 0, B, S, S, emb.data_ptr(), N.FR_EMBED_RAW, s), "fr_embed")

        def explain():
            N.check(L.fr_explain(m.handle, u8.data_ptr(), 0, B, S, S, None, cam.data_ptr(), None, emb.data_ptr(), s),
                    "fr_explain")

        for _ in range(4):
            embed()
            explain()
        torch.cuda.synchronize()
        t = {"embed": [], "explain": []}
        for _ in range(a.iters):
            for name, fn in (("embed", embed), ("explain", explain)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                t[name].append(e0.elapsed_time(e1))
        med = {k: statistics.median(v) for k, v in t.items()}
        tiles = (B + 7) // 8
        by = {"head_w": tiles * D * K * 2 if a.arch != "irv1_facenet" else 0, "act": B * h * w * C * 2,
              "grad": 2 * B * K * 4 if a.arch != "irv1_facenet" else 0, "map": 3 * B * S * S * 4}
        print(json.dumps({"arch": a.arch, "dtype": a.dtype, "B": B, "embed_ms": round(med["embed"], 4),
                          "explain_ms": round(med["explain"], 4), "extra_ms": round(med["explain"] - med["embed"], 4),
                          "embed_min_ms": round(min(t["embed"]), 4), "explain_min_ms": round(min(t["explain"]), 4),
                          "image_tiles": tiles, "bytes": by, "bytes_total": sum(by.values())}))
    m.close()


if __name__ == "__main__":
    main()
