#!/usr/bin/env python3
"""DeviceMTCNN.detect_batch (the box logic on the device, one pass over a batch of frames) against the parent path,
DeviceMTCNN.detect_face called frame by frame with its host box logic, as FaceDetector.detect / the engine call it.

Frames: tools/mtcnn_bench.py's smooth 1080p frame() with distinct seeds, the calibrated synthetic weights
(trained-detector box volumes).  Batch sizes 1 and 16.  Both sides take host (numpy) frames, so each includes its
upload; each timed call ends in a device synchronise; the two sides alternate call by call and the median over the
calls is reported, per frame.  The results of the two sides are compared first (they must be equal).

    python tools/detect_batch_bench.py [--iters 15] [--out profiles/detect_batch.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def clock(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def main():
    from facerecognition_amd import face_detector as FD
    from mtcnn_bench import frame
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("detect_batch_bench needs the GPU: a CPU run measures nothing")
    dev = FD.DeviceMTCNN(FD.synth_mtcnn_state(7, calibrated=True), device=0)
    all_frames = np.stack([frame(seed=s) for s in range(max(a.batches))])
    res = {"frame": "1920x1080 synthetic RGB u8, seeds 0..B-1", "weights": "synth_mtcnn_state(7, calibrated=True)",
           "pyramid_levels": len(FD.pyramid_scales(1080, 1920)), "iters": a.iters, "capacity": dev.capacity,
           "timing": "host clock around a call on host frames ending in torch.cuda.synchronize(); sides alternate; "
                     "median over iters", "batches": {}}
    for B in a.batches:
        frames = all_frames[:B]

        def parent():
            return [tuple(r[0] for r in dev.detect_face(f[None])) for f in frames]

        def batched():
            return dev.detect_batch(frames)

        for _ in range(2):  # warm every shape of both sides
            ref = parent()
            gb, gp = batched()
        equal = all(np.array_equal(gb[b], ref[b][0]) and np.array_equal(gp[b], ref[b][1]) for b in range(B))
        FD.STATS = {}
        batched()
        st = dict(FD.STATS)
        FD.STATS = {}
        parent()
        sp = dict(FD.STATS)
        FD.STATS = None
        tp, tb = [], []
        for _ in range(a.iters):
            tp.append(clock(parent)[0])
            tb.append(clock(batched)[0])
        r = {"parent_ms_per_frame": round(float(np.median(tp)) / B, 3),
             "detect_batch_ms_per_frame": round(float(np.median(tb)) / B, 3),
             "parent_ms_per_frame_min_max": [round(min(tp) / B, 3), round(max(tp) / B, 3)],
             "detect_batch_ms_per_frame_min_max": [round(min(tb) / B, 3), round(max(tb) / B, 3)],
             "speedup": round(float(np.median(tp) / np.median(tb)), 2), "results_equal": bool(equal),
             "faces": [int(len(x)) for x in gb],
             "detect_batch": {"readbacks_per_call": st.get("readback_n"), "device_fallbacks": st.get("device_fallback_n", 0),
                              "pnet_candidates": st.get("pnet_pass_n"), "rnet_inputs": st.get("rnet_ms_n"),
                              "onet_inputs": st.get("onet_ms_n"), "min_nms_inputs": st.get("nms_ms_n"),
                              "final": st.get("final_n"),
                              "host_ms_to_readback": {k: round(st.get(k + "_ms", 0.0), 3) for k in ("pnet", "rnet", "onet")}},
             "parent": {"pnet_levels_read_back": res["pyramid_levels"] * B, "pnet_candidates": sp.get("pnet_pass_n"),
                        "rnet_inputs": sp.get("rnet_ms_n"), "onet_inputs": sp.get("onet_ms_n"),
                        "host_nms_calls_boxes": sp.get("nms_ms_n"), "final": sp.get("final_n")}}
        print(f"B={B}:", json.dumps(r), flush=True)
        if not equal:
            raise SystemExit(f"B={B}: detect_batch and detect_face disagree")
        res["batches"][str(B)] = r
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
