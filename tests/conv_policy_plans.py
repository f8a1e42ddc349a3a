"""The fixed conv policy as fr_debug_plan reports it: the plan text of a freshly loaded model, before any forward at
a batch size has measured anything (csrc/convs.cpp default_choice; the stage lines come from stages.cpp's fixed
rules).  No embed call is made, so only the load-time weight packers run on the device.

tests/test_gpu_conv_policy.py compares `plans(name)` with tests/golden/plans/<name>.json.  Run as a script this module
writes those files (they are recorded at the commit before a change to the conv selection, and then pin it):

    python -m tests.conv_policy_plans [output directory, default tests/golden/plans]

One file per model: {"B=<batch> invariant=<0|1>": [plan lines]}.  B = 1 and 8 reach fit_split's small-M splits, B = 256
the ROWS / IMG28 / BAND ranks of the policy, invariant = 1 the unsplit cost-model branch (refused on fp8 handles, so
those have the invariant = 0 plans only).

fr_debug_plan does not show the plan's tensors, so a second file per model, <name>_tensors.json, pins them:
{"tensors": [[name, H, W, C, dtype]]} in plan order, dtype the storage type ("bf16", "f16") that fr_debug_tensor_dtype
reports (a bf16 InceptionResnetV1 plan keeps a section in f16)."""
from __future__ import annotations

import ctypes
import json
import os
import sys

from facerecognition_amd import _native as N

# name -> (arch, dtype)
MODELS = {
    "iresnet100_bf16": ("iresnet100", "bf16"),
    "resnet50_arcface_bf16": ("resnet50_arcface", "bf16"),
    "irv1_facenet_bf16": ("irv1_facenet", "bf16"),
    "iresnet100_f16": ("iresnet100", "f16"),
    "iresnet100_fp8": ("iresnet100", "fp8"),
}
BATCHES = (1, 8, 256)
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plans")


def plan_lines(m, B):
    buf = ctypes.create_string_buffer(1 << 20)
    N.check(N.lib().fr_debug_plan(m.handle, B, buf, len(buf)), "fr_debug_plan")
    return buf.value.decode().splitlines()


def plans(name):
    from facerecognition_amd.model import FRModel
    arch, dtype = MODELS[name]
    m = FRModel.synthetic(arch, max_batch=256, dtype=dtype)
    out = {}
    try:
        for inv in (0, 1) if dtype != "fp8" else (0,):
            m.set_option(N.FR_OPT_BATCH_INVARIANT, inv)
            for B in BATCHES:
                out[f"B={B} invariant={inv}"] = plan_lines(m, B)
    finally:
        m.close()
    return out


def tensors(name):
    from facerecognition_amd.model import FRModel
    arch, dtype = MODELS[name]
    m = FRModel.synthetic(arch, dtype=dtype)
    L = N.lib()
    dtypes = {v: k for k, v in N.FR_DTYPE.items()}
    out = []
    try:
        for t in range(L.fr_debug_tensor_count(m.handle)):
            H, W, C = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            N.check(L.fr_debug_tensor_shape(m.handle, t, ctypes.byref(H), ctypes.byref(W), ctypes.byref(C)))
            out.append([L.fr_debug_tensor_name(m.handle, t).decode(), H.value, W.value, C.value,
                        dtypes[L.fr_debug_tensor_dtype(m.handle, t)]])
    finally:
        m.close()
    return {"tensors": out}


def golden(name):
    with open(os.path.join(GOLDEN_DIR, name + ".json")) as f:
        return json.load(f)


if __name__ == "__main__":
    out_dir = sys.argv[1] if len(sys.argv) > 1 else GOLDEN_DIR
    os.makedirs(out_dir, exist_ok=True)
    for name in MODELS:
        with open(os.path.join(out_dir, name + ".json"), "w") as f:
            json.dump(plans(name), f, indent=0, sort_keys=True)
            f.write("\n")
        with open(os.path.join(out_dir, name + "_tensors.json"), "w") as f:
            json.dump(tensors(name), f, indent=0, sort_keys=True)
            f.write("\n")
        print("wrote", name)
