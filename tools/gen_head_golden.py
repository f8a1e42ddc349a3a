"""Writes tests/golden/head_golden.npz: one small head-training case (inputs, the dropout mask, and every forward and
backward output) computed by torch float64 autograd on the CPU.  tests/test_head_ref.py pins tests/head_ref.py to it.

    python tools/gen_head_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.head_ref import BATCH_STATS, DROPOUT, dropout_mask, make_case  # noqa: E402
from tests.test_head_ref import torch_head  # noqa: E402


def main():
    B, Cin, S, N = 6, 4, 4, 8
    p, eps, mom, seed, offset = 0.5, 1e-5, 0.1, 0x123456789ABCDEF, 3
    case = make_case(11, B, Cin, S, N, input_bn=True, bias=True)
    keep = dropout_mask(B, Cin * S, p, seed, offset)
    t = torch_head(case, S, BATCH_STATS | DROPOUT, p, eps, mom, keep)
    out = {"in_" + k: v for k, v in case.items() if v is not None}
    out.update({"out_" + k: v for k, v in t.items()})
    out["keep"] = keep
    out["scalars"] = np.array([S, BATCH_STATS | DROPOUT, p, eps, mom], np.float64)
    out["seed_offset"] = np.array([seed, offset], np.uint64)
    path = os.path.join(ROOT, "tests", "golden", "head_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
