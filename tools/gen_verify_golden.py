#!/usr/bin/env python3
"""Generate the verification fixture tests/golden/verify_golden.npz (run where tools/gen_golden.py runs: it needs the
reference checkout; no test and no GPU run needs this tool).

The reference's OWN ``compute_verification_accuracy`` (models/arcface/train_arcface.py:114-210; the copy in
models/facenet/train_facenet.py:64-160 is the same text), loaded by file path with tools/gen_golden.py's torchvision
stubs, on one seeded input: 66 float32 rows of dimension 16, not of unit length, in 12 classes of five rows plus six
singletons (which its ``valid_labels`` drops), ``np.random.seed(SEED)`` immediately before the call, 400 pairs.  The
classes overlap, so the accuracy is well below 1 and the best threshold is inside the sweep.

Output: data only (the inputs and what the function returned).
"""
import contextlib
import importlib.util
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_golden as GG  # noqa: E402  (the reference's location and the torchvision stubs)

SEED, NUM_PAIRS, D = 20240, 400, 16


def inputs():
    rng = np.random.default_rng(5)
    labels = np.r_[np.repeat(np.arange(12) * 3 + 100, 5), 900 + np.arange(6)]
    centres = rng.standard_normal((int(labels.max()) + 1, D))
    E = centres[labels] + 1.1 * rng.standard_normal((len(labels), D))
    E *= rng.uniform(0.5, 2.0, size=(len(labels), 1))
    order = rng.permutation(len(labels))
    return E[order].astype(np.float32), labels[order].astype(np.int64)


def main(out=os.path.join(ROOT, "tests", "golden", "verify_golden.npz")):
    if not os.path.isdir(GG.REF):
        raise SystemExit(f"{GG.REF} not present: goldens are generated where the reference checkout is")
    GG.install_shims()
    spec = importlib.util.spec_from_file_location("ref_train_arcface",
                                                  os.path.join(GG.REF, "models/arcface/train_arcface.py"))
    mod = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stdout(io.StringIO()):
        spec.loader.exec_module(mod)
    E, labels = inputs()
    np.random.seed(SEED)
    acc, thr, m = mod.compute_verification_accuracy(E, labels, num_pairs=NUM_PAIRS)
    res = dict(E=E, labels=labels, seed=np.int64(SEED), num_pairs=np.int64(NUM_PAIRS), accuracy=np.float64(acc),
               best_threshold=np.float64(thr), pos_sim_mean=np.float64(m["pos_sim_mean"]),
               neg_sim_mean=np.float64(m["neg_sim_mean"]), num_pos_pairs=np.int64(m["num_pos_pairs"]),
               num_neg_pairs=np.int64(m["num_neg_pairs"]))
    print({k: v for k, v in res.items() if k not in ("E", "labels")})
    np.savez_compressed(out, **res)
    print(f"wrote {out} ({os.path.getsize(out) / 1024:.1f} KiB, {len(res)} arrays)")


if __name__ == "__main__":
    main()
