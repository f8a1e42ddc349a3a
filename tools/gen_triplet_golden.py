#!/usr/bin/env python3
"""Generate the triplet fixture tests/golden/triplet_golden.npz (run where tools/gen_golden.py runs: it needs the
reference checkout; no test and no GPU run needs this tool).

The reference's OWN ``mine_semi_hard_triplets`` and ``mine_batch_hard_triplets`` (models/facenet/
facenet_dataloader.py:169-284), ``mine_triplets`` and ``TripletLoss`` (models/facenet/facenet_model.py:53-115), loaded
by file path with tools/gen_golden.py's torchvision stubs and an empty ``facenet_pytorch``, in float64 on the CPU with
autograd, on one tiny case (N = 14, D = 16, margin 0.5) whose rows are float32 values.  The case contains a singleton
label, two identical rows of one label (d_ap = 0, and an inactive triplet: every negative is farther than the margin),
pairs that take the semi-hard branch and pairs that fall back, and rows that are anchor, positive and negative at
once.  The seed is searched until every comparison the mining makes (d_an against d_ap and against d_ap + margin, the
winner against the runner-up) is decided by at least GAP = 50 times the bound on float32's error in it
(tests/triplet_ref.py), so that float32 and float64 make the same choices; distances that are equal because two rows
are equal stay equal in any precision.

Output: data only (inputs and expected outputs).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gen_golden as GG  # noqa: E402  (the reference's location and the torchvision stubs)
import triplet_ref as TR  # noqa: E402

N, D, MARGIN, U, GAP = 14, 16, 0.5, 1.7, 50.0
LABELS = np.array([0, 0, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 7, 9])  # 7 and 9: singletons (7 is every anchor's negative)


def inputs(seed):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((10, D)) * 0.22
    E = centres[LABELS] + rng.standard_normal((N, D)) * 0.09
    E[0] = centres[0] + 1.2 * np.sign(centres[0]) / np.sqrt(D)  # a tight class far from every other row
    E[1] = E[0]
    return E.astype(np.float32).astype(np.float64)


def min_gap(E):
    """The smallest ratio of a comparison's gap to the bound on float32's error in it (tests/triplet_ref.py), over
    every comparison of the three mining rules; distances of equal rows, equal in any precision, aside."""
    d, db = TR.dist_f64(E)
    idx = np.arange(N)
    worst = np.inf
    for i in range(N):
        pos = idx[(LABELS == LABELS[i]) & (idx != i)]
        neg = idx[LABELS != LABELS[i]]
        for group in (pos, neg):  # the winner against every other candidate
            for j in group:
                for k in group:
                    if j < k and not np.array_equal(E[j], E[k]):
                        worst = min(worst, abs(d[i, j] - d[i, k]) / (db[i, j] + db[i, k]))
        for p in pos:
            tau = db[i, neg] + db[i, p] + 2 * TR.EPS * (d[i, p] + MARGIN)
            worst = min(worst, (np.abs(d[i, neg] - d[i, p]) / tau).min(),
                        (np.abs(d[i, p] + MARGIN - d[i, neg]) / tau).min())
    return worst


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(GG.REF, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(out=os.path.join(ROOT, "tests", "golden", "triplet_golden.npz")):
    if not os.path.isdir(GG.REF):
        raise SystemExit(f"{GG.REF} not present: goldens are generated where the reference checkout is")
    GG.install_shims()
    fp = types.ModuleType("facenet_pytorch")
    fp.InceptionResnetV1 = object
    sys.modules.setdefault("facenet_pytorch", fp)
    dl = load("models/facenet/facenet_dataloader.py", "ref_facenet_dataloader")
    fm = load("models/facenet/facenet_model.py", "ref_facenet_model")

    labels = torch.from_numpy(LABELS)
    for seed in range(100000):
        E = inputs(seed)
        if min_gap(E) < GAP:
            continue
        x = torch.from_numpy(E)
        semi = dl.mine_semi_hard_triplets(x, labels, MARGIN)
        d = torch.cdist(x, x)
        took = [bool(d[a, p] < d[a, n] < d[a, p] + MARGIN) for a, p, n in zip(*semi)]
        if 0.3 <= np.mean(took) <= 0.7:
            break
    else:
        raise SystemExit("no seed meets the gap")
    print(f"seed {seed}: min gap / bound {min_gap(E):.1f}, semi-hard share {np.mean(took):.2f}")

    hard = dl.mine_batch_hard_triplets(x, labels)
    first = [(int(a), int(p), int(n)) for a, p, n in fm.mine_triplets(x, labels, MARGIN)]
    res = dict(E=E, labels=LABELS, margin=np.float64(MARGIN), u=np.float64(U), semi_took=np.array(took, np.uint8))
    for key, (a, p, n) in (("semi", semi), ("hard", hard), ("first", tuple(zip(*first)))):
        a, p, n = (np.array([int(v) for v in w], np.int64) for w in (a, p, n))
        xg = torch.from_numpy(E).clone().requires_grad_(True)
        loss = fm.TripletLoss(margin=MARGIN)(xg[a], xg[p], xg[n])
        (U * loss).backward()
        res.update({f"{key}_a": a, f"{key}_p": p, f"{key}_n": n, f"{key}_loss": loss.detach().numpy(),
                    f"{key}_dE": xg.grad.numpy().copy()})
        print(key, len(a), "triplets, loss", float(loss.detach()))
    np.savez_compressed(out, **res)
    print(f"wrote {out} ({os.path.getsize(out) / 1024:.1f} KiB, {len(res)} arrays)")


if __name__ == "__main__":
    main()
