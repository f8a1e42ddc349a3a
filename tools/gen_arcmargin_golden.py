#!/usr/bin/env python3
"""Generate the margin-loss fixture tests/golden/arcmargin_golden.npz (run where tools/gen_golden.py runs: it needs
the reference checkout; no test and no GPU run needs this tool).

The reference's OWN ``ArcMarginProduct`` (models/arcface/arcface_model.py:23-62, loaded by file path) and
``nn.CrossEntropyLoss(label_smoothing=..., reduction='none')`` in float64 with autograd, on one tiny case
(B = 8, C = 11, D = 16) that contains every branch: label cosines on the phi branch, below cos(pi - m), below 0,
and +1 / -1 (the 1e-7 clamp of the sine); a label shared by two samples; classes nobody labels.  Both margin
modes, label smoothing 0 and 0.1, without mixup and with mixup at lam = 0.3 (lam CE(z, y) + (1 - lam) CE(z, y'),
logits from the first label).  The gradient is that of sum_b u_b loss_b for a fixed non-uniform u.

Output: data only (inputs and expected outputs).
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_golden as GG  # noqa: E402  (the reference's location)

B, C, D = 8, 11, 16
SCALE, MARGIN, LAM = 64.0, 0.5, 0.3


def inputs():
    rng = np.random.default_rng(20240)
    W = rng.standard_normal((C, D)) * rng.uniform(0.5, 2.0, (C, 1))
    E = rng.standard_normal((B, D)) * rng.uniform(0.3, 5.0, (B, 1))
    label = np.array([0, C - 1, 3, 3, 5, 7, 2, 9])
    label_b = np.array([4, 0, 3, C - 1, 1, 7, 6, 2])
    E[0] = 3.0 * W[0]                                   # cosine +1: the clamp on the phi branch
    E[1] = -2.0 * W[C - 1]                              # cosine -1: the clamp, below both thresholds
    E[2] = 1.5 * W[3] + 0.4 * rng.standard_normal(D)    # a high cosine, phi branch
    E[4] = -W[5] + 0.15 * rng.standard_normal(D)        # below cos(pi - m)
    E[5] = -0.3 * W[7] + rng.standard_normal(D)         # between the two thresholds, most likely
    return E, W, label, label_b


def main(out=os.path.join(ROOT, "tests", "golden", "arcmargin_golden.npz")):
    if not os.path.isdir(GG.REF):
        raise SystemExit(f"{GG.REF} not present: goldens are generated where the reference checkout is")
    spec = importlib.util.spec_from_file_location("ref_arcface_model",
                                                  os.path.join(GG.REF, "models/arcface/arcface_model.py"))
    am = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(am)
    torch.set_default_dtype(torch.float64)  # the module's own zeros() / FloatTensor follow it

    E, W, label, label_b = inputs()
    u = np.linspace(0.5, 2.0, B)
    res = dict(E=E, W=W, label=label, label_b=label_b, u=u, scale=np.float64(SCALE), margin=np.float64(MARGIN),
               lam=np.float64(LAM))
    for easy in (0, 1):
        head = am.ArcMarginProduct(D, C, scale=SCALE, margin=MARGIN, easy_margin=bool(easy)).double()
        with torch.no_grad():
            head.weight.copy_(torch.from_numpy(W))
        for ls in (0.0, 0.1):
            crit = torch.nn.CrossEntropyLoss(label_smoothing=ls, reduction="none")
            for mix in (0, 1):
                x = torch.from_numpy(E).clone().requires_grad_(True)
                head.zero_grad()
                z = head(x, torch.from_numpy(label))
                if mix:
                    loss = LAM * crit(z, torch.from_numpy(label)) + (1 - LAM) * crit(z, torch.from_numpy(label_b))
                else:
                    loss = crit(z, torch.from_numpy(label))
                (loss * torch.from_numpy(u)).sum().backward()
                key = f"easy{easy}_ls{int(ls * 10)}_mix{mix}"
                res[key + "_z"] = z.detach().numpy()
                res[key + "_loss"] = loss.detach().numpy()
                res[key + "_dE"] = x.grad.numpy().copy()
                res[key + "_dW"] = head.weight.grad.numpy().copy()
    Eh = E / np.linalg.norm(E, axis=1, keepdims=True)
    Wh = W / np.linalg.norm(W, axis=1, keepdims=True)
    print("label cosines:", np.round((Eh @ Wh.T)[np.arange(B), label], 4), " cos(pi - m) =", np.cos(np.pi - MARGIN))
    np.savez_compressed(out, **res)
    print(f"wrote {out} ({os.path.getsize(out) / 1024:.1f} KiB, {len(res)} arrays)")


if __name__ == "__main__":
    main()
