"""tests/arcmargin_ref.py (the float64 restatement the GPU tests check the device against) reproduces the reference's
own ArcMarginProduct + CrossEntropyLoss under float64 autograd (tests/golden/arcmargin_golden.npz, written by
tools/gen_arcmargin_golden.py) to 1e-12 relative: logits, per-sample loss, dE and dW, both margin modes, label
smoothing 0 / 0.1, without and with mixup."""
import os

import numpy as np
import pytest

from tests.arcmargin_ref import arcmargin_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arcmargin_golden.npz")
CASES = [(easy, ls, mix) for easy in (0, 1) for ls in (0, 1) for mix in (0, 1)]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_fixture_contains_every_branch(gold):
    r = arcmargin_ref(gold["E"], gold["W"], gold["label"], margin=float(gold["margin"]))
    c, th = r["c_label"], r["th"]
    assert np.any(np.abs(c - 1) < 1e-12) and np.any(np.abs(c + 1) < 1e-12)  # the sine's clamp, both ends
    assert np.any((c > th) & (c < 0)) and np.any((c < th) & (c > -1 + 1e-6)) and np.any((c > 0) & (c < 1 - 1e-6))
    lab = gold["label"]
    assert len(set(lab.tolist())) < len(lab) < len(gold["W"])  # a shared label, classes nobody labels
    assert 0 in lab and len(gold["W"]) - 1 in lab


@pytest.mark.parametrize("easy,ls,mix", CASES)
def test_ref_reproduces_the_reference(gold, easy, ls, mix):
    key = f"easy{easy}_ls{ls}_mix{mix}"
    r = arcmargin_ref(gold["E"], gold["W"], gold["label"], gold["label_b"] if mix else None,
                      lam=float(gold["lam"]) if mix else 1.0, scale=float(gold["scale"]), margin=float(gold["margin"]),
                      easy_margin=bool(easy), label_smoothing=ls / 10, u=gold["u"])
    for name in ("z", "loss", "dE", "dW"):
        assert rel(r[name], gold[f"{key}_{name}"]) <= 1e-12, (key, name, rel(r[name], gold[f"{key}_{name}"]))


def test_ignored_labels_and_bounds_are_well_formed(gold):
    lab = gold["label"].copy()
    lab[2], lab[6] = -1, len(gold["W"])
    r = arcmargin_ref(gold["E"], gold["W"], lab, label_smoothing=0.1)
    assert r["loss"][2] == 0 and r["loss"][6] == 0 and np.all(r["dE"][[2, 6]] == 0)
    keep = np.array([b for b in range(len(lab)) if b not in (2, 6)])
    k = arcmargin_ref(gold["E"][keep], gold["W"], lab[keep], label_smoothing=0.1)
    assert rel(r["dW"], k["dW"]) <= 1e-12 and rel(r["loss"][keep], k["loss"]) <= 1e-12
    for name in ("z_bound", "lse_bound", "loss_bound", "dE_bound", "dW_bound"):
        assert np.all(np.isfinite(r[name])) and np.all(r[name] >= 0), name
