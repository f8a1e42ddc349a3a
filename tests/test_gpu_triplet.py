"""fr_triplet_* and facerecognition_amd.triplet on the GPU against tests/triplet_ref.py: bitwise against its float32
part on exact-grid inputs, and on float inputs judged by its float64 part, which also supplies every bound (eps = 2^-24;
derivations in its docstring).  Each assertion on a float result is error / bound <= 1; the largest ratio of every
quantity is printed (recorded in DESIGN.md §4 "Triplet mining and loss").

Measured largest ratios (MI355X; per case in DESIGN.md): loss 0.0035, hinge terms 0.016, pos_dist 0.016, neg_dist 0.025,
dE 0.027 (raw calls), 0.104 (Python paths against float64 torch); pairs undecided within the bounds: 0 of 510 at
(70, 16), 2 of 690 at (130, 128), 11 of 1070 at (257, 512).

Shapes: the smallest that cross each boundary of a 64 x 64 tile, of a 64-float D chunk and of a 64-anchor band
(N 2 / 70 / 130 / 257, D 16 / 128 / 512); T = 1, 65 and about 770 cross the 4-triplet workgroup, the 256-triplet scan
chunk and leave the last chunk ragged.
"""
import functools

import numpy as np
import pytest

from tests import triplet_ref as R

pytestmark = pytest.mark.gpu

MODES = (R.SEMI_HARD, R.BATCH_HARD, R.FIRST)
worst = {}


def note(name, err, bound):
    err, bound = np.abs(np.asarray(err, np.float64)), np.asarray(bound, np.float64)
    assert np.all(err <= bound), (name, float(np.max(err - bound)))
    r = float(np.max(err / np.maximum(bound, 1e-300)))
    worst[name] = max(worst.get(name, 0.0), r)
    print(f"  {name}: largest error / bound = {r:.3g}")
    return r


@functools.lru_cache(maxsize=None)
def grid_ref(N, D):
    E, labels = R.grid_case(N, D, seed=3)
    return E, labels, R.gram_dist_f32(E)


@functools.lru_cache(maxsize=None)
def float_ref(N, D):
    E, labels = R.float_case(N, D, seed=7)
    return (E, labels) + R.dist_f64(E)


def mine(gpu, E, labels, mode, margin, ws_bytes=None):
    import torch

    from facerecognition_amd import triplet as T

    out = T._mine(torch.from_numpy(E).to(gpu), torch.from_numpy(labels).to(gpu), mode, margin, ws_bytes)
    return [t.cpu().numpy() for t in out]


def min_ws(N):
    return 4 * (64 * N + 64 * ((N + 63) // 64))


@pytest.mark.parametrize("margin", [0.2, 0.5])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,D", [(2, 16), (70, 16), (130, 512)])
def test_exact_grid_is_bitwise_the_float32_reference(gpu, N, D, mode, margin):
    E, labels, d32 = grid_ref(N, D)
    lims, a, p, n, semi = R.mine(d32, labels, mode, margin)
    ga, gp, gn, gsemi, glims = mine(gpu, E, labels, mode, margin)
    assert np.array_equal(glims, lims)
    assert np.array_equal(ga, a) and np.array_equal(gp, p) and np.array_equal(gn, n)
    assert np.array_equal(gsemi, semi)
    assert (len(a) > 0) == (N > 2)


@pytest.mark.parametrize("N", [2, 70])
def test_one_label_or_all_distinct_labels_give_no_triplets(gpu, N):
    E = R.grid_case(N, 16, seed=3)[0]
    for labels in (np.full(N, 5, np.int32), np.arange(N, dtype=np.int32) - 3):
        for mode in MODES:
            a, p, n, semi, lims = mine(gpu, E, labels, mode, 0.2)
            assert len(a) == len(p) == len(n) == len(semi) == 0 and not lims.any()


@pytest.mark.parametrize("N,D", [(130, 512), (257, 128)])
def test_band_height_changes_no_bit(gpu, N, D):
    E, labels = R.float_case(N, D, seed=11)
    for mode in MODES:
        full = mine(gpu, E, labels, mode, R.FLOAT_MARGIN)
        banded = mine(gpu, E, labels, mode, R.FLOAT_MARGIN, ws_bytes=min_ws(N))
        assert len(full[0]) > N // 2
        for x, y in zip(full, banded):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,D", R.FLOAT_SHAPES)
def test_float_inputs_every_choice_is_valid(gpu, N, D, mode):
    E, labels, d, db = float_ref(N, D)
    a, p, n, semi, lims = mine(gpu, E, labels, mode, R.FLOAT_MARGIN)
    rl, ra, rp, _, _ = R.mine(d, labels, mode, R.FLOAT_MARGIN)
    assert np.array_equal(lims, rl) and np.array_equal(a, ra)
    if mode != R.BATCH_HARD:
        assert np.array_equal(p, rp)  # anchors ascending, then positives ascending
    cases = {}
    for t in range(len(a)):
        ok, case = R.valid_choice(d, db, labels, mode, R.FLOAT_MARGIN, a[t], p[t], n[t])
        assert ok, (t, a[t], p[t], n[t], case)
        assert case != "semi" or semi[t] == 1
        assert case not in ("fallback", "hard") or semi[t] == 0
        cases[case] = cases.get(case, 0) + 1
    print(f"  ({N}, {D}) mode {mode}: {cases}")


def loss_case(T, seed=5):
    """Unit-norm float rows (N = 130, D = 128) with one duplicated row, random triplets over them: row HUB is the
    anchor, the positive and the negative of a quarter of the triplets each, the duplicate pair appears as (a, p)."""
    rng = np.random.default_rng(seed)
    E = R.float_case(130, 128, seed=7)[0].copy()
    E[21] = E[20]
    HUB = 9
    a, p, n = (rng.integers(0, 130, T).astype(np.int32) for _ in range(3))
    if T > 1:
        a[0::8], p[1::8], n[2::8] = HUB, HUB, HUB
        a[3], p[3] = 20, 21       # delta_ap = 1e-6 sqrt(D)
        a[4], n[4] = 21, 20       # delta_an tiny: active, with a large weight
    return E, a, p, n


def run_loss(gpu, E, a, p, n, margin, u):
    import torch

    from facerecognition_amd import triplet as T

    e = torch.from_numpy(E).to(gpu)
    ia, ip, in_ = (torch.from_numpy(v).to(gpu) for v in (a, p, n))
    stats, terms = T._forward(e, ia, ip, in_, margin)
    dE = T._backward(e, ia, ip, in_, margin, u)
    return stats.cpu().numpy(), terms.cpu().numpy(), dE.cpu().numpy()


def check_loss(tag, ref, stats, terms, dE):
    note(f"{tag} loss", stats[0] - ref["loss"], ref["loss_bound"])
    note(f"{tag} hinge", terms[:, 0] - ref["hinge"], ref["hinge_bound"])
    note(f"{tag} pos_dist", stats[2] - ref["pos_dist"], ref["pos_dist_bound"])
    note(f"{tag} neg_dist", stats[3] - ref["neg_dist"], ref["neg_dist_bound"])
    assert ref["accuracy_lo"] - 4 * R.EPS <= stats[1] <= ref["accuracy_hi"] + 4 * R.EPS
    note(f"{tag} dE", dE - ref["dE"], ref["dE_bound"])


@pytest.mark.parametrize("T", [1, 65, 770])
def test_loss_and_gradient_within_the_float64_bounds(gpu, T):
    E, a, p, n = loss_case(T)
    margin, u = 0.5, 1.7
    ref = R.loss_ref(E, a, p, n, margin, u)
    if T > 1:
        assert ref["active"].any() and not ref["active"].all()  # inactive triplets
        assert ref["delta_ap"].min() < 1e-4 and ref["delta_an"].min() < 1e-4  # the duplicates
        assert min((a == 9).sum(), (p == 9).sum(), (n == 9).sum()) >= T // 8
        assert ref["unsure"].mean() < 0.05
    stats, terms, dE = run_loss(gpu, E, a, p, n, margin, u)
    touched = np.zeros(len(E), bool)
    touched[np.concatenate([a, p, n])] = True
    assert not dE[~touched].any()  # rows of no triplet are written as zeros
    check_loss(f"T={T}", ref, stats, terms, dE)


def test_gradient_passes_at_the_hinge_zero(gpu):
    """Grid rows, rows p and n equal, margin below half an ulp of delta: fl(margin + delta) - delta is exactly 0 in
    float32, the triplet is active (clamp_min passes the gradient at equality) and rows p and n receive -+ the term."""
    E = R.grid_case(70, 16, seed=3)[0].copy()
    E[31] = E[30]
    a = np.array([2, 5, 2], np.int32)
    p = np.array([30, 30, 7], np.int32)
    n = np.array([31, 31, 8], np.int32)
    margin = 1e-8
    ref = R.loss_ref(E, a, p, n, margin)
    assert ref["delta_ap"][:2].min() > 0.5 and ref["active"][:2].all() and not ref["unsure"][:2].any()
    stats, terms, dE = run_loss(gpu, E, a, p, n, margin, 1.0)
    assert terms[0, 3] == 0 and terms[1, 3] == 0 and terms[0, 0] == 0  # exactly at the hinge's zero
    assert np.abs(ref["dE"][30]).max() > 1e-3
    assert np.abs(dE[30]).max() > 1e-3 and np.array_equal(dE[31], -dE[30])
    check_loss("hinge zero", ref, stats, terms, dE)


def test_two_runs_are_bitwise_equal(gpu):
    E, labels = R.float_case(257, 512, seed=7)
    runs = []
    for _ in range(2):
        a, p, n, semi, lims = mine(gpu, E, labels, R.SEMI_HARD, R.FLOAT_MARGIN)
        stats, terms, dE = run_loss(gpu, E, a, p, n, 0.5, 1.7)
        runs.append((a, p, n, semi, lims, stats, terms, dE))
    for x, y in zip(*runs):
        assert np.array_equal(x, y)
    assert np.abs(runs[0][-1]).max() > 0


def test_python_face_runs_the_reference_training_step(gpu):
    import torch
    from torch import nn

    import facerecognition_amd as fra

    E, labels, d, db = float_ref(130, 128)
    y = torch.from_numpy(labels).to(gpu).long()
    emb = torch.from_numpy(E).to(gpu).requires_grad_(True)
    # the reference's step: mine on detached embeddings, gather, criterion, backward
    a_idx, p_idx, n_idx = fra.mine_semi_hard_triplets(emb.detach(), y, 0.2)
    assert a_idx.dtype == torch.int64 and a_idx.device == emb.device and len(a_idx) == len(R.mine(d, labels, 0, 0.2)[1])
    criterion = fra.TripletLoss(margin=0.5)
    anchor, positive, negative = emb[a_idx], emb[p_idx], emb[n_idx]
    loss = criterion(anchor, positive, negative)
    assert loss.dim() == 0
    loss.backward()
    a, p, n = (v.cpu().numpy() for v in (a_idx, p_idx, n_idx))
    ref = R.loss_ref(E, a, p, n, 0.5)
    x64 = torch.from_numpy(E).double().requires_grad_(True)
    l64 = nn.TripletMarginLoss(margin=float(np.float32(0.5)), p=2)(x64[a], x64[p], x64[n])
    l64.backward()
    assert abs(float(l64) - ref["loss"]) <= 1e-12 and np.abs(x64.grad.numpy() - ref["dE"]).max() <= 1e-12
    note("module loss", loss.item() - float(l64), ref["loss_bound"])
    note("module dE", emb.grad.cpu().numpy() - x64.grad.numpy(), ref["dE_bound"])
    # the fused gather form: the same gradient, written as dE directly
    emb2 = torch.from_numpy(E).to(gpu).requires_grad_(True)
    fused = fra.triplet_loss(emb2, a_idx, p_idx, n_idx, 0.5)
    (3.0 * fused).backward()
    assert fused.item() == loss.item()
    note("fused dE", emb2.grad.cpu().numpy() / 3.0 - x64.grad.numpy(), ref["dE_bound"] + 2 * R.EPS * np.abs(ref["dE"]))
    assert np.all(np.abs(emb2.grad.cpu().numpy() / 3.0 - emb.grad.cpu().numpy()) <= 2 * ref["dE_bound"])
    # metrics and the one-call step
    m = fra.compute_triplet_metrics(anchor.detach(), positive.detach(), negative.detach())
    assert set(m) == {"accuracy", "pos_dist", "neg_dist"} and all(isinstance(v, float) for v in m.values())
    note("metrics pos_dist", m["pos_dist"] - ref["pos_dist"], ref["pos_dist_bound"])
    note("metrics neg_dist", m["neg_dist"] - ref["neg_dist"], ref["neg_dist_bound"])
    assert ref["accuracy_lo"] - 4 * R.EPS <= m["accuracy"] <= ref["accuracy_hi"] + 4 * R.EPS
    emb3 = torch.from_numpy(E).to(gpu).requires_grad_(True)
    step_loss, info = fra.online_triplet_loss(emb3, y, margin=0.2, mining="semi_hard", loss_margin=0.5)
    assert step_loss.item() == loss.item() and info["triplets"] == len(a)
    assert info["accuracy"] == m["accuracy"] and info["pos_dist"] == m["pos_dist"] and info["neg_dist"] == m["neg_dist"]
    assert 0.2 <= info["semi_hard_fraction"] <= 0.8
    step_loss.backward()
    assert torch.equal(emb3.grad * 3.0, emb2.grad)
    hard = fra.mine_batch_hard_triplets(emb.detach(), y)
    assert hard[0].tolist() == R.mine(d, labels, R.BATCH_HARD, 1.0)[1].tolist() and len(hard[2]) == len(hard[0])
    trip = fra.mine_triplets(emb.detach(), y)
    assert isinstance(trip, list) and len(trip) == len(a) and all(isinstance(v, int) for v in trip[0])
    none_loss, none_info = fra.online_triplet_loss(emb, torch.arange(130, device=gpu))
    assert none_loss is None and none_info["triplets"] == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fra.mine_semi_hard_triplets(emb.detach().cpu(), y.cpu())
