"""CPU checks of tests/stage_ref.py, before a GPU sees it: the float64 restatement of the IResNet100 stages and of
the layer1.0 transition reproduces the fp32 oracle, the per-conv bound holds for legitimate float32 arithmetic and
sees the faults these kernels can have, the selection weights have the properties that make
test_gpu_stage_exact.py's equality exact, and slice_stats sees localized faults of the transition."""
import functools

import numpy as np
import pytest
import torch

from tests import stage_ref as SR
from facerecognition_amd import weights as Wt
from facerecognition_amd.synthetic import synthetic_crops

ARCH = SR.ARCH
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
GROUPS = ("trans", "layer1", "layer2", "layer3")


@functools.lru_cache(maxsize=None)
def state_dict(which):
    return Wt.synth_state_dict(ARCH) if which == "synth" else SR.selection_state_dict(0)


@functools.lru_cache(maxsize=None)
def folded(which):
    return Wt.fold_state_dict(ARCH, state_dict(which))


@functools.lru_cache(maxsize=None)
def oracle_tensors(which):
    """{module name: NHWC float64 output} of one oracle forward on 3 crops: the stem's prelu, layer1.0 and its prelu,
    and every tensor of the three stages."""
    from oracle import models as M
    u8 = synthetic_crops(3, Wt.INPUT_SIZE[ARCH], seed=31)
    om = M.build_model(ARCH, state_dict(which))
    names = {"prelu", "layer1.0.prelu", "layer1.0"} | {n for s in SR.STAGES for n in SR.stage_tensors(s)}
    got, hooks = {}, []
    for n in sorted(names):
        hooks.append(om.get_submodule(n).register_forward_hook(
            lambda _m, _i, o, n=n: got.__setitem__(n, o.detach().permute(0, 2, 3, 1).contiguous().double().numpy())))
    M.embed(om, ARCH, u8)
    for h in hooks:
        h.remove()
    return got


# ---- the restatement is the network: unrounded and chained over a whole group, it reproduces every hooked tensor of
# the oracle from the group's hooked input to fp32 noise.  Measured largest max|diff| / max|out| over the group's
# tensors (synth / selection): trans 5.2e-7 / 5.6e-8, layer1 5.1e-7 / 9.1e-8, layer2 5.6e-7 / 1.6e-7, layer3 5.6e-7 /
# 2.1e-7 -- none above 1e-6.
@pytest.mark.parametrize("which", ["synth", "selection"])
@pytest.mark.parametrize("group", GROUPS)
def test_restatement_matches_oracle(group, which):
    got, fw = oracle_tensors(which), folded(which)
    if group == "trans":
        out = SR.transition(got["prelu"], fw, None)
        names = ["layer1.0.prelu", "layer1.0"]
    else:
        out = SR.chain(group, got[SR.stage_tensors(group)[0]], fw, None)
        names = SR.stage_tensors(group)[1:]
    worst = 0.0
    for n in names:
        want = got[n]
        assert out[n].shape == want.shape
        err, top = np.abs(out[n] - want).max(), np.abs(want).max()
        worst = max(worst, err / top)
        assert err <= 1e-5 * top, f"{group} {n}: the restatement differs from the oracle by {err:.3e} on {top:.3g}"
    print(f"{group} {which}: {len(names)} tensors, largest max|diff| / max|out| {worst:.1e}")


# ---- the bound
# one conv of each geometry: (conv, kind, input, residual, output)
CASES = {"56x56x64": ("layer1.1.conv2", "conv2", "layer1.1.prelu", "layer1.0", "layer1.1"),
         "28x28x128": ("layer2.6.conv1", "conv1", "layer2.5", None, "layer2.6.prelu"),
         "14x14x256": ("layer3.15.conv2", "conv2", "layer3.15.prelu", "layer3.14", "layer3.15"),
         "tail256-512": ("layer4.0.conv1", "tail", "layer3.29", None, "layer4.0.prelu")}


@functools.lru_cache(maxsize=None)
def stored(name, dtype):
    """The oracle's tensor rounded to the storage type: a stage conv's stored input (synthetic weights)."""
    return SR.rnd(oracle_tensors("synth")[name], DT[dtype])


@functools.lru_cache(maxsize=None)
def case_ref(case, dtype):
    conv, kind, tin, tres, _ = CASES[case]
    X = None if tres is None else stored(tres, dtype)
    return SR.conv_ref(stored(tin, dtype), folded("synth"), conv, kind, DT[dtype], X)


# Measured largest |rounded f32 result - ref| / bound (the same for both orders to three digits):
#   bf16: 56x56x64 0.976, 28x28x128 0.852, 14x14x256 0.916, tail 0.711
#   f16:  56x56x64 0.870, 28x28x128 0.496, 14x14x256 0.648, tail 0.280
# (the worst element is a storage rounding next to a tie, h |ref| of it; the accumulation term makes the room that the
# K-step order needs)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_bound_holds_for_float32_orders(case, dtype):
    conv, kind, tin, tres, _ = CASES[case]
    dt, fw = DT[dtype], folded("synth")
    I, X = stored(tin, dtype), None if tres is None else stored(tres, dtype)
    ref, bound = case_ref(case, dtype)
    assert np.isfinite(ref).all() and (bound > 0).all()
    outs = []
    for perm in (None, np.random.default_rng(1).permutation(I.shape[3])):
        y, _ = SR.conv_ref(I, fw, conv, kind, dt, X, False, np.float32, perm)
        assert y.dtype == np.float32
        outs.append(y)
        r = SR.ratio(SR.rnd(y, dt), ref, bound).max()
        print(f"{case} {conv} {dtype} order {len(outs)}: largest error / bound {r:.3f}")
        assert r <= 1, f"{case} {dtype}: a legitimate float32 evaluation is outside the bound ({r:.3f})"
    assert not np.array_equal(outs[0], outs[1]), "the two evaluations are the same order"


def _fro(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _report(what, dtype, r, faulty, clean, rows=None):
    """Prints the planted fault's ratio with what the existing Frobenius bars (tests/test_gpu_stage.py: 2e-2 per
    tensor, per image and 14-row part in the split-stage test) see of it at this conv."""
    part = ""
    if rows is not None:
        part = f", worst image and 14-row part {max(_fro(faulty[i:i + 1, rows], clean[i:i + 1, rows]) for i in range(len(clean))):.2e}"
    print(f"FAULT {what} {dtype}: ratio {r:.3g}; Frobenius of the tensor {_fro(faulty, clean):.2e}{part}")


# ---- the bound sees the faults these kernels can have.  `clean` is the rounded float64 result (ratio <= 1 by
# construction); each fault is planted into it and must give a ratio > 1 at the planted place.  Measured ratio
# (bf16 / f16) and, in brackets, the Frobenius error the fault leaves in the conv's own output tensor (bf16):
#   1 K-step dropped              56x56x64 1570 / 1900 (2.9e-2), 28x28x128 360 / 431 (6.8e-2),
#                                 14x14x256 73 / 131 (5.1e-3), tail 113 / 134 (2.3e-2)
#   2 corner pixel, interior b9   28x28x128 180 / 289 (2.3e-3), tail 173 / 215 (7.5e-3)
#   3 stale halo row (below)      28 rows: 1540 - 1700 / 1700 - 2010 (2.5e-2 - 2.6e-2; of its image and part 3.8e-2 - 4.0e-2)
#                                 56 rows: 566 - 751 / 658 - 925 (1.5e-2 - 2.1e-2; of its image and part 3.4e-2 - 4.9e-2)
#   4 two taps swapped            56x56x64 2870 / 3510 (7.4e-2), 28x28x128 1460 / 1470 (3.8e-1),
#                                 14x14x256 549 / 890 (8.3e-2), tail 685 / 716 (4.9e-1)
#   5 residual left out, a pixel  56x56x64 437 / 2370 (9.9e-3), 14x14x256 428 / 1290 (4.2e-2)
# The smallest ratio is 73: every fault is far outside the bound, where the Frobenius numbers straddle the 2e-2 of
# tests/test_gpu_stage.py (test_frobenius_bars_downstream_of_a_fault measures them where that file looks).
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_bound_sees_planted_faults(dtype):
    dt, fw = DT[dtype], folded("synth")
    for case in sorted(CASES):
        conv, kind, tin, tres, _ = CASES[case]
        I, X = stored(tin, dtype), None if tres is None else stored(tres, dtype)
        ref, bound = case_ref(case, dtype)
        clean = SR.rnd(ref, dt)
        assert SR.ratio(clean, ref, bound).max() <= 1
        w = SR.weight(fw, conv, dt)

        def redo(I2=I, w2=w, X2=X):
            """The conv with another input / weights / residual, rounded."""
            f2 = dict(fw)
            f2[conv + ".w"] = w2.astype(np.float32)
            return SR.rnd(SR.conv_ref(I2, f2, conv, kind, dt, X2, False)[0], dt)

        # 1. one K-step dropped: 32 input channels of one tap, for one 16-channel output fragment
        w1 = w.copy()
        w1[16:32, 2, 1, 32:64] = 0
        f = clean.copy()
        f[..., 16:32] = redo(w2=w1)[..., 16:32]
        r = SR.ratio(f, ref, bound)
        assert r[..., :16].max() <= 1 and r[..., 32:].max() <= 1
        _report(f"1 K-step dropped {case}", dtype, r[..., 16:32].max(), f, clean)
        assert r[..., 16:32].max() > 1, f"{case}: a dropped K-step stays inside the bound"

        # 4. two taps of the conv swapped
        w4 = w.copy()
        w4[:, 0, 0], w4[:, 0, 1] = w[:, 0, 1], w[:, 0, 0]
        f = redo(w2=w4)
        r = SR.ratio(f, ref, bound).max()
        _report(f"4 taps swapped {case}", dtype, r, f, clean)
        assert r > 1, f"{case}: two swapped taps stay inside the bound"

        if kind != "conv2":
            # 2. the corner pixel (0, 0) of image 1 given the interior row of b9
            b9 = np.asarray(fw[conv + ".b9"], np.float64)
            f2 = dict(fw)
            f2[conv + ".b9"] = np.repeat(b9[4:5], 9, axis=0).astype(np.float32)
            assert not np.array_equal(b9[0], b9[4])
            f = clean.copy()
            f[1, 0, 0] = SR.rnd(SR.conv_ref(I, f2, conv, kind, dt, None, False)[0], dt)[1, 0, 0]
            r = SR.ratio(f, ref, bound)
            _report(f"2 corner class {case}", dtype, r[1, 0, 0].max(), f, clean)
            assert r[1, 0, 0].max() > 1, f"{case}: a corner pixel with the interior bias stays inside the bound"
            assert np.count_nonzero(r > 1) == np.count_nonzero(r[1, 0, 0] > 1)
        else:
            # 5. the residual of conv2 left out at one pixel
            f = clean.copy()
            f[2, 5, 7] = redo(X2=np.zeros_like(X))[2, 5, 7]
            r = SR.ratio(f, ref, bound)
            _report(f"5 residual left out {case}", dtype, r[2, 5, 7].max(), f, clean)
            assert r[2, 5, 7].max() > 1, f"{case}: a lost residual stays inside the bound"


# the convs of fault 3: (stage, conv, kind, input, residual, the tensor two convs before the input)
STALE = [("layer2", "layer2.6.conv2", "conv2", "layer2.6.prelu", "layer2.5", "layer2.5.prelu"),
         ("layer1", "layer1.2.conv1", "conv1", "layer1.1", None, "layer1.0")]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("stage,conv,kind,tin,tres,told", STALE)
def test_bound_sees_stale_halo_row(stage, conv, kind, tin, tres, told, dtype):
    """3. The split stages exchange the boundary rows of every conv's input through parity-double-buffered slots: a
    part that reads its neighbour's row before the exchange sees the row of the tensor two convs earlier.  Planted
    for both parts of every boundary (rows 13 / 14 of a 28-row image; 13 / 14, 27 / 28, 41 / 42 of a 56-row one)."""
    dt, fw = DT[dtype], folded("synth")
    H = SR.STAGES[stage][1]
    I, old = stored(tin, dtype), stored(told, dtype)
    X = None if tres is None else stored(tres, dtype)
    ref, bound = SR.conv_ref(I, fw, conv, kind, dt, X)
    clean = SR.rnd(ref, dt)
    for edge in range(14, H, 14):
        for own, halo in ((edge - 1, edge), (edge, edge - 1)):  # the part's last / first row and its halo row
            I2 = I.copy()
            I2[:, halo] = old[:, halo]
            f = clean.copy()
            f[:, own] = SR.rnd(SR.conv_ref(I2, fw, conv, kind, dt, X, False)[0], dt)[:, own]
            r = SR.ratio(f, ref, bound)
            part = slice(14 * (own // 14), 14 * (own // 14) + 14)
            _report(f"3 stale halo row {halo} read by row {own} ({conv})", dtype, r[:, own].max(), f, clean, part)
            assert r[:, own].max() > 1, f"{conv}: a stale halo row {halo} stays inside the bound"
            assert np.delete(r, own, axis=1).max() <= 1


# ---- selection weights
def test_selection_state_dict_properties():
    sd, base, fw = state_dict("selection"), state_dict("synth"), folded("selection")
    touched, differs = set(), []
    for pre, member, blk in SR.selection_convs():
        name = f"{pre}.{member}"
        key = pre + (".downsample.0.weight" if member == "downsample" else f".{member}.weight")
        bns = {"conv1": (".bn1", ".bn2"), "conv2": (".bn3",), "downsample": (".downsample.1",)}[member]
        touched |= {key} | {pre + bn + s for bn in bns for s in (".weight", ".bias", ".running_mean", ".running_var")}
        w = fw[name + ".w"]  # [Cout, kh, kw, Cin]
        cout, kh, kw, cin = w.shape
        want = 0.25 if member == "conv2" else 1.0
        assert set(np.unique(w)) == {0.0, want}, f"{name}: f32 weights {np.unique(w)}"
        for dt in DT.values():  # the 16-bit weights are exactly 0 and one `want` per output channel
            wq = torch.from_numpy(w).to(dt).double().numpy().reshape(cout, -1)
            assert set(np.unique(wq)) == {0.0, want}, f"{name}: 16-bit weights {np.unique(wq)}"
            assert np.all((wq != 0).sum(axis=1) == 1), f"{name}: not one nonzero weight per output channel"
        # coverage: every (tap, 32-channel half) K-step
        o, r, s, c = np.nonzero(w)
        steps = set(zip((r * kw + s).tolist(), (c // 32).tolist()))
        assert len(steps) == kh * kw * (cin // 32), f"{name}: {len(steps)} of {kh * kw * (cin // 32)} K-steps reached"
        if member != "conv1":
            assert np.all(fw[name + ".b"] == 0), f"{name}: a bias on a conv that adds the residual / the downsample"
            continue
        touched.add(pre + ".prelu.weight")
        b9 = fw[name + ".b9"].astype(np.float64)  # [9, Cout]
        assert np.all(b9 * 16 == np.round(b9 * 16)) and np.abs(b9).max() <= 1.5, f"{name}: b9 is not exact"
        assert np.array_equal(fw[name + ".b"], fw[name + ".b9"][4])
        assert np.unique(b9[4]).size > 8, f"{name}: the biases do not vary"
        slope = fw[name + ".slope"].astype(np.float64)
        assert set(np.unique(slope)) == {0.125, 0.25, 0.5}, f"{name}: slopes {np.unique(slope)}"
        # b9 = t2 + [the selected tap is inside the image] t1: it differs between classes exactly where the tap leaves
        assert np.array_equal(o, np.arange(cout))
        tap = r * kw + s
        t1 = sd[pre + ".bn1.bias"].astype(np.float64)[c]
        t2 = sd[pre + ".bn2.bias"].astype(np.float64)
        assert np.all(t1 != 0) and np.all(t1 * 16 == np.round(t1 * 16)) and np.all(np.abs(t2) <= 0.5)
        for cls in range(9):
            rc, cc = divmod(cls, 3)
            tr, tc = np.divmod(tap, 3)
            inside = ~(((rc == 0) & (tr == 0)) | ((rc == 2) & (tr == 2)) | ((cc == 0) & (tc == 0)) | ((cc == 2) & (tc == 2)))
            assert np.array_equal(b9[cls], t2 + inside * t1), f"{name}: b9 class {cls}"
        differs.append(float((b9.max(axis=0) != b9.min(axis=0)).mean()))
        assert differs[-1] >= 0.25, f"{name}: b9 differs between classes in only {differs[-1]:.2f} of the channels"
    print(f"b9 differs between classes in {min(differs):.3f} .. {max(differs):.3f} of the channels")
    # nothing else changed (the stem, the strided .0 blocks' conv2 / downsample, layer4 and the head stay synthetic)
    assert set(sd) == set(base)
    for k in base:
        if k not in touched:
            assert np.array_equal(sd[k], base[k]), f"{k} changed"
    assert len(touched) == 20 + (2 + 12 + 29) * 15 + 2 * 10 and all(k in sd for k in touched)
    for k in ("layer2.0.conv1.weight", "layer3.0.conv2.weight", "layer4.0.downsample.0.weight", "conv1.weight", "fc.weight"):
        assert k not in touched


# Measured nonzero fraction of the least-filled stored tensor (bf16 / f16): trans 0.998 / 0.999, layer1 0.996 / 0.998,
# layer2 0.995 / 0.998, layer3 0.994 / 0.998.
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("group", GROUPS)
def test_selection_not_vacuous(group, dtype):
    """The rounded restatement with selection weights, on the oracle-captured input: at least half of every stored
    tensor's elements are nonzero, and moving one conv's taps by one position changes the result."""
    fw, dt, got = folded("selection"), DT[dtype], oracle_tensors("selection")
    if group == "trans":
        x = SR.rnd(got["prelu"], dt)
        run = lambda f: SR.transition(x, f, dt)
        conv, last = "layer1.0.conv2", "layer1.0"
    else:
        x = SR.rnd(got[SR.stage_tensors(group)[0]], dt)
        run = lambda f: SR.chain(group, x, f, dt)
        conv, last = SR.stage_convs(group)[-1][0], SR.stage_convs(group)[-1][4]
    out = run(fw)
    fracs = []
    for n, v in out.items():
        fracs.append(float((v != 0).mean()))
        assert fracs[-1] >= 0.5, f"{group} {n}: only {fracs[-1]:.3f} of the elements are nonzero"
        assert np.isfinite(v).all() and np.array_equal(v, SR.rnd(v, dt))
    print(f"{group} {dtype}: {len(out)} tensors, least nonzero fraction {min(fracs):.3f}, max {max(np.abs(v).max() for v in out.values()):.4g}")
    w = fw[conv + ".w"]
    moved = dict(fw)
    moved[conv + ".w"] = np.roll(w.reshape(w.shape[0], -1, w.shape[3]), 1, axis=1).reshape(w.shape)
    assert not np.array_equal(run(moved)[last], out[last]), f"{group}: shifting the taps of {conv} is invisible"


# ---- the detectors for the transition (synthetic weights): two legitimate f32 summation orders against the float64
# restatement, and two planted faults.  Measured (bf16 / f16), elem, pixel, channel statistic of layer1.0:
#   order 1          1.57e-2, 1.96e-3, 2.80e-4   /   1.96e-3, 2.45e-4, 3.97e-5
#   order 2          1.57e-2, 1.96e-3, 2.80e-4   /   1.96e-3, 2.46e-4, 3.64e-5      (ratios 1.00, 1.00, 1.00 / 1.00, 1.01, 1.09)
#   fragment x 1.10  channel statistic 1.21e-1 / 1.21e-1 (430x / 3000x);  Frobenius against order 2: 2.8e-2
#   column x 1.05    pixel statistic 9.69e-2 / 9.69e-2 (50x / 390x);  Frobenius 4.5e-3 (test_gpu_trans.py's bf16 bar: 4e-3)
# Both orders accumulate K-step by K-step (stage_ref.conv_sum) and flip few roundings between them.  Each conv as one
# float32 BLAS product instead measured, on the development host (bf16), 1.46e-2, 1.82e-3, 2.61e-4 with the channels
# in place and 7.8e-3, 1.09e-3, 1.56e-4 permuted: 1.86x, 1.67x, 1.67x apart, and 2.00x, 1.79x, 1.79x below order 1.  The
# element statistic is one element's distance in storage ulps (here one ulp against two in the same binade), so it moves
# in such steps; no pair is more than 2x apart.  These are not asserted, because they depend on the host's BLAS.  The
# factor 2 of test_gpu_stage_exact.py's test C stands on these measurements.
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_slice_stats_see_localized_faults_of_the_transition(dtype):
    dt, fw = DT[dtype], folded("synth")
    x = SR.rnd(oracle_tensors("synth")["prelu"], dt)
    n = "layer1.0"
    ref = SR.transition(x, fw, dt)[n]
    a = SR.transition(x, fw, dt, compute=np.float32)[n]
    b = SR.transition(x, fw, dt, compute=np.float32, perm_seed=1)[n]
    sa, sb = SR.slice_stats(a, ref), SR.slice_stats(b, ref)
    print(f"{dtype}: order 1 {sa}, order 2 {sb}, ratios {[max(p, q) / min(p, q) for p, q in zip(sa, sb)]}")
    assert not np.array_equal(a, b), "the two evaluations are the same order"
    for va, vb in zip(sa, sb):
        assert 0 < max(va, vb) <= 2 * min(va, vb), f"two legitimate orders differ by more than 2x: {sa} vs {sb}"
    clean = [max(va, vb) for va, vb in zip(sa, sb)]
    frag = a.copy()
    frag[1, :, :, 32:48] *= 1.10  # one 16-channel n-fragment of one image
    sf = SR.slice_stats(frag, ref)
    fro = _fro(frag, b)
    col = a.copy()
    col[1, :, 0, :] *= 1.05  # one border column of one image
    sc = SR.slice_stats(col, ref)
    print(f"{dtype}: fragment {sf} (Frobenius vs order 2 {fro:.2e}), column {sc} (Frobenius {_fro(col, b):.2e})")
    assert sf[2] > 2 * clean[2], f"fragment fault: channel statistic {sf[2]:.3e} vs clean {clean[2]:.3e}"
    assert sc[1] > 2 * clean[1], f"column fault: pixel statistic {sc[1]:.3e} vs clean {clean[1]:.3e}"


# ---- what the existing Frobenius bars see of such faults.  The layer2 split stage (bf16, three images) run free from
# its input, clean and with one fault planted in block 3 in every image; then the numbers test_gpu_stage.py asserts:
# the whole-tensor relative error of the tensors it looks at downstream of the fault (layer2.6, layer2.12,
# layer3.0.prelu; bar 2e-2), and the worst image and 14-row part of layer2.12 (test_split_stage_batches_and_exchange;
# bar 2e-2).  Measured:
#                                at its own output   layer2.6  layer2.12  layer3.0.prelu   worst part of layer2.12
#   0 another f32 order (noise)  1.2e-5              1.9e-3    4.3e-3     5.2e-3           4.7e-3
#   1 K-step dropped             5.9e-2              1.3e-2    1.5e-2     1.6e-2           1.6e-2      passes
#   2 corner class               3.7e-3              7.5e-4    1.9e-3     2.4e-3           2.6e-3      passes (below the noise)
#   3 stale halo row             2.7e-2              2.8e-2    3.0e-2     3.3e-2           4.5e-2      seen
#   4 taps swapped               3.8e-1              8.5e-2    8.9e-2     9.5e-2           9.7e-2      seen
#   5 residual left out, a pixel 3.3e-2              3.4e-2    3.5e-2     3.8e-2           6.8e-2      seen
# Faults 3 and 5 are seen by 1.4x - 1.9x when they hit every image of the batch; in one image of B the whole-tensor
# number falls by sqrt(B) (B = 5: 1.3e-2, passes) and only the per-image, per-part bar of the split-stage test still
# sees them.  The synthetic trunk amplifies an error along the residual stream (row 0: 1.2e-5 -> 4.3e-3), which is
# what lifts a one-row fault over the bar; in layer3 a dropped K-step is 5.1e-3 at its own conv.
LOOKED_AT = ("layer2.6", "layer2.12", "layer3.0.prelu")


@functools.lru_cache(maxsize=None)
def _layer2_clean():
    return SR.chain("layer2", stored("layer2.0", "bf16"), folded("synth"), torch.bfloat16)


def _layer2_faulty(at, plant=None, fw=None):
    """SR.chain's loop with conv `at` replaced: other folded weights `fw`, or plant(inputs so far, I, X) -> output."""
    dt, base = torch.bfloat16, folded("synth")
    out = {"layer2.0": stored("layer2.0", "bf16")}
    for name, kind, tin, tres, tout in SR.stage_convs("layer2"):
        X = None if tres is None else out[tres]
        y = SR.rnd(SR.conv_ref(out[tin], fw if name == at and fw else base, name, kind, dt, X, False)[0], dt)
        if name == at and plant:
            y = plant(out, out[tin], X, y, lambda I2, X2: SR.rnd(SR.conv_ref(I2, base, name, kind, dt, X2, False)[0], dt))
        out[tout] = y
    return out


def _stale(out, I, X, y, redo):  # part 0 (rows 0..13) reads halo row 14 from the tensor two convs earlier
    I2 = I.copy()
    I2[:, 14] = out["layer2.2.prelu"][:, 14]
    y = y.copy()
    y[:, 13] = redo(I2, X)[:, 13]
    return y


def _no_residual(out, I, X, y, redo):
    y = y.copy()
    y[:, 5, 7] = redo(I, np.zeros_like(X))[:, 5, 7]
    return y


def _edited(conv, edit):
    fw = dict(folded("synth"))
    edit(fw, conv)
    return fw


def _drop_kstep(fw, conv):
    fw[conv + ".w"] = fw[conv + ".w"].copy()
    fw[conv + ".w"][16:32, 2, 1, 32:64] = 0


def _corner(fw, conv):
    fw[conv + ".b9"] = fw[conv + ".b9"].copy()
    fw[conv + ".b9"][0] = fw[conv + ".b9"][4]


def _swap(fw, conv):
    w = fw[conv + ".w"].copy()
    w[:, 0, 0], w[:, 0, 1] = fw[conv + ".w"][:, 0, 1], fw[conv + ".w"][:, 0, 0]
    fw[conv + ".w"] = w


FAULTS = {"1 K-step dropped": ("layer2.3.conv1", None, _drop_kstep), "2 corner class": ("layer2.3.conv1", None, _corner),
          "3 stale halo row": ("layer2.3.conv2", _stale, None), "4 taps swapped": ("layer2.3.conv1", None, _swap),
          "5 residual left out": ("layer2.3.conv2", _no_residual, None)}


@pytest.mark.parametrize("fault", ["0 another f32 order"] + sorted(FAULTS))
def test_frobenius_bars_downstream_of_a_fault(fault):
    clean = _layer2_clean()
    if fault.startswith("0"):  # what the bars have to allow: the same stage summed in float32 in another order
        at, tout = "every conv", "layer2.1.prelu"
        bad = SR.chain("layer2", stored("layer2.0", "bf16"), folded("synth"), torch.bfloat16, np.float32, 1)
    else:
        at, plant, edit = FAULTS[fault]
        bad = _layer2_faulty(at, plant, _edited(at, edit) if edit else None)
        tout = [c[4] for c in SR.stage_convs("layer2") if c[0] == at][0]
    assert not np.array_equal(bad[tout], clean[tout]), "nothing was planted"
    whole = {n: _fro(bad[n], clean[n]) for n in LOOKED_AT}
    a, b = bad["layer2.12"], clean["layer2.12"]
    part = max(_fro(a[i:i + 1, r:r + 14], b[i:i + 1, r:r + 14]) for i in range(len(a)) for r in (0, 14))
    print(f"DOWNSTREAM {fault} at {at}: at {tout} {_fro(bad[tout], clean[tout]):.2e}; " +
          ", ".join(f"{n} {v:.2e}" for n, v in whole.items()) + f"; worst image and part of layer2.12 {part:.2e}")
    # the record of the gap: the 2e-2 bars pass a dropped K-step and a wrong corner class; they do see swapped taps
    if fault[0] in "012":
        assert max(whole.values()) < 2e-2 and part < 2e-2, f"{fault}: {whole}, part {part:.3e}"
    if fault[0] == "4":
        assert min(whole.values()) > 2e-2
