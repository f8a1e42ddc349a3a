"""The four hand-scheduled IResNet100 kernels -- the layer3 LDS-resident stage (conv_stage.hip), the layer2 / layer1
split stages (conv_split_stage.hip) with the tail convs layer3.0.conv1 / layer4.0.conv1 they run on their final patch,
and the fused layer1.0 transition (conv_trans.hip) -- conv by conv and element by element against the float64
restatement of tests/stage_ref.py (checked on the CPU by tests/test_stage_ref.py).  test_gpu_stage.py and
test_gpu_trans.py compare these kernels with the per-conv path alone, one Frobenius norm per tensor or 14-row part,
which a dropped K-step and a wrong border class of b9 at a corner pass, and a stale halo row in one image of a batch
passes in all but the per-part test (test_stage_ref.py measures it); and they cannot see a fault the two paths share
(the fold, the b9 table, the packed weights).

A  synthetic weights, FR_OPT_KEEP_INTERMEDIATES, B = 9 (the smallest batch that puts the split stages' workgroups
   into a second, padded group of eight): every conv of every stage, tails included, from its own stored input:
   |stored - float64| <= the float32 bound of stage_ref.conv_ref, for images 0, 4 and 8.  No tolerance is chosen.
B  selection weights (stage_ref.selection_state_dict) on the production path (no intermediates kept, so the
   transition kernel runs): every stored value is the correctly rounded sum of at most two exactly representable terms,
   so the fused run, the member run and the free-running restatement must agree value for value.
C  synthetic weights, the transition: slice_stats (worst element, pixel, channel, relative to the image's RMS) of
   layer1.0 against the rounded restatement is at most twice the member path's.  Both differ from the restatement only
   by 16-bit roundings that another f32 summation order flips (test_stage_ref.py: no two of four orders more than 2x
   apart, the element statistic moving in steps of one storage ulp; a one-fragment or one-column fault 50x or more).

The e4m3 stage (conv_stage8.hip) and the e4m3 convs are held the same way by tests/test_gpu_fp8_exact.py (tests/fp8_ref.py).
Not covered: the layer3 variants 1-3 (bit-identical to the
default by test_gpu_stage.py::test_stage_variants_bit_identical), and batch sizes whose only difference is the grid.

Measured on an MI355X.  A, B = 9, images 0, 4, 8: the largest |stored - float64| / bound per stage, kind of conv and
storage type, with the conv that has it (the largest possible for a correctly rounded result is 1 at a rounding tie
of an element whose accumulation term is negligible):

    stage   dtype  conv1                     conv2                      tail
    layer1  bf16   0.941 (layer1.1.conv1)    0.977 (layer1.1.conv2)     -
    layer1  f16    0.709 (layer1.2.conv1)    0.887 (layer1.2.conv2)     -
    layer2  bf16   0.876 (layer2.7.conv1)    0.966 (layer2.12.conv2)    0.876 (layer3.0.conv1)
    layer2  f16    0.527 (layer2.9.conv1)    0.808 (layer2.7.conv2)     0.580 (layer3.0.conv1)
    layer3  bf16   0.753 (layer3.20.conv1)   0.938 (layer3.23.conv2)    0.715 (layer4.0.conv1)
    layer3  f16    0.314 (layer3.24.conv1)   0.687 (layer3.20.conv2)    0.261 (layer4.0.conv1)

The CPU's float32 evaluations of test_stage_ref.py measure 0.976 / 0.852 / 0.916 / 0.711 (bf16) on one conv of each
geometry: the kernels sit where legitimate float32 arithmetic sits.  Under both storage types the plan holds no conv
line for layer3.0.prelu or layer4.0.prelu: the stages write both tails.

B: every tensor equal, value for value, in all three comparisons, bf16 and f16; the groups' inputs (prelu, layer1.0,
layer2.0, layer3.0) are equal between the fused and the member run, so one restatement serves both.

C, B = 3, layer1.0, fused / member (ratio):

    dtype  element                      pixel                        channel
    bf16   1.39e-02 / 1.56e-02 (0.89)   1.74e-03 / 2.19e-03 (0.80)   2.49e-04 / 2.79e-04 (0.89)
    f16    1.95e-03 / 1.95e-03 (1.00)   2.50e-04 / 2.59e-04 (0.96)   4.74e-05 / 4.41e-05 (1.08)

bf16: 305 of 602,112 elements differ from the member ops, the worst element (img 0, row 42, col 52, ch 6) is -2.82812
for -2.84375 in both paths, one bf16 ulp; f16: 2,568 differ, the worst (img 2, row 1, col 26, ch 41) is -2.11719 for
-2.11523, one f16 ulp.
"""
import ctypes

import numpy as np
import pytest
import torch

from facerecognition_amd import _native as N
from tests import stage_ref as SR

pytestmark = pytest.mark.gpu

ARCH = SR.ARCH
BA, IMGS = 9, (0, 4, 8)  # A and B: the batch, and the images held against the (per-image) reference
BC = 3                   # C
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
TAILS = ("layer3.0.prelu", "layer4.0.prelu")
# B: group -> (input tensor, output tensors)
GROUPS = {"trans": ("prelu", ("layer1.0",)), "layer1": ("layer1.0", ("layer1.2",)),
          "layer2": ("layer2.0", ("layer2.12", "layer3.0.prelu")), "layer3": ("layer3.0", ("layer3.29", "layer4.0.prelu"))}


def _plan(m, B):
    buf = ctypes.create_string_buffer(1 << 20)
    N.check(N.lib().fr_debug_plan(m.handle, B, buf, len(buf)), "fr_debug_plan")
    return buf.value.decode()


def _tensors(m, B, names, images=None):
    """{name: the stored values [len(images), H, W, C] as float64 numpy (all B images without `images`)}"""
    L, out = N.lib(), {}
    for t in range(L.fr_debug_tensor_count(m.handle)):
        name = L.fr_debug_tensor_name(m.handle, t).decode()
        if name not in names:
            continue
        dt = torch.float16 if L.fr_debug_tensor_dtype(m.handle, t) == N.FR_DTYPE_F16 else torch.bfloat16
        H, W, C = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        N.check(L.fr_debug_tensor_shape(m.handle, t, ctypes.byref(H), ctypes.byref(W), ctypes.byref(C)))
        buf = torch.empty((B, H.value, W.value, C.value), dtype=dt, device="cuda")
        N.check(L.fr_debug_copy_tensor(m.handle, t, B, buf.data_ptr(), N.stream_ptr()))
        torch.cuda.synchronize()
        buf = buf.cpu()
        out[name] = (buf if images is None else buf[list(images)]).double().numpy()
    missing = set(names) - set(out)
    assert not missing, f"no plan tensor named {sorted(missing)}"
    return out


def _stage_lines(plan):
    return [ln for ln in plan.splitlines() if ln.startswith("stage ")]


def _synth_runs(dtype):
    """One model with the synthetic weights: A's forward (intermediates kept), then C's fused and member forwards."""
    from facerecognition_amd.model import FRModel
    from facerecognition_amd.synthetic import synthetic_crops
    from facerecognition_amd.weights import fold_state_dict, synth_state_dict
    sd = synth_state_dict(ARCH)
    m = FRModel(ARCH, sd, dtype=dtype)
    out = {"fw": fold_state_dict(ARCH, sd)}
    try:
        m.set_option(N.FR_OPT_KEEP_INTERMEDIATES, 1)
        m.set_option(N.FR_OPT_STAGE, 2)
        out["plan"] = _plan(m, BA)
        m.embed(torch.from_numpy(synthetic_crops(BA, 112, seed=91)))
        out["timeouts"] = N.lib().fr_debug_stage_timeouts(m.handle)
        out["A"] = _tensors(m, BA, {n for s in SR.STAGES for n in SR.stage_tensors(s)}, IMGS)
        m.set_option(N.FR_OPT_KEEP_INTERMEDIATES, 0)
        xc = torch.from_numpy(synthetic_crops(BC, 112, seed=92))
        out["plan_fused"] = _plan(m, BC)
        m.embed(xc)
        out["fused"] = _tensors(m, BC, {"prelu", "layer1.0"})
        m.set_option(N.FR_OPT_STAGE, 0)
        out["plan_member"] = _plan(m, BC)
        m.embed(xc)
        out["member"] = _tensors(m, BC, {"prelu", "layer1.0"})
    finally:
        m.close()
    return out


def _selection_runs(dtype):
    """One model with the selection weights on the production path: the fused run (FR_OPT_STAGE 2), then the member
    run (0), at B = 9."""
    from facerecognition_amd.model import FRModel
    from facerecognition_amd.synthetic import synthetic_crops
    from facerecognition_amd.weights import fold_state_dict
    sd = SR.selection_state_dict(0)
    names = {n for tin, touts in GROUPS.values() for n in (tin,) + touts}
    m = FRModel(ARCH, sd, dtype=dtype)
    out = {"fw": fold_state_dict(ARCH, sd)}
    x = torch.from_numpy(synthetic_crops(BA, 112, seed=93))
    try:
        assert m.get_option(N.FR_OPT_KEEP_INTERMEDIATES) == 0
        for mode, key in ((2, "fused"), (0, "member")):
            m.set_option(N.FR_OPT_STAGE, mode)
            out["plan_" + key] = _plan(m, BA)
            m.embed(x)
            out[key] = _tensors(m, BA, names)
        out["timeouts"] = N.lib().fr_debug_stage_timeouts(m.handle)
    finally:
        m.close()
    return out


@pytest.fixture(scope="module")
def runs(gpu):
    """runs(which, dtype): the forwards of _synth_runs / _selection_runs, once per module."""
    cache = {}

    def get(which, dtype):
        if (which, dtype) not in cache:
            cache[which, dtype] = (_synth_runs if which == "synth" else _selection_runs)(dtype)
        return cache[which, dtype]

    yield get
    cache.clear()


def _assert_stages_planned(plan, dtype):
    lines = _stage_lines(plan)
    for stage, last in SR.PLAN_END.items():
        assert any(ln.endswith(" " + last) for ln in lines), f"{stage}: no stage line ending in {last}:\n{plan}"
    # a tail conv that the stage computes is a member of the stage op: its own conv line leaves the plan
    own = [t for t in TAILS if any(ln.startswith("conv ") and ln.endswith(" " + t) for ln in plan.splitlines())]
    if dtype == "bf16":
        assert not own, f"the tail convs {own} run as convs of their own, not on the stage's final patch"
    return own


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("stage", sorted(SR.STAGES))
def test_every_stage_conv_within_its_bound(runs, stage, dtype):
    """A: every conv of the stage, from its stored input, within the float32 bound of its float64 restatement."""
    run = runs("synth", dtype)
    own = _assert_stages_planned(run["plan"], dtype)
    assert run["timeouts"] == 0
    dt, fw, t = DT[dtype], run["fw"], run["A"]
    worst, fails = {}, []
    for conv, kind, tin, tres, tout in SR.stage_convs(stage):
        y = t[tout]
        assert np.array_equal(y, SR.rnd(y, dt)), f"{tout} is not stored as {dtype}"
        ref, bound = SR.conv_ref(t[tin], fw, conv, kind, dt, None if tres is None else t[tres])
        assert y.shape == ref.shape and np.isfinite(ref).all() and np.isfinite(y).all()
        r = SR.ratio(y, ref, bound)
        i, row, col, ch = np.unravel_index(int(r.argmax()), r.shape)
        if r[i, row, col, ch] > worst.get(kind, (0.0,))[0]:
            worst[kind] = (float(r[i, row, col, ch]), conv)
        if r[i, row, col, ch] > 1:
            fails.append(f"{conv} ({kind}): {np.count_nonzero(r > 1)} of {r.size} elements outside the bound, worst image "
                         f"{IMGS[i]}, row {row}, col {col}, channel {ch} (part {row // 14}): stored {y[i, row, col, ch]:.8g}, "
                         f"float64 {ref[i, row, col, ch]:.8g}, bound {bound[i, row, col, ch]:.3g} (ratio {r[i, row, col, ch]:.3g})")
    print(f"RATIO {stage} {dtype}: " + "  ".join(f"{k} {v[0]:.3f} ({v[1]})" for k, v in sorted(worst.items())) +
          (f"  [convs of their own: {own}]" if own else ""))
    assert not fails, f"{stage} {dtype}:\n" + "\n".join(fails[:12])


def _mismatch(a, b, what, images):
    bad = np.argwhere(a != b)
    rows = "; ".join(f"(img {images[i]}, row {r}, col {c}, ch {ch}, part {r // 14}): {a[i, r, c, ch]:.6g} vs {b[i, r, c, ch]:.6g}"
                     for i, r, c, ch in bad[:6].tolist())
    return f"{what}: {len(bad)} of {a.size} elements differ, first {rows}"


def _restate(group, x, fw, dt):
    return SR.transition(x, fw, dt) if group == "trans" else SR.chain(group, x, fw, dt)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("group", list(GROUPS))
def test_selection_weights_value_exact(runs, group, dtype):
    """B: with selection weights the kernels' outputs equal the member ops' (all nine images) and the rounded float64
    restatement run free over the group from the member run's stored input (images 0, 4, 8), value for value
    (-0 = +0)."""
    run = runs("selection", dtype)
    fused, member, dt = run["fused"], run["member"], DT[dtype]
    _assert_stages_planned(run["plan_fused"], dtype)
    assert "trans " in run["plan_fused"] and "trans " not in run["plan_member"]
    assert not _stage_lines(run["plan_member"])
    for t in TAILS:
        assert any(ln.startswith("conv ") and ln.endswith(" " + t) for ln in run["plan_member"].splitlines()), t
    assert run["timeouts"] == 0
    tin, touts = GROUPS[group]
    every = list(range(BA))
    fails = []
    for n in touts:
        if not np.array_equal(fused[n], member[n]):
            fails.append(_mismatch(fused[n], member[n], f"{n}: kernel vs member ops", every))
    same_input = np.array_equal(fused[tin], member[tin])
    refs = {"member": _restate(group, member[tin][list(IMGS)], run["fw"], dt)}
    # the stem and the strided .0 blocks between the groups run the same kernels in both runs; where their outputs
    # differ all the same, each run is held against the restatement from its own input
    refs["fused"] = refs["member"] if same_input else _restate(group, fused[tin][list(IMGS)], run["fw"], dt)
    if not same_input:
        print(f"{group} {dtype}: " + _mismatch(fused[tin], member[tin], f"the input {tin} differs between the runs", every))
    for n in touts:
        r = refs["member"][n]
        frac = float((r != 0).mean())
        print(f"{group} {dtype} {n}: nonzero {frac:.3f}, max |value| {np.abs(r).max():.5g}")
        assert np.isfinite(r).all() and frac >= 0.5, f"{n}: the restatement is mostly zero ({frac:.3f}): the equality would be vacuous"
        for key, got in (("fused", fused), ("member", member)):
            if not np.array_equal(got[n][list(IMGS)], refs[key][n]):
                fails.append(_mismatch(got[n][list(IMGS)], refs[key][n], f"{n}: {key} run vs float64 restatement", IMGS))
    assert not fails, f"{group} {dtype}:\n" + "\n".join(fails)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_transition_elementwise(runs, dtype):
    """C: with the synthetic weights no element, pixel or channel of the transition kernel's layer1.0 is further from
    the rounded float64 restatement than twice the member path's worst."""
    run = runs("synth", dtype)
    assert "trans " in run["plan_fused"] and "trans " not in run["plan_member"]
    dt = DT[dtype]
    assert np.array_equal(run["fused"]["prelu"], run["member"]["prelu"]), "the stem's output differs between the runs"
    y, ym = run["fused"]["layer1.0"], run["member"]["layer1.0"]
    r = SR.transition(run["member"]["prelu"], run["fw"], dt)["layer1.0"]
    sf, sm = SR.slice_stats(y, r), SR.slice_stats(ym, r)
    print(f"STATS trans {dtype} layer1.0: " + "  ".join(
        f"{lab} {f:.2e} / {mm:.2e} ({f / mm if mm else float('nan'):.2f})" for lab, f, mm in zip(("elem", "pixel", "channel"), sf, sm)))
    rms = np.sqrt((r ** 2).mean(axis=(1, 2, 3), keepdims=True))
    i, row, col, ch = np.unravel_index(int((np.abs(y - r) / rms).argmax()), r.shape)
    v = torch.tensor(r[i, row, col, ch]).to(dt)
    ulp = (v.view(torch.int16) + 1).view(dt).double().item() - v.double().item()
    print(f"      worst element (img {i}, row {row}, col {col}, ch {ch}): restatement {r[i, row, col, ch]:.6g}, kernel "
          f"{y[i, row, col, ch]:.6g}, member ops {ym[i, row, col, ch]:.6g}, one ulp {ulp:.3g}; "
          f"{np.count_nonzero(y != ym)} of {y.size} elements differ from the member ops")
    fails = [f"worst {lab} error {f:.3e} against the member path's {mm:.3e}"
             for lab, f, mm in zip(("element", "pixel", "channel"), sf, sm) if not f <= 2 * mm]
    assert not fails, f"transition {dtype}:\n" + "\n".join(fails)
