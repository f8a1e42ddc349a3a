"""The six hand-scheduled ResNet-50 / InceptionResnetV1 kernels (conv_stem_r50, conv_bneck28, conv_chain_r50,
conv_stem160, conv_chain35, conv_chain .hip) element by element: against the plan's member ops and against the
float64 restatement of tests/fused_ref.py (checked on the CPU by tests/test_fused_ref.py).  test_gpu_chain.py
compares one whole-tensor Frobenius norm, which a wrong halo column or a swapped weight fragment passes.

A  selection weights (fused_ref.selection_state_dict): every stored value is the correctly rounded sum of at most
   two exactly representable terms, so the kernel, the member ops and the restatement must agree value for value.
   Kinds 4, 8, 16, 32 (the stems fold 1/255 and a hi/lo weight split, which is not exact).
B  synthetic weights, all six kinds: slice_stats (worst single element, worst pixel, worst channel, each relative
   to the image's RMS) of the kernel against the rounded float64 restatement is at most twice the member path's.
   Both paths differ from the restatement only by 16-bit roundings that another f32 summation order flips; two such
   orders measure within 1.33x of each other on the CPU (test_fused_ref.py), a one-fragment or one-column fault
   5-10x.

The storage type is the section's (fr_debug_tensor_dtype), not the plan's: the bf16 InceptionResnetV1 plan keeps
conv2d_1a .. repeat_2 in f16, so its three kinds run the f16 kernels under either dtype.

Measured on an MI355X, B = 3, fused / member (ratio) per statistic:

    kind       plan  stored    tensor               element                    pixel                      channel
    stem160    bf16  f16       model.conv2d_3b      7.08e-03 / 5.96e-03 (1.19)  1.65e-03 / 1.73e-03 (0.95)  8.89e-04 / 8.90e-04 (1.00)
    stem160    f16   f16       model.conv2d_3b      7.08e-03 / 5.96e-03 (1.19)  1.65e-03 / 1.73e-03 (0.95)  8.89e-04 / 8.90e-04 (1.00)
    chain35    bf16  f16       model.repeat_1.4     1.00e-02 / 5.53e-03 (1.81)  1.04e-03 / 7.95e-04 (1.31)  8.04e-04 / 6.26e-04 (1.28)
    chain35    f16   f16       model.repeat_1.4     1.00e-02 / 5.53e-03 (1.81)  1.04e-03 / 7.95e-04 (1.31)  8.04e-04 / 6.26e-04 (1.28)
    chain17    bf16  f16       model.repeat_2.9     8.25e-03 / 8.25e-03 (1.00)  7.77e-04 / 7.39e-04 (1.05)  1.43e-03 / 1.46e-03 (0.98)
    chain17    f16   f16       model.repeat_2.9     8.25e-03 / 8.25e-03 (1.00)  7.77e-04 / 7.39e-04 (1.05)  1.43e-03 / 1.46e-03 (0.98)
    stem_r50   bf16  bf16      backbone.maxpool     8.48e-03 / 8.48e-03 (1.00)  1.06e-03 / 1.06e-03 (1.00)  5.25e-04 / 5.25e-04 (1.00)
    stem_r50   f16   f16       backbone.maxpool     2.12e-03 / 2.12e-03 (1.00)  3.75e-04 / 3.75e-04 (1.00)  2.06e-04 / 2.06e-04 (1.00)
    bneck28    bf16  bf16      backbone.layer1.0    1.14e-02 / 6.06e-03 (1.88)  1.11e-03 / 6.58e-04 (1.69)  4.06e-04 / 2.16e-04 (1.88)
    bneck28    bf16  bf16      backbone.layer1.1    2.11e-02 / 2.33e-02 (0.91)  1.68e-03 / 2.38e-03 (0.71)  7.54e-04 / 8.30e-04 (0.91)
    bneck28    bf16  bf16      backbone.layer1.2    2.24e-02 / 2.24e-02 (1.00)  3.82e-03 / 3.08e-03 (1.24)  1.43e-03 / 1.45e-03 (0.98)
    bneck28    f16   f16       backbone.layer1.0    3.03e-03 / 3.03e-03 (1.00)  4.01e-04 / 4.01e-04 (1.00)  1.14e-04 / 1.14e-04 (0.99)
    bneck28    f16   f16       backbone.layer1.1    5.27e-03 / 2.91e-03 (1.81)  5.15e-04 / 4.91e-04 (1.05)  2.19e-04 / 2.64e-04 (0.83)
    bneck28    f16   f16       backbone.layer1.2    5.08e-03 / 5.25e-03 (0.97)  7.47e-04 / 6.88e-04 (1.09)  3.62e-04 / 3.72e-04 (0.97)
    chain_r50  bf16  bf16      backbone.layer3.5    4.08e-02 / 4.08e-02 (1.00)  4.11e-03 / 4.21e-03 (0.98)  6.97e-03 / 6.76e-03 (1.03)
    chain_r50  f16   f16       backbone.layer3.5    7.23e-03 / 9.64e-03 (0.75)  7.35e-04 / 7.16e-04 (1.03)  1.13e-03 / 1.44e-03 (0.79)

The ratios above 1.5 are single elements one or two 16-bit ulps from the restatement where the member ops happen to
hit it: layer1.0 bf16 (1.88 / 1.69 / 1.88) is one element, (img 2, row 3, col 17, ch 228), 1.28125 for 1.28906, one
bf16 ulp -- only 80 of 602,112 elements differ from the member ops at all, so that flip is also the worst pixel and
the worst channel (1.14e-2 / sqrt(784) = 4.06e-4); layer1.1 f16 (1.81) is (img 0, row 3, col 8, ch 39), 2.91992 for
2.92383, and repeat_1.4 (1.81) is (img 1, row 6, col 7, ch 201), 4.07422 for 4.06641 (member ops 4.07031): two f16
ulps each, one flipped rounding in each of two blocks carried along the residual stream.  The kernels sum K in
another order than the member ops (conv_bneck28.hip conv1 reads the x planes s + 8 lg, conv3 and conv_chain35.hip
P4 accumulate onto bias + x), so sums next to a rounding tie fall the other way; their pixel and channel
statistics, which average over 256 channels / 289-784 pixels, stay within 1.31x.
"""
import ctypes

import numpy as np
import pytest
import torch

from facerecognition_amd import _native as N
from tests import fused_ref as FR

pytestmark = pytest.mark.gpu

B = 3  # the geometry is the model's; three images keep the image index live
SEED = {"resnet50_arcface": 29, "irv1_facenet": 13}
ARCH_KINDS = {a: [k for k, v in FR.KINDS.items() if v[0] == a] for a in ("resnet50_arcface", "irv1_facenet")}
EXACT_KINDS = ("bneck28", "chain_r50", "chain35", "chain17")
CASES = [(k, dt) for a in sorted(ARCH_KINDS) for k in ARCH_KINDS[a] for dt in ("bf16", "f16")]


def _plan(m):
    buf = ctypes.create_string_buffer(1 << 20)
    N.check(N.lib().fr_debug_plan(m.handle, B, buf, len(buf)), "fr_debug_plan")
    return buf.value.decode()


def _tensors(m, names):
    """{name: (NHWC values as float64 on the CPU, storage dtype)}"""
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
        out[name] = (buf.cpu().double(), dt)
    missing = set(names) - set(out)
    assert not missing, f"no plan tensor named {sorted(missing)}"
    return out


def _make_runs(arch, dtype, which):
    """One model, the member path once (FR_OPT_STAGE 0), then each of the arch's kinds alone (FR_OPT_STAGE 2 with
    its single FR_OPT_FUSED_MASK bit).  {"u8", "fw", "member": tensors, kind: tensors}; shared by the tests."""
    from facerecognition_amd.model import FRModel
    from facerecognition_amd.synthetic import synthetic_crops
    from facerecognition_amd.weights import INPUT_SIZE, fold_state_dict, synth_state_dict
    sd = synth_state_dict(arch) if which == "synth" else FR.selection_state_dict(arch, 0)
    u8 = synthetic_crops(B, INPUT_SIZE[arch], seed=SEED[arch])
    x = torch.from_numpy(u8)
    kinds = ARCH_KINDS[arch]
    names = {n for k in kinds for n in ((FR.KINDS[k][2],) if FR.KINDS[k][2] else ()) + FR.KINDS[k][3]}
    m = FRModel(arch, sd, dtype=dtype)
    try:
        m.set_option(N.FR_OPT_STAGE, 0)
        plan = _plan(m)
        for k in kinds:
            assert FR.PLAN_MARK[k] not in plan, f"member run: the plan holds the {k} kernel"
        m.embed(x)
        out = {"u8": u8, "fw": fold_state_dict(arch, sd), "member": _tensors(m, names)}
        m.set_option(N.FR_OPT_STAGE, 2)
        for k in kinds:
            m.set_option(N.FR_OPT_FUSED_MASK, FR.KINDS[k][1])
            plan = _plan(m)
            assert FR.PLAN_MARK[k] in plan, f"{k}: mask {FR.KINDS[k][1]} does not plan its kernel"
            for o in kinds:
                assert o == k or FR.PLAN_MARK[o] not in plan, f"{k}: the plan also holds the {o} kernel"
            m.embed(x)
            out[k] = _tensors(m, names)
    finally:
        m.close()
    return out


@pytest.fixture(scope="module")
def runs(gpu):
    """runs(arch, dtype, which): _make_runs once per module, shared by the kinds of an arch x dtype."""
    cache = {}

    def get(arch, dtype, which):
        if (arch, dtype, which) not in cache:
            cache[arch, dtype, which] = _make_runs(arch, dtype, which)
        return cache[arch, dtype, which]

    yield get
    cache.clear()


def _reference(run, kind):
    """The member run's input of the kind (the stems: the crops), its storage dtype, the rounded restatement."""
    _, _, tin, touts = FR.KINDS[kind]
    dt = run["member"][touts[0]][1]
    for n in touts + ((tin,) if tin else ()):  # one storage type per group (run_stage: the kernel's)
        assert run["member"][n][1] == dt and run[kind][n][1] == dt
    xin = run["u8"] if tin is None else run["member"][tin][0]
    return dt, FR.RESTATE[kind](xin, run["fw"], dt)


def _mismatch(a, b, what):
    bad = (a != b).nonzero()
    rows = "; ".join(f"(img {i}, row {r}, col {c}, ch {ch}): {a[i, r, c, ch].item():.6g} vs {b[i, r, c, ch].item():.6g}"
                     for i, r, c, ch in bad[:6].tolist())
    return f"{what}: {len(bad)} of {a.numel()} elements differ, first {rows}"


@pytest.mark.parametrize("kind,dtype", [c for c in CASES if c[0] in EXACT_KINDS])
def test_selection_weights_value_exact(runs, kind, dtype):
    """A: with selection weights the kernel's outputs equal the member ops' and the rounded float64 restatement's,
    value for value (-0 = +0)."""
    arch, _, tin, touts = FR.KINDS[kind]
    run = runs(arch, dtype, "selection")
    assert torch.equal(run[kind][tin][0], run["member"][tin][0]), f"{kind}: the input {tin} differs between the runs"
    dt, ref = _reference(run, kind)
    fails = []
    for n in touts:
        y, ym, r = run[kind][n][0], run["member"][n][0], ref[n]
        assert y.shape == r.shape and torch.isfinite(r).all()
        frac = (r != 0).double().mean().item()
        print(f"{kind} {dtype} ({dt}) {n}: nonzero {frac:.3f}, max {r.max().item():.5g}")
        assert frac >= 0.5, f"{n}: the restatement is mostly zero ({frac:.3f}): the equality would be vacuous"
        for a, b, what in ((y, r, f"{n}: kernel vs float64 restatement"), (y, ym, f"{n}: kernel vs member ops"),
                           (ym, r, f"{n}: member ops vs float64 restatement")):
            if not torch.equal(a, b):
                fails.append(_mismatch(a, b, what))
    assert not fails, f"{kind} {dtype}:\n" + "\n".join(fails)


@pytest.mark.parametrize("kind,dtype", CASES)
def test_synthetic_weights_elementwise(runs, kind, dtype):
    """B: with the synthetic weights no element, pixel or channel of the kernel's output is further from the
    rounded float64 restatement than twice the member path's worst."""
    arch, _, tin, touts = FR.KINDS[kind]
    run = runs(arch, dtype, "synth")
    if tin is not None:
        assert torch.equal(run[kind][tin][0], run["member"][tin][0]), f"{kind}: the input {tin} differs between the runs"
    dt, ref = _reference(run, kind)
    fails = []
    for n in touts:
        sf = FR.slice_stats(run[kind][n][0], ref[n])
        sm = FR.slice_stats(run["member"][n][0], ref[n])
        print(f"STATS {kind} {dtype} ({str(dt)[6:]}) {n}: " + "  ".join(
            f"{lab} {f:.2e} / {mm:.2e} ({f / mm if mm else float('nan'):.2f})" for lab, f, mm in zip(("elem", "pixel", "channel"), sf, sm)))
        y, ym, r = run[kind][n][0], run["member"][n][0], ref[n]
        i, row, col, ch = np.unravel_index(int(((y - r).abs() / r.pow(2).mean(dim=(1, 2, 3), keepdim=True).sqrt()).argmax()), r.shape)
        ulp = (r[i, row, col, ch].to(dt).view(torch.int16) + 1).view(dt).double() - r[i, row, col, ch]
        print(f"      worst element (img {i}, row {row}, col {col}, ch {ch}): restatement {r[i, row, col, ch].item():.6g}, kernel "
              f"{y[i, row, col, ch].item():.6g}, member ops {ym[i, row, col, ch].item():.6g}, one ulp {ulp.item():.3g}; "
              f"{(y != ym).sum().item()} of {y.numel()} elements differ from the member ops")
        for lab, f, mm in zip(("element", "pixel", "channel"), sf, sm):
            if not f <= 2 * mm:
                fails.append(f"{n}: worst {lab} error {f:.3e} against the member path's {mm:.3e}")
    assert not fails, f"{kind} {dtype}:\n" + "\n".join(fails)
