"""CPU checks of tests/fp8_ref.py, before a GPU sees it: the scale exponent and the e4m3 quantisation against the
format's own definition, the per-element bound of one e4m3 conv against legitimate float32 arithmetic, the faults the
e4m3 kernels can have, planted at the shapes tests/test_gpu_fp8_exact.py runs (tests/fp8_op.py), and the e4m3 stage's
restatement chain8: its selection weights quantise to the e4m3 value 448 with power-of-two scales, its ambiguity rule
stays within the cap on a random input, and a dropped K-step, a corner border class, a stale halo row in one image and
an exponent taken from another image each break the equality outside the excluded set."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import fp8_op as OP
from tests import fp8_ref as R

BF16 = torch.bfloat16


# ---- the scale exponent
@pytest.mark.parametrize("k", [-3, 0, 5])
def test_act_exp_at_the_boundary(k):
    for clamp in (R.CLAMP_CONV, R.CLAMP_STAGE):
        assert R.act_exp(np.float32(448 * 2.0 ** k), clamp) == k
        assert R.act_exp(np.float32(450 * 2.0 ** k), clamp) == k + 1       # the next bf16 above
        assert R.act_exp(np.float32(446 * 2.0 ** k), clamp) == k           # the next bf16 below
        assert R.act_exp(np.nextafter(np.float32(448 * 2.0 ** k), np.float32(np.inf)), clamp) == k + 1


def test_act_exp_is_the_smallest_exponent():
    assert R.act_exp(0.0, 60) == 0 and R.act_exp(np.float32(0), 100) == 0
    rng = np.random.default_rng(0)
    a = np.abs(rng.standard_normal(2000) * 2.0 ** rng.integers(-40, 40, 2000)).astype(np.float32)
    for v in a[a > 0]:
        e = R.act_exp(v, 100)
        assert Fraction(float(v)) <= 448 * Fraction(2) ** e and Fraction(float(v)) > 448 * Fraction(2) ** (e - 1)
    assert R.act_exp(np.float32(1e30), 60) == 60 and R.act_exp(np.float32(1e-30), 60) == -60
    assert R.act_exp(np.float32(1e30), 100) == 91 and R.act_exp(np.float32(1e-45), 100) == -100


# ---- the quantisation: all 256 codes and their midpoints
@pytest.mark.parametrize("e", [0, -3, 6])
def test_quant_every_code_and_midpoint(e):
    codes = np.arange(256, dtype=np.uint8)
    val = R.decode(codes)
    fin = np.isfinite(val)
    assert fin.sum() == 254 and len(R.GRID) == 253 and R.GRID[0] == -448 and R.GRID[-1] == 448
    # the format itself: sign, 4 exponent bits (bias 7), 3 mantissa bits, subnormals at exponent 0
    for c in codes[fin]:
        ex, m = (int(c) >> 3) & 15, int(c) & 7
        mag = m * 2.0 ** -9 if ex == 0 else (8 + m) * 2.0 ** (ex - 10)
        assert val[c] == (-mag if c & 0x80 else mag)
    s = 2.0 ** e
    q, lo, hi = R.quant(val[fin] * s, e)
    assert np.array_equal(q, val[fin] * s)                                  # every code is a fixed point
    k = np.searchsorted(R.GRID, val[fin])
    assert np.array_equal(lo, R.GRID[np.maximum(k - 1, 0)] * s) and np.array_equal(hi, R.GRID[np.minimum(k + 1, 252)] * s)
    # midpoints of neighbours: to the neighbour whose code is even; a float32 step off the midpoint: to the nearer
    a, b = R.GRID[:-1], R.GRID[1:]
    mid = (a + b) / 2
    even = np.where(R.encode(a) & 1, b, a)
    assert np.all(((R.encode(a) & 1) != (R.encode(b) & 1)) | (a * b == 0))
    even[a == 0], even[b == 0] = 0.0, 0.0                                   # +-2^-10: to zero (code 0 is even)
    assert np.array_equal(R.quant(mid * s, e)[0], even * s)
    m32 = mid.astype(np.float32)
    assert np.array_equal(m32.astype(np.float64), mid)
    up, down = np.nextafter(m32, np.float32(np.inf)).astype(np.float64), np.nextafter(m32, np.float32(-np.inf)).astype(np.float64)
    assert np.array_equal(R.quant(up * s, e)[0], b * s) and np.array_equal(R.quant(down * s, e)[0], a * s)
    # flush below 2^-10, and the fault's rounding differs from RNE exactly on the ties that RNE sends towards zero
    assert R.quant(np.array([2.0 ** -10, -2.0 ** -10, 2.0 ** -11]) * s, e)[0].tolist() == [0, 0, 0]
    away = R.quant_half_away(mid * s, e)
    assert np.array_equal(away, np.where(mid > 0, b, a) * s)
    assert np.array_equal(R.quant_half_away(val[fin] * s, e), val[fin] * s)


def test_general_conv_sum_agrees_with_stage_ref():
    """fp8_ref.conv_sum's own loop (non-square taps, no padding) against stage_ref.conv_sum where both apply."""
    rng = np.random.default_rng(3)
    I, w = rng.standard_normal((2, 5, 6, 64)), rng.standard_normal((8, 3, 3, 64))
    from tests import stage_ref as SR
    want = SR.conv_sum(I, w, 1)
    Ip = np.zeros((2, 7, 8, 64))
    Ip[:, 1:6, 1:7] = I
    got = R.conv_sum(Ip, w, (1, 1), (0, 0))  # the general path: explicit padding
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    g32 = R.conv_sum(Ip, w, (1, 1), (0, 0), np.float32)
    assert g32.dtype == np.float32 and np.array_equal(g32, SR.conv_sum(I, w, 1, np.float32))


# ---- the bound
# one case of each geometry
FLOAT32_CASES = ["b9-prelu-ys-y2-s64", "none-res-xs-y2-s64", "b9-relu-res-xs-ys-y2-s64-over", "b-res-s64", "none-prelu-xs-ys-y2"]


def _f32_eval(c, perm=None, **over):
    _, _, _, Cin, Cout, _, _, stride, pad = c["geom"]
    args = dict(c["ref_args"])
    e = over.pop("e", c["e"])
    codes = over.pop("codes", c["codes"])
    args.update(over)
    return R.conv_ref(c["xv"], codes, c["wscale"][:Cout].double().numpy(), e, stride, pad, compute=np.float32, perm=perm, **args)


def _f64_rounded(c, **over):
    """The case recomputed in float64 with something replaced, rounded to bf16: (y, y2 or None)."""
    _, _, _, Cin, Cout, _, _, stride, pad = c["geom"]
    args = dict(c["ref_args"])
    e = over.pop("e", c["e"])
    codes = over.pop("codes", c["codes"])
    args.update(over)
    out = R.conv_ref(c["xv"], codes, c["wscale"][:Cout].double().numpy(), e, stride, pad, **args)
    return R.rnd(out[0], BF16), (R.rnd(out[2], BF16) if len(out) == 4 else None)


@pytest.mark.parametrize("name", FLOAT32_CASES)
def test_bound_holds_for_float32_orders(name):
    c = OP.case(name)
    assert np.isfinite(c["ref"]).all() and (c["bound"] > 0).all()
    Cin = c["geom"][3]
    outs = []
    for perm in (None, np.random.default_rng(1).permutation(Cin)):
        v, v2 = _f32_eval(c, perm)
        outs.append(v)
        r = R.ratio(R.rnd(v, BF16), c["ref"], c["bound"]).max()
        r2 = R.ratio(R.rnd(v2, BF16), c["ref2"], c["bound2"]).max() if v2 is not None else 0.0
        print(f"FLOAT32 {name} order {len(outs)}: largest error / bound y {r:.3f}, y2 {r2:.3f}")
        assert r <= 1 and r2 <= 1, f"{name}: a legitimate float32 evaluation is outside the bound ({r:.3f}, {r2:.3f})"
    assert not np.array_equal(outs[0], outs[1]), "the two evaluations are the same order"


def test_input_has_subnormals_and_ties():
    """The cases' inputs: a real share in e4m3's subnormal range and one eighth on exact ties."""
    c = OP.case("b9-prelu-ys-y2-s64")
    x, e = c["xv"], c["e"]
    q, lo, hi = R.quant(x, e)
    sub = (np.abs(x) < 2.0 ** (e - 6)) & (x != 0)
    tie = (np.abs(x - q) * 2 == np.minimum(hi - q, q - lo)) & (x != q)
    print(f"INPUT share subnormal {sub.mean():.3f}, ties {tie.mean():.3f}, flushed {((q == 0) & (x != 0)).mean():.3f}")
    assert sub.mean() >= 0.1 and tie.mean() >= 0.1


# ---- the planted faults, at the shapes of test_gpu_fp8_exact.py.  `clean` is the rounded float64 result (ratio <= 1
# by construction); each fault must leave at least one element outside the bound.  Measured largest ratio over the seven
# cases with a nonzero input (smallest .. largest; the smallest is always 3000 randn or the K = 1728 conv):
#   dropped 64-channel chunk of one tap   43.6 .. 8540
#   corner pixel with an edge class       169, 224 (the two bias9 cases; 66 and 70 of the pixel's channels)
#   res_off + 8                           443 .. 14400
#   e + 1                                 0.286 .. 0.953: not seen by a conv; the converter table sees 752 values
#   round half away                       3.41 (3000 randn: ties only where forced) .. 614
#   output fragments swapped              154 .. 15800
# The float32 evaluations (both orders) measure 0.577 .. 0.953 for y and 0.767 .. 0.962 for y2.
def _report(what, name, r):
    print(f"FAULT {what} [{name}]: largest ratio {r.max():.3g}, {np.count_nonzero(r > 1)} of {r.size} elements outside the bound")


def _every_case():
    return [OP.case(n) for n in sorted(OP.CASES) if OP.CASES[n][1].get("input") != "zero"]


def test_fault_dropped_chunk():
    """One 64-channel chunk of one tap missing from the sum."""
    for c in _every_case():
        codes = c["codes"].copy()
        kh, kw = codes.shape[1:3]
        codes[:, kh // 2, kw - 1, -64:] = 0
        y, _ = _f64_rounded(c, codes=codes)
        r = R.ratio(y, c["ref"], c["bound"])
        _report("dropped 64-channel chunk", c["name"], r)
        assert r.max() > 1


def test_fault_corner_class():
    """The corner pixel (0, 0) of image 1 with the top edge's row of bias9."""
    n = 0
    for c in _every_case():
        b9 = c["ref_args"]["bias9"]
        if b9 is None:
            continue
        n += 1
        wrong = b9.copy()
        wrong[0] = b9[1]
        y, y2 = _f64_rounded(c, bias9=wrong)
        f = R.rnd(c["ref"], BF16)
        f[1, 0, 0] = y[1, 0, 0]
        r = R.ratio(f, c["ref"], c["bound"])
        _report("corner pixel with an edge class", c["name"], r)
        assert r[1, 0, 0].max() > 1 and np.count_nonzero(r > 1) == np.count_nonzero(r[1, 0, 0] > 1)
    assert n >= 2


def test_fault_res_off():
    """The residual read 8 channels further on."""
    n = 0
    for c in _every_case():
        if "res" not in c:
            continue
        n += 1
        Cout = c["geom"][4]
        y, _ = _f64_rounded(c, res=c["res"][..., 16:16 + Cout].double().numpy())
        r = R.ratio(y, c["ref"], c["bound"])
        _report("res_off + 8", c["name"], r)
        assert r.max() > 1
    assert n >= 3


def test_fault_exponent_one_too_large():
    """e + 1.  The normal e4m3 grid is the same at every power-of-two scale, so the fault moves only the values that
    e sends into the subnormal range or below the flush, which are small in any sum: no case reaches a ratio of 1
    (printed below; with u_acc = u two of the seven reached 1.31 and 2.09, 7 elements each).  The converter table
    (tests/fp8_op.table) is the check that sees this fault, exactly and for every input."""
    for c in _every_case():
        y, _ = _f64_rounded(c, e=c["e"] + 1)
        _report("e + 1", c["name"], R.ratio(y, c["ref"], c["bound"]))
    for a in OP.TABLE_AMAX:
        t = OP.table(a)
        wrong = 0.875 * t["sign"] * R.quant(t["xv"], t["e"] + 1)[0]
        print(f"FAULT e + 1 [table {a:g}]: {np.count_nonzero(wrong != t['want'])} of {wrong.size} values differ")
        assert np.count_nonzero(wrong != t["want"]) >= 256  # at least the binade that e + 1 makes subnormal, both signs


def test_fault_round_half_away():
    """Ties of the activation quantisation rounded away from zero."""
    for c in _every_case():
        y, _ = _f64_rounded(c, quantize=R.quant_half_away)
        r = R.ratio(y, c["ref"], c["bound"])
        _report("round half away", c["name"], r)
        assert r.max() > 1
    t = OP.table(448.0)
    wrong = 0.875 * t["sign"] * R.quant_half_away(t["xv"], t["e"])
    assert np.count_nonzero(wrong != t["want"]) > 50


def test_fault_fragment_swapped():
    """A 16-channel output fragment stored in its neighbour's place."""
    for c in _every_case():
        f = R.rnd(c["ref"], BF16)
        f[..., 16:32], f[..., 32:48] = f[..., 32:48].copy(), f[..., 16:32].copy()
        r = R.ratio(f, c["ref"], c["bound"])
        _report("output fragments swapped", c["name"], r)
        assert r.max() > 1


def test_table_covers_the_converter():
    """The table's input holds every finite bf16 of both signs up to x_amax once, and its expected values span ties,
    subnormals, the flush and the top code."""
    for a in OP.TABLE_AMAX:
        t = OP.table(a)
        x = t["xv"].reshape(-1)
        n = int(torch.tensor([a]).to(BF16).view(torch.int16).item()) + 1
        assert len(np.unique(t["x"].view(torch.int16).numpy().reshape(-1)[:2 * n])) == 2 * n
        assert np.abs(x).max() == a and t["x"].shape[1] <= 1024
        q = np.abs(t["want"]).reshape(-1) / 0.875 / 2.0 ** t["e"]
        assert set(np.unique(q)) == set(R.GRID[R.GRID >= 0][:len(np.unique(q))])
        assert q.max() == (448 if a != 450 * 32 else 224) and (q == 0).sum() > 1000
        assert np.array_equal(R.rnd(t["want"], BF16), t["want"])           # exactly representable in bf16


# ---- the e4m3 stage's restatement (fp8_ref.chain8)
import functools  # noqa: E402


@functools.lru_cache(maxsize=None)
def stage8_q():
    from facerecognition_amd import weights as Wt
    return Wt.quantize_fp8(Wt.fold_state_dict(R.SR.ARCH, R.stage8_state_dict(0)), convs=Wt.fp8_plan(R.SR.ARCH))


@functools.lru_cache(maxsize=None)
def stage8_input():
    """A random bf16 stage input [3, 14, 14, 256] of the size of a real layer3.15 (values of a few units), half of it
    spread over 14 binades below, so that the exponent decides what is flushed."""
    rng = np.random.default_rng(8)
    v = rng.standard_normal((3, 14, 14, 256)) * 2.0
    return R.rnd(v * 2.0 ** -(rng.integers(0, 15, v.shape) * rng.integers(0, 2, v.shape)), BF16)


@functools.lru_cache(maxsize=None)
def stage8_clean():
    return R.chain8(stage8_input(), stage8_q())


def test_stage8_selection_weights_quantise_exactly():
    q = stage8_q()
    n = 0
    for i in range(R.STAGE8[0], R.STAGE8[1] + 1):
        for member, scale in (("conv1", 2.0 ** -9), ("conv2", 2.0 ** -11)):
            w, s = q[f"layer3.{i}.{member}.w"], q[f"layer3.{i}.{member}.wscale"]
            assert set(np.unique(w)) == {0.0, 448.0} and (np.count_nonzero(w.reshape(256, -1), axis=1) == 1).all()
            assert (s == np.float32(scale)).all()
            n += 1
        b9 = np.asarray(q[f"layer3.{i}.conv1.b9"], np.float64)
        assert np.array_equal(b9 * 128, np.round(b9 * 128)) and not np.any(q[f"layer3.{i}.conv2.b"])
    assert n == 28 and "layer3.15.conv1.wscale" not in q


def test_stage8_reference_stays_within_the_cap():
    """The ambiguity rule excludes at most 1e-3 of every tensor on a random stage input, and the chain stays alive."""
    worst = 0.0
    for name, (v, ex) in stage8_clean().items():
        worst = max(worst, ex.mean())
        assert ex.mean() <= R.CAP, f"{name}: {ex.mean():.2e} of the tensor excluded"
        assert np.isfinite(v).all() and (v != 0).mean() >= 0.5 and np.array_equal(v, R.rnd(v, BF16))
    print(f"STAGE8 reference: largest excluded share of a tensor {worst:.2e}")


def _stage8_fault_seen(what, faulty, at=None):
    """The faulty chain differs from the clean one outside both excluded sets, in the block of the fault already."""
    clean = stage8_clean()
    first = None
    for name in clean:
        keep = ~(clean[name][1] | faulty[name][1])
        n = int(((clean[name][0] != faulty[name][0]) & keep).sum())
        if n and first is None:
            first = (name, n)
    print(f"FAULT stage8 {what}: first seen in {first[0] if first else None}, {first[1] if first else 0} values; "
          f"layer3.29: {int(((clean['layer3.29'][0] != faulty['layer3.29'][0]) & ~(clean['layer3.29'][1] | faulty['layer3.29'][1])).sum())}")
    assert first is not None and (at is None or first[0] == at), (what, first)
    assert ((clean["layer3.29"][0] != faulty["layer3.29"][0]) & ~(clean["layer3.29"][1] | faulty["layer3.29"][1])).any()


def test_stage8_fault_dropped_k_step():
    q = dict(stage8_q())
    w = q["layer3.20.conv2.w"].copy()
    assert w[:, 1, 2, 128:].any()
    w[:, 1, 2, 128:] = 0  # one tap x 128 channels
    q["layer3.20.conv2.w"] = w
    _stage8_fault_seen("dropped K-step", R.chain8(stage8_input(), q), "layer3.20")


def test_stage8_fault_corner_class():
    q = dict(stage8_q())
    b9 = q["layer3.18.conv1.b9"].copy()
    assert not np.array_equal(b9[0], b9[1])
    b9[0] = b9[1]
    q["layer3.18.conv1.b9"] = b9
    faulty = R.chain8(stage8_input(), q)
    _stage8_fault_seen("corner border class", faulty, "layer3.18")


def test_stage8_fault_stale_halo_row():
    faulty = R.chain8(stage8_input(), stage8_q(), fault=("halo", "layer3.22.conv1", 1))
    _stage8_fault_seen("stale halo row, image 1", faulty, "layer3.22")
    clean = stage8_clean()
    for i in (0, 2):
        assert np.array_equal(faulty["layer3.22"][0][i], clean["layer3.22"][0][i])


def test_stage8_fault_exponent_of_another_image():
    x = stage8_input().copy()
    x[0] *= 4  # image 0 two binades above image 2 (exact in bf16)
    clean = R.chain8(x, stage8_q())
    faulty = R.chain8(x, stage8_q(), fault=("exp", "layer3.16.conv1", 2, 0))
    keep = ~(clean["layer3.16"][1] | faulty["layer3.16"][1])
    n = int(((clean["layer3.16"][0] != faulty["layer3.16"][0]) & keep).sum())
    print(f"FAULT stage8 exponent of image 2 from image 0: {n} values of layer3.16 differ")
    assert n > 0 and np.array_equal(clean["layer3.16"][0][:2], faulty["layer3.16"][0][:2])
