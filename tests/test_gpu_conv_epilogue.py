"""The conv epilogue (csrc/conv_epilogue.h), feature by feature, in every kernel that takes it.

The epilogue turns an f32 accumulator into stored activations: bias or the border-class bias9, residual, ReLU /
PReLU, the bf16 / f16 store (or bf16 from an f16 conv), the second output y2 = v * aff_s + aff_b and max |y|.  Every
kernel that claims implicit-GEMM tile 0's bits (the other tiles, conv_wring, conv_direct, conv_small at one wave per
tile) is run through fr_op_conv2d / fr_op_conv2d_ex (helpers.conv_op: the plain entry point forwards to _ex with
no ext, and any ext field takes _ex itself) with its tile forced, over the cross of the features it accepts, and every
tensor it writes must equal tile 0's on the same inputs bit for bit (compared as int16, so the sign of a zero counts).
y_amax (none, 1 slot, 64 slots) is cycled over the configurations of the cross, not crossed with them.
The split-K reducers sum in another order: the in-launch reduction must equal the two-launch one bit for bit, and the
two-launch one is held to the float reference at test_conv_split_k's tolerance.  conv_band keeps its own K order
(K_OWN): the same cross against the float reference at test_conv_band's tolerance.

Shapes are the smallest at which both predications are live (pixels no multiple of 16, Cout < Npad); the inputs have
a zeroed weight row with a zero and with a negative bias, so some accumulators are exactly 0, some outputs negative,
and PReLU slopes lie on both sides of 1, at 0 and below 0 (0 * slope = -0)."""
import functools
import itertools
import math

import pytest
import torch

from facerecognition_amd import _native as N
from tests.helpers import TORCH_DT, conv_op, conv_ref
from tests.test_gpu_ops import _border_class, _close

pytestmark = pytest.mark.gpu

IGEMM_TILES = [0, 1, 2, 3, 4, 5, 6, 8, 9, 17, 18, 19]
PADC, OFF = 16, 8  # a sliced buffer has Cout + PADC channels, the slice starts at OFF

# shape: B, H, W, Cin, Cout, k, pad
IGEMM_SHAPE = (1, 9, 9, 64, 72, 3, 1)     # K = Kpad = 576 (9 K-tiles), M = 81, Npad = 128
WRING_SHAPE = (1, 9, 9, 128, 256, 3, 1)
SMALL_SHAPE = (1, 9, 9, 64, 64, 3, 1)
DIRECT3_SHAPE = (1, 9, 9, 32, 32, 3, 1)   # conv_direct_kernel (patch in LDS)
DIRECT1_SHAPE = (1, 9, 9, 32, 32, 1, 0)   # conv_direct1_kernel (1x1 / s1: the one with a residual)
BAND4_SHAPE = (1, 14, 14, 64, 128, 3, 1)  # band variant 1: the 4-channel epilogue from registers
BAND8_SHAPE = (1, 14, 14, 64, 256, 3, 1)  # band variant 3: the LDS-staged 8-channel epilogue

# kind -> (shape, forced tile, split_k, what it takes beyond bias / activation / y slice)
KINDS = {f"tile{t}": (IGEMM_SHAPE, t, 1, {"bias9", "res", "y2", "ybf16", "amax"}) for t in IGEMM_TILES}
KINDS.update({
    "wring": (WRING_SHAPE, N.FR_TILE_WRING, 1, {"bias9", "res", "ybf16"}),
    "wring_tile0": (WRING_SHAPE, 0, 1, {"bias9", "res", "ybf16"}),
    "small_64": (SMALL_SHAPE, N.FR_TILE_SMALL, 1, {"bias9", "res", "ybf16"}),
    "small_32": (SMALL_SHAPE, N.FR_TILE_SMALL, 1 | 2 << 8, {"bias9", "res", "ybf16"}),
    "small_16": (SMALL_SHAPE, N.FR_TILE_SMALL, 1 | 1 << 8, {"bias9", "res", "ybf16"}),
    "small_tile0": (SMALL_SHAPE, 0, 1, {"bias9", "res", "ybf16"}),
    "direct3": (DIRECT3_SHAPE, N.FR_TILE_DIRECT, 1, {"ybf16"}),
    "direct3_tile0": (DIRECT3_SHAPE, 0, 1, {"ybf16"}),
    "direct1": (DIRECT1_SHAPE, N.FR_TILE_DIRECT, 1, {"res", "ybf16"}),
    "direct1_tile0": (DIRECT1_SHAPE, 0, 1, {"res", "ybf16"}),
    "band4": (BAND4_SHAPE, N.FR_TILE_BAND, 1, {"bias9", "res", "y2"}),
    "band8": (BAND8_SHAPE, N.FR_TILE_BAND, 1, {"bias9", "res", "y2"}),
})
for _t, _s in itertools.product((0, 17), (3, 4)):  # split 3: 3 + 3 + 3 K-tiles; split 4: 3 + 3 + 3 + 0 (ragged)
    KINDS[f"splitk_t{_t}_s{_s}"] = (IGEMM_SHAPE, _t, _s, {"bias9", "res", "y2", "amax", "two_launch"})
    KINDS[f"inlaunch_t{_t}_s{_s}"] = (IGEMM_SHAPE, _t, _s, {"bias9", "res", "y2", "amax", "inlaunch"})


def configs(takes, dtype):
    """The cross of the features a kind accepts; y_amax cycles through none / 1 slot / 64 slots."""
    out = []
    for bias, act, res, ysl, y2 in itertools.product(("none", "bias", "bias9"), (0, 1, 2), (False, True), (False, True),
                                                     (False, True)):
        if (bias == "bias9" and "bias9" not in takes) or (res and "res" not in takes) or (y2 and "y2" not in takes):
            continue
        out.append(dict(bias=bias, act=act, res=res, ysl=ysl, y2=y2, ybf16=False,
                        amax=(0, 1, 64)[len(out) % 3] if "amax" in takes else 0))
    if "ybf16" in takes and dtype == "f16":  # the bf16 store of an f16 conv takes neither residual nor y2
        for bias, act, ysl in itertools.product(("none", "bias", "bias9"), (0, 1, 2), (False, True)):
            if bias == "bias9" and "bias9" not in takes:
                continue
            out.append(dict(bias=bias, act=act, res=False, ysl=ysl, y2=False, ybf16=True, amax=0))
    return out


def cfg_name(c):
    return (f"{c['bias']}_act{c['act']}" + ("_res" if c["res"] else "") + ("_ysl" if c["ysl"] else "") +
            ("_y2" if c["y2"] else "") + ("_ybf16" if c["ybf16"] else "") + (f"_amax{c['amax']}" if c["amax"] else ""))


@functools.lru_cache(maxsize=None)
def inputs(shape, dtype):
    B, H, W, Cin, Cout, k, pad = shape
    g = torch.Generator().manual_seed(sum(shape) + (dtype == "f16"))
    dt = TORCH_DT[dtype]
    I = dict(x=torch.randn(B, H, W, Cin, generator=g).to(dt).cuda(),
             w=torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k),
             bias=torch.randn(Cout, generator=g) * 0.1, b9=torch.randn(9, Cout, generator=g) * 0.1,
             slope=torch.rand(Cout, generator=g) * 1.5, aff_s=torch.rand(Cout, generator=g) + 0.5,
             aff_b=torch.randn(Cout, generator=g) * 0.1,
             res=torch.randn(B, H, W, Cout + PADC, generator=g).to(dt),
             fill=torch.randn(B, H, W, Cout + PADC, generator=g))
    I["w"][3] = 0  # accumulators of channels 3 and 5 are exactly 0 ...
    I["w"][5] = 0
    I["bias"][3], I["bias"][5] = 0.0, -0.25  # ... channel 3 stays 0 (without residual), channel 5 goes negative
    I["b9"][:, 3], I["b9"][:, 5] = 0.0, -0.25
    I["slope"][0], I["slope"][1], I["slope"][3], I["slope"][5] = 0.0, 1.5, -0.5, 0.25
    I["res"][:, ::2, :, OFF + 3] = 0  # and stays 0 at every other row with one
    I["res"] = I["res"].cuda()
    return I


def run(shape, dtype, tile, split, cfg, inlaunch=False):
    """One launch; every tensor it wrote, on the CPU: y (the whole buffer), y2, max over the y_amax slots."""
    B, H, W, Cin, Cout, k, pad = shape
    I = inputs(shape, dtype)
    ydt = torch.bfloat16 if cfg["ybf16"] else TORCH_DT[dtype]
    kw = dict(pad=(pad, pad), dtype=dtype, tile=tile, split_k=split, act=cfg["act"], y_bf16=cfg["ybf16"], inlaunch=inlaunch)
    if cfg["bias"] == "bias":
        kw["bias"] = I["bias"]
    elif cfg["bias"] == "bias9":
        kw["bias9"] = I["b9"]
    if cfg["act"] == 2:
        kw["slope"] = I["slope"]
    if cfg["res"]:
        kw.update(res=I["res"], res_off=OFF)
    if cfg["ysl"]:
        kw.update(y=I["fill"].to(ydt).cuda(), y_off=OFF)
    y2 = ya = None
    if cfg["y2"]:
        y2 = torch.zeros(B, H, W, Cout, dtype=TORCH_DT[dtype], device="cuda")
        kw.update(y2=y2, aff_s=I["aff_s"], aff_b=I["aff_b"])
    if cfg["amax"]:
        ya = torch.zeros(cfg["amax"], device="cuda")
        kw.update(y_amax=ya, amax_slots=cfg["amax"])
    out = {"y": conv_op(I["x"], I["w"], **kw).cpu()}
    if y2 is not None:
        out["y2"] = y2.cpu()
    if ya is not None:
        out["amax"] = ya.max().cpu().reshape(1)
    return out


@functools.lru_cache(maxsize=None)
def outputs(kind, dtype):
    """Every output of every config of a kind: {config name: {tensor name: tensor}}.  Computed once and shared."""
    shape, tile, split, takes = KINDS[kind]
    return {cfg_name(c): run(shape, dtype, tile, split, c, inlaunch="inlaunch" in takes) for c in configs(takes, dtype)}


def pick(kind, dtype, **fields):
    """The outputs of the kind's first config with these fields."""
    c = next(c for c in configs(KINDS[kind][3], dtype) if all(c[k] == v for k, v in fields.items()))
    return outputs(kind, dtype)[cfg_name(c)]


def bits(t):
    return t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t.view(torch.int32)


def assert_same_bits(got, want, what):
    assert got.keys() == want.keys(), what
    for name in want:
        assert got[name].keys() == want[name].keys(), (what, name)
        for t in want[name]:
            assert got[name][t].dtype == want[name][t].dtype and torch.equal(bits(got[name][t]), bits(want[name][t])), \
                f"{what}: {t} of {name} differs"


def float_ref(shape, dtype, cfg):
    """The epilogue in f32 on conv_ref's sums: (y, y2 from the kernel's own stored y is checked by the caller)."""
    B, H, W, Cin, Cout, k, pad = shape
    I = inputs(shape, dtype)
    v = conv_ref(I["x"], I["w"], pad=(pad, pad), dtype=dtype)
    if cfg["bias"] == "bias":
        v = v + I["bias"]
    elif cfg["bias"] == "bias9":
        v = v + I["b9"][_border_class(H, W)]
    if cfg["res"]:
        v = v + I["res"].float().cpu()[..., OFF:OFF + Cout]
    if cfg["act"] == 1:
        v = torch.relu(v)
    elif cfg["act"] == 2:
        v = torch.where(v > 0, v, v * I["slope"])
    return v


def check_against_float(kind, dtype, tol):
    shape, tile, split, takes = KINDS[kind]
    Cout, I = shape[4], inputs(shape, dtype)
    got = outputs(kind, dtype)
    for c in configs(takes, dtype):
        o = got[cfg_name(c)]
        y = o["y"][..., OFF:OFF + Cout] if c["ysl"] else o["y"]
        _close(y, float_ref(shape, dtype, c), tol=1e-2 if c["ybf16"] else tol)  # a bf16 store rounds as bf16
        if c["y2"]:
            _close(o["y2"], y.float() * I["aff_s"] + I["aff_b"], tol=tol)


def check_outside_slice_unchanged(kind, dtype):
    shape, tile, split, takes = KINDS[kind]
    Cout, I = shape[4], inputs(shape, dtype)
    for c in configs(takes, dtype):
        if c["ysl"]:
            y = outputs(kind, dtype)[cfg_name(c)]["y"]
            before = I["fill"].to(y.dtype)
            assert torch.equal(bits(y[..., :OFF]), bits(before[..., :OFF])), (kind, cfg_name(c))
            assert torch.equal(bits(y[..., OFF + Cout:]), bits(before[..., OFF + Cout:])), (kind, cfg_name(c))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_reference_tile0_has_the_edge_values(gpu, dtype):
    """Tile 0, the bits everything else is held to: close to the float reference, columns outside a y slice
    untouched, and the inputs do reach the activation's edge: exact zeros of both signs and negative outputs."""
    check_against_float("tile0", dtype, tol=1e-2 if dtype == "bf16" else 2e-3)
    check_outside_slice_unchanged("tile0", dtype)
    plain = dict(bias="bias", res=False, ysl=False, y2=False, ybf16=False)
    y = pick("tile0", dtype, act=0, **plain)["y"]
    assert (bits(y[..., 3]) == 0).all() and (y[..., 5] == -0.25).all()
    y = pick("tile0", dtype, act=1, **plain)["y"]
    assert (bits(y[..., 3]) == 0).all() and (bits(y[..., 5]) == 0).all(), "ReLU of +0 and of -0.25 is +0"
    y = pick("tile0", dtype, act=2, **plain)["y"]
    assert (bits(y[..., 3]) == -32768).all(), "PReLU: +0 * (slope -0.5) is -0"
    assert (y[..., 5] == -0.0625).all(), "PReLU: -0.25 * (slope 0.25)"
    for name, o in outputs("tile0", dtype).items():
        if "amax" in o:  # max |v| before the output rounding: within the 16-bit formats' rounding of max |y|
            yy = o["y"][..., OFF:OFF + IGEMM_SHAPE[4]] if "_ysl" in name else o["y"]
            want = yy.float().abs().max().item()
            assert abs(o["amax"].item() - want) <= 2.0 ** -8 * want, (name, o["amax"].item(), want)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("tile", IGEMM_TILES[1:])
def test_every_igemm_tile_equals_tile0(gpu, tile, dtype):
    assert_same_bits(outputs(f"tile{tile}", dtype), outputs("tile0", dtype), f"tile {tile}")


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["wring", "small_64", "small_32", "small_16", "direct3", "direct1"])
def test_specialised_kernel_equals_tile0(gpu, kind, dtype):
    assert_same_bits(outputs(kind, dtype), outputs(kind.split("_")[0] + "_tile0", dtype), kind)
    check_outside_slice_unchanged(kind, dtype)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("split", [3, 4])
@pytest.mark.parametrize("tile", [0, 17])
def test_splitk_reducers(gpu, tile, split, dtype):
    """The two split-K sites: the in-launch reduction's bits are the two-launch reduction's, and those are the float
    reference's values at test_conv_split_k's tolerance."""
    two, one = f"splitk_t{tile}_s{split}", f"inlaunch_t{tile}_s{split}"
    assert_same_bits(outputs(one, dtype), outputs(two, dtype), one)
    check_against_float(two, dtype, tol=1e-2)
    check_outside_slice_unchanged(two, dtype)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["band4", "band8"])
def test_band_epilogues(gpu, kind, dtype):
    """conv_band sums K in its own order: both of its epilogues against the float reference, at test_conv_band's
    tolerance."""
    check_against_float(kind, dtype, tol=1e-2 if dtype == "bf16" else 2e-3)
    check_outside_slice_unchanged(kind, dtype)
