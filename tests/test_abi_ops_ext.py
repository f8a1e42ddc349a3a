"""The op-level entry points behind tests/test_gpu_ops_ext.py, on a machine without a GPU: they are exported
and bound, every host-side refusal returns FR_ERR_ARG with a message naming its entry point before anything is
launched (the device pointers below are never dereferenced), and the test helpers' packed projection rows and
reference agree with an independent float64 im2col product."""
import ctypes

import pytest
import torch

from facerecognition_amd import _native as N
from tests.helpers import conv_ref, pack_weight_cat

NEW = ["fr_op_conv2d_ex", "fr_op_head_gemv", "fr_op_proj_l2", "fr_op_l2norm_rows", "fr_op_amax", "fr_op_maxpool_cvt"]
P = 0x10000  # a non-null "device pointer": refused calls never touch it


def test_new_entry_points_exported_and_bound():
    L = N.lib()
    names = N.header_functions()
    for n in NEW:
        assert n in names and hasattr(L, n) and n in N._SIGS, n
    assert ctypes.sizeof(N.FrConvExt) == 56  # x2 8 | 6 ints 24 | y_bf16 4 + pad 4 | splitk_cnt 8 | amax_slots 4 + pad 4
    assert L.fr_abi_version() == 1


def _desc(**kw):
    """A valid 3x3 / stride 2 conv 14x14x64 -> 7x7x128 whose rows hold a 64-channel projection (Kpad = 576 + 64)."""
    d = N.FrConvDesc()
    d.x, d.B, d.H, d.W, d.Cx, d.x_off, d.Cin = P, 2, 14, 14, 64, 0, 64
    d.w, d.Cout, d.Kh, d.Kw, d.stride_h, d.stride_w, d.pad_h, d.pad_w, d.Npad, d.Kpad = P, 128, 3, 3, 2, 2, 1, 1, 128, 640
    d.y, d.Cy, d.Ho, d.Wo = P, 128, 7, 7
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _ext(proj=True, **kw):
    e = N.FrConvExt()
    if proj:
        e.x2, e.H2, e.W2, e.Cx2, e.x2_off, e.C2, e.st2 = P, 14, 14, 64, 0, 64, 2
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def _refused(d, e, word):
    L = N.lib()
    L.fr_op_avgpool(None, 1, 1, 1, 8, None, 0, None)  # another entry point's message first: a stale one cannot pass
    rc = L.fr_op_conv2d_ex(ctypes.byref(d), ctypes.byref(e), None)
    msg = L.fr_last_error().decode()
    assert rc == -1, (rc, msg)
    assert "fr_op_conv2d" in msg and word in msg, msg
    return msg


@pytest.mark.parametrize("dkw,ekw", [
    ({}, {"H2": 12}),                      # (Ho - 1) * st2 = 12 is past the last row of x2
    ({}, {"W2": 12}),
    ({"Cin": 32, "Cx": 32}, {}),           # Cin % 64
    ({}, {"C2": 32}),                      # C2 % 64
    ({"Kpad": 576}, {}),                   # K1 + C2 > Kpad
    ({}, {"x2_off": 8}),                   # x2_off + C2 > Cx2
    ({}, {"x2_off": 4, "Cx2": 128}),       # unaligned slice
    ({}, {"st2": 0}),
])
def test_projection_shape_rule_refused(dkw, ekw):
    assert "fr_op_conv2d_ex" in _refused(_desc(**dkw), _ext(**ekw), "x2")


@pytest.mark.parametrize("tile", [N.FR_TILE_BAND, N.FR_TILE_ROWS, N.FR_TILE_IMG28, N.FR_TILE_IMG56, N.FR_TILE_DIRECT])
def test_projection_refused_on_kernels_without_it(tile):
    assert "fr_op_conv2d_ex" in _refused(_desc(tile=tile + 1), _ext(), "x2")


def test_projection_refused_with_fp8():
    d = _desc(dtype=N.FR_DTYPE_FP8, wscale=P, x_amax=P, Kpad=640)
    assert "fr_op_conv2d_ex" in _refused(d, _ext(), "fp8")


@pytest.mark.parametrize("tile", [1, 4, 5, 6, 8, 9, N.FR_TILE_BAND, N.FR_TILE_WRING, N.FR_TILE_SMALL, N.FR_TILE_64x64, 40])
def test_fp8_refuses_tiles_it_does_not_have(tile):
    """conv_fp8.hip has the 128x128, 128x64 and 64x128 tiles; any other id used to run the 128x128 kernel."""
    d = _desc(dtype=N.FR_DTYPE_FP8, wscale=P, x_amax=P, Kpad=640, tile=tile + 1)
    L = N.lib()
    L.fr_op_avgpool(None, 1, 1, 1, 8, None, 0, None)
    for rc in (L.fr_op_conv2d(ctypes.byref(d), None), L.fr_op_conv2d_ex(ctypes.byref(d), ctypes.byref(_ext(False)), None)):
        msg = L.fr_last_error().decode()
        assert rc == N.FR_ERR_ARG and "fr_op_conv2d" in msg and "fp8" in msg and "FR_TILE_64x128" in msg, (rc, msg)


def test_projection_forced_kernels_keep_their_own_shape_checks():
    _refused(_desc(tile=N.FR_TILE_WRING + 1, Kpad=704), _ext(), "wring")  # K1 + C2 != Kpad
    d = _desc(tile=N.FR_TILE_SMALL + 1, Kh=7, Kw=7, pad_h=3, pad_w=3, Kpad=49 * 64 + 64)  # more than 32 taps
    _refused(d, _ext(), "small")


def test_y_bf16_refusals():
    assert "fr_op_conv2d_ex" in _refused(_desc(dtype=N.FR_DTYPE_BF16), _ext(False, y_bf16=1), "y_bf16")
    f16 = N.FR_DTYPE_F16
    _refused(_desc(dtype=f16, res=P, Cres=128), _ext(False, y_bf16=1), "y_bf16")
    _refused(_desc(dtype=f16, y2=P, Cy2=128, aff_s=P, aff_b=P), _ext(False, y_bf16=1), "y_bf16")
    _refused(_desc(dtype=f16, tile=N.FR_TILE_BAND + 1), _ext(False, y_bf16=1), "y_bf16")


@pytest.mark.parametrize("tile", [N.FR_TILE_WRING, N.FR_TILE_SMALL, N.FR_TILE_DIRECT, N.FR_TILE_BAND, N.FR_TILE_ROWS])
def test_inlaunch_counters_refused_off_the_igemm_tiles(tile):
    d = _desc(tile=tile + 1, split_k=4, partial=P)
    assert "fr_op_conv2d_ex" in _refused(d, _ext(False, splitk_cnt=P), "splitk_cnt")


def test_negative_amax_slots_refused():
    _refused(_desc(), _ext(False, amax_slots=-1), "amax_slots")


def test_null_descriptor_still_refused_through_ex():
    L = N.lib()
    assert L.fr_op_conv2d_ex(None, None, None) == -1 and b"fr_op_conv2d" in L.fr_last_error()
    d = N.FrConvDesc()
    assert L.fr_op_conv2d_ex(ctypes.byref(d), ctypes.byref(N.FrConvExt()), None) == -1


def _rc_msg(rc):
    return rc, N.lib().fr_last_error().decode()


def test_head_gemv_refusals():
    L = N.lib()
    ok = dict(B=1, K=64, N=512, Npad=512, Kpad=64, S=8, dtype=0)
    for bad in ({"B": 9}, {"B": 0}, {"K": 12, "Kpad": 16}, {"Kpad": 56}, {"Npad": 520, "N": 8}, {"N": 510},
                {"N": 1028, "Npad": 1040}, {"S": 0}, {"dtype": 2}, {"Kpad": 68}):
        a = dict(ok, **bad)
        rc, msg = _rc_msg(L.fr_op_head_gemv(P, a["B"], a["K"], P, a["N"], a["Npad"], a["Kpad"], None, 0, P, a["S"], P,
                                            a["dtype"], None))
        assert rc == -1 and "fr_op_head_gemv" in msg, (bad, rc, msg)
    rc, msg = _rc_msg(L.fr_op_head_gemv(P, 1, 64, P, 512, 512, 64, None, 0, P, 8, None, 0, None))  # no partial
    assert rc == -1 and "fr_op_head_gemv" in msg


def test_misc_op_refusals():
    L = N.lib()
    rc, msg = _rc_msg(L.fr_op_proj_l2(P, 2, 1032, P, None, 512, 1, P, None))
    assert rc == -1 and "fr_op_proj_l2" in msg
    rc, msg = _rc_msg(L.fr_op_proj_l2(None, 2, 512, P, None, 512, 1, P, None))
    assert rc == -1 and "fr_op_proj_l2" in msg
    rc, msg = _rc_msg(L.fr_op_l2norm_rows(P, 2, 0, None))
    assert rc == -1 and "fr_op_l2norm_rows" in msg
    for n, slots, dt in ((12, 1, 0), (0, 1, 0), (16, 0, 0), (16, 1, 2)):
        rc, msg = _rc_msg(L.fr_op_amax(P, n, dt, P, slots, None))
        assert rc == -1 and "fr_op_amax" in msg, (n, slots, dt)
    for k in (2, 5):
        rc, msg = _rc_msg(L.fr_op_maxpool_cvt(P, 1, 8, 8, 8, 0, 8, k, 2, 0, P, 8, 0, 3, 3, None))
        assert rc == -1 and "fr_op_maxpool_cvt" in msg


# ------------------------------------------------------------------ the helpers' packer and reference
PROJ_SHAPES = [
    # B, H, W, Cin, Cout, k, stride, H2, Cx2, x2_off, C2, st2   (tests/test_gpu_ops_ext.py's, the last one at Cout 64)
    (2, 14, 14, 64, 128, 3, 2, 14, 64, 0, 64, 2),
    (3, 7, 7, 64, 256, 1, 1, 7, 128, 0, 128, 1),
    (2, 9, 9, 128, 256, 1, 1, 17, 128, 0, 128, 2),
    (1, 8, 8, 128, 64, 3, 1, 8, 256, 64, 192, 1),
]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", PROJ_SHAPES)
def test_projection_packer_times_im2col_equals_reference(case, dtype):
    """out[m, n] = sum_k rows[n, k] * A[m, k] with A[m] = [the conv's (r, s, c) patch | x2 at (oh * st2, ow * st2),
    channels x2_off ..] written out by index in float64: what the kernels compute from pack_weight_cat's rows.  It
    must equal conv_ref (two F.conv2d calls), so a packer and a reference wrong in the same way cannot pass."""
    B, H, W, Cin, Cout, k, st, H2, Cx2, x2_off, C2, st2 = case
    g = torch.Generator().manual_seed(sum(case))
    dt = torch.bfloat16 if dtype == "bf16" else torch.float16
    x = torch.randn(B, H, W, Cin, generator=g).to(dt)
    x2 = torch.randn(B, H2, H2, Cx2, generator=g).to(dt)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    w2 = torch.randn(Cout, C2, 1, 1, generator=g) / C2 ** 0.5
    bias = torch.randn(Cout, generator=g) * 0.1
    pad = k // 2
    rows, npad, kpad = pack_weight_cat(w, w2, "cpu", dtype)
    K1 = k * k * Cin
    assert npad % 128 == 0 and kpad % 64 == 0 and kpad >= K1 + C2
    assert torch.count_nonzero(rows[Cout:]) == 0 and torch.count_nonzero(rows[:, K1 + C2:]) == 0
    Ho, Wo = (H + 2 * pad - k) // st + 1, (W + 2 * pad - k) // st + 1
    xd, x2d = x.double(), x2.double()
    A = torch.zeros(B, Ho, Wo, kpad, dtype=torch.float64)
    for oh in range(Ho):
        for ow in range(Wo):
            for r in range(k):
                for s in range(k):
                    ih, iw = oh * st - pad + r, ow * st - pad + s
                    if 0 <= ih < H and 0 <= iw < W:
                        A[:, oh, ow, (r * k + s) * Cin:(r * k + s + 1) * Cin] = xd[:, ih, iw]
            A[:, oh, ow, K1:K1 + C2] = x2d[:, oh * st2, ow * st2, x2_off:x2_off + C2]
    got = A @ rows[:Cout].double().t() + bias.double()
    kw = dict(stride=(st, st), pad=(pad, pad), bias=bias, dtype=dtype, x2=x2, w2=w2, st2=st2, x2_off=x2_off)
    ref = conv_ref(x, w, f64=True, **kw)
    scale = ref.abs().max().item()
    assert (got - ref).abs().max().item() <= 1e-6 * scale
    # the f32 reference the GPU tests compare against is that float64 one up to f32 summation error
    assert (conv_ref(x, w, **kw).double() - ref).abs().max().item() <= 1e-5 * scale
    # and the epilogue order: bias, then residual, then the activation
    res = torch.randn(B, Ho, Wo, Cout, generator=g).to(dt)
    slope = torch.rand(Cout, generator=g) * 0.5
    full = conv_ref(x, w, f64=True, res=res, act=2, slope=slope, **kw)
    pre = got + res.double()
    assert (torch.where(pre > 0, pre, pre * slope.double()) - full).abs().max().item() <= 1e-6 * scale
