"""Op-level parity for the conv and head paths that only whole-model forwards used to reach (fr_op_conv2d_ex and
the fr_op_head_gemv / proj_l2 / l2norm_rows / amax / maxpool_cvt entry points): the K-concatenated 1x1 projection
in every kernel that implements it, the in-launch split-K reduction at forced tiles and splits, the f16 -> bf16
boundary stores, the small-batch head GEMV and the small misc.hip kernels.

Each kernel is forced and compared with (a) an f32 / f64 reference of the same op on 16-bit-exact operands at
test_gpu_ops.py's tolerances (|got - ref| <= tol * (|ref| + max|ref| / 8), tol 1e-2 bf16 / 2e-3 f16: summation
order and the output rounding only), and (b) bit for bit with implicit-GEMM tile 0 wherever a kernel documents the
same K order -- which is what catches a wrong row, a dropped K step or a stale counter that a tolerance hides.
tests/test_abi_ops_ext.py checks the helpers' packer and reference against each other without a GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

from facerecognition_amd import _native as N
from tests.helpers import TORCH_DT, conv_op, conv_ref, pack_weight, q16
from tests.test_gpu_ops import _close

pytestmark = pytest.mark.gpu

TOL = {"bf16": 1e-2, "f16": 2e-3}
IGEMM_TILES = [0, 1, 2, 3, 4, 5, 6, 8, 9, 17, 18, 19]

# ---------------------------------------------------------------------------------- K-concatenated projection
PROJ_CASES = [
    # B, H, W, Cin, Cout, k, stride, H2, Cx2, x2_off, C2, st2
    (2, 14, 14, 64, 128, 3, 2, 14, 64, 0, 64, 2),    # iresnet: 3x3/s2 + 1x1/s2; Ho = 7 reads x2 row / column 12 of 14
    (3, 7, 7, 64, 256, 1, 1, 7, 128, 0, 128, 1),     # r50 conv3 + downsample: M = 147, ragged in every tile
    (2, 9, 9, 128, 256, 1, 1, 17, 128, 0, 128, 2),   # H2 odd, (Ho - 1) * st2 = H2 - 1 exactly
    (1, 8, 8, 128, 256, 3, 1, 8, 256, 64, 192, 1),   # the projection reads channels [64, 256) of x2
    (2, 7, 7, 128, 256, 3, 1, 7, 128, 0, 128, 1),    # built for conv_wring's 128-channel stages (Kpad / 128 = 10)
]
PROJ_EPILOGUES = ["prelu", "relu_y2", "slice"]


def _proj_inputs(case, dtype, gpu):
    B, H, W, Cin, Cout, k, st, H2, Cx2, x2_off, C2, st2 = case
    g = torch.Generator().manual_seed(sum(case) + (dtype == "f16"))
    x = torch.randn(B, H, W, Cin, generator=g).to(TORCH_DT[dtype]).to(gpu)
    x2 = torch.randn(B, H2, H2, Cx2, generator=g).to(TORCH_DT[dtype]).to(gpu)
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    w2 = torch.randn(Cout, C2, 1, 1, generator=g) / math.sqrt(C2)
    t = dict(bias=torch.randn(Cout, generator=g) * 0.1, slope=torch.rand(Cout, generator=g) * 0.5,
             aff_s=torch.rand(Cout, generator=g) + 0.5, aff_b=torch.randn(Cout, generator=g) * 0.1,
             fill=torch.randn(B, (H + 2 * (k // 2) - k) // st + 1, (W + 2 * (k // 2) - k) // st + 1, Cout + 48, generator=g))
    kw = dict(stride=(st, st), pad=(k // 2, k // 2), dtype=dtype, x2=x2, w2=w2, st2=st2, x2_off=x2_off, bias=t["bias"])
    return x, w, kw, t


class _Epilogue:
    """One of the three epilogues: run(tile, ...) -> every tensor the launch wrote; ref -> what conv_ref says of them."""

    def __init__(self, name, case, dtype, gpu):
        self.name, self.dtype, self.gpu = name, dtype, gpu
        self.x, self.w, self.kw, self.t = _proj_inputs(case, dtype, gpu)
        self.Cout = case[4]
        self.ref = conv_ref(self.x, self.w, act={"prelu": 2, "relu_y2": 1, "slice": 0}[name], slope=self.t["slope"], **self.kw)

    def run(self, tile, **more):
        kw = dict(self.kw, tile=tile, **more)
        if self.name == "prelu":
            return (conv_op(self.x, self.w, act=2, slope=self.t["slope"], **kw),)
        if self.name == "relu_y2":
            y2 = torch.zeros(self.ref.shape, dtype=TORCH_DT[self.dtype], device=self.gpu)
            y = conv_op(self.x, self.w, act=1, y2=y2, aff_s=self.t["aff_s"], aff_b=self.t["aff_b"], **kw)
            return y, y2
        buf = self.t["fill"].to(TORCH_DT[self.dtype]).to(self.gpu)  # the output goes to channels [24, 24 + Cout)
        conv_op(self.x, self.w, y=buf, y_off=24, **kw)
        return (buf,)

    def check_close(self, out):
        tol = TOL[self.dtype]
        if self.name == "slice":
            before = self.t["fill"].to(TORCH_DT[self.dtype])
            got = out[0].cpu()
            _close(got[..., 24:24 + self.Cout], self.ref, tol=tol)
            assert torch.equal(got[..., :24], before[..., :24]) and torch.equal(got[..., 24 + self.Cout:], before[..., 24 + self.Cout:])
            return
        _close(out[0], self.ref, tol=tol)
        if self.name == "relu_y2":
            _close(out[1], out[0].float().cpu() * self.t["aff_s"] + self.t["aff_b"], tol=tol)


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("epi", PROJ_EPILOGUES)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", PROJ_CASES)
def test_projection_every_implementation(gpu, case, dtype, epi):
    """(a) every implicit-GEMM tile, conv_wring and conv_small (1 / 4 / 8 waves per tile) against the f32 reference,
    (b) bit for bit with tile 0 where the K order is tile 0's (all but conv_small's K splits)."""
    E = _Epilogue(epi, case, dtype, gpu)
    base = E.run(0)
    E.check_close(base)
    for tile in IGEMM_TILES[1:]:
        out = E.run(tile)
        E.check_close(out)
        assert _same(out, base), f"tile {tile} differs from tile 0"
    if epi == "relu_y2":  # neither kernel has a second output: refused, never run elsewhere
        with pytest.raises(RuntimeError, match="wring"):
            E.run(N.FR_TILE_WRING)
        with pytest.raises(RuntimeError, match="small"):
            E.run(N.FR_TILE_SMALL)
        return
    out = E.run(N.FR_TILE_WRING)
    E.check_close(out)
    assert _same(out, base), "conv_wring differs from tile 0"
    for ks in (1, 4, 8):
        out = E.run(N.FR_TILE_SMALL, split_k=ks)
        E.check_close(out)
        if ks == 1:
            assert _same(out, base), "conv_small (one wave per tile) differs from tile 0"


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", [c for c in PROJ_CASES if c[5] == 1])
def test_projection_1x1_equals_plain_conv_over_concatenated_input(gpu, case, dtype):
    """(c) a 1x1 conv with a projection is a plain 1x1 conv over [x | x2[:, ::st2, ::st2, slice]] with the same K
    steps in the same order: tile 0 over the host-concatenated input gives the bits every implementation must
    give, which checks the projection's addressing with no tolerance at all."""
    B, H, W, Cin, Cout, k, st, H2, Cx2, x2_off, C2, st2 = case
    assert st == 1
    x, w, kw, t = _proj_inputs(case, dtype, gpu)
    xcat = torch.cat([x, kw["x2"][:, ::st2, ::st2][:, :H, :W, x2_off:x2_off + C2]], dim=-1).contiguous()
    wcat = torch.cat([w, kw["w2"]], dim=1)
    want = conv_op(xcat, wcat, bias=t["bias"], act=2, slope=t["slope"], dtype=dtype, tile=0)
    impls = [(tile, 1) for tile in IGEMM_TILES] + [(N.FR_TILE_WRING, 1), (N.FR_TILE_SMALL, 1)]
    for tile, sp in impls:
        got = conv_op(x, w, act=2, slope=t["slope"], tile=tile, split_k=sp, **kw)
        assert torch.equal(got, want), f"tile {tile}: projection differs from the concatenated-input conv"


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_projection_split_k(gpu, dtype):
    """(d) two-launch split-K with the projection's K steps in the last chunk(s): a chunk boundary on K1 and off it
    (both occur over the cases, asserted), and the in-launch reduction equal to it bit for bit."""
    on_k1 = set()
    for case in PROJ_CASES:
        B, H, W, Cin, Cout, k, st, H2, Cx2, x2_off, C2, st2 = case
        E = _Epilogue("prelu", case, dtype, gpu)
        nkt, kt1 = (k * k * Cin + C2 + 63) // 64, k * k * Cin // 64
        for split in (2, 3):
            per = -(-nkt // split)
            on_k1.add(kt1 % per == 0)
            for tile in (0, 17):
                out = E.run(tile, split_k=split)
                E.check_close(out)
                assert _same(E.run(tile, split_k=split, inlaunch=True), out), (case, split, tile)
    assert on_k1 == {True, False}


def test_projection_refusals_leave_output_untouched(gpu):
    """(e) what fr_op_conv2d_ex cannot run is an error, and nothing was launched: y keeps its bytes."""
    case = PROJ_CASES[0]
    x, w, kw, t = _proj_inputs(case, "bf16", gpu)
    y = torch.randn(2, 7, 7, 128).to(torch.bfloat16).to(gpu)
    before = y.clone()
    bad = [
        dict(st2=3),                                                             # (Ho - 1) * st2 = 18 past H2 = 14
        dict(x2=kw["x2"][:, :12].contiguous()),                                  # H2 = 12: row 12 does not exist
        dict(x2=kw["x2"][:, :, :12].contiguous()),                               # W2 = 12
        dict(x2_off=8),                                                          # x2_off + C2 > Cx2
        dict(w2=kw["w2"][:, :32], x2=kw["x2"][..., :32].contiguous()),           # C2 % 64
        dict(tile=N.FR_TILE_BAND), dict(tile=N.FR_TILE_ROWS), dict(tile=N.FR_TILE_IMG28), dict(tile=N.FR_TILE_IMG56),
        dict(tile=N.FR_TILE_DIRECT),
        dict(tile=N.FR_TILE_WRING, split_k=2, inlaunch=True), dict(tile=N.FR_TILE_SMALL, split_k=4, inlaunch=True),
        dict(y_bf16=True),                                                       # bf16 input
    ]
    for b in bad:
        with pytest.raises(RuntimeError, match="fr_op_conv2d_ex"):
            conv_op(x, w, y=y, **dict(kw, **b))
        assert torch.equal(y, before), b
    x32 = x[..., :32].contiguous()  # Cin % 64
    with pytest.raises(RuntimeError, match="fr_op_conv2d_ex"):
        conv_op(x32, w[:, :32], y=y, **kw)
    xh, x2h = x.to(torch.float16), kw["x2"].to(torch.float16)
    res = torch.zeros(2, 7, 7, 128, dtype=torch.float16, device=gpu)
    with pytest.raises(RuntimeError, match="y_bf16"):  # the boundary store takes no residual
        conv_op(xh, w, y=y, res=res, y_bf16=True, **dict(kw, dtype="f16", x2=x2h))
    with pytest.raises(RuntimeError, match="y_bf16"):  # nor a second output
        conv_op(xh, w, y=y, y2=res, aff_s=t["aff_s"], aff_b=t["aff_b"], y_bf16=True, **dict(kw, dtype="f16", x2=x2h))
    assert torch.equal(y, before)
    torch.cuda.synchronize()


def test_zeroed_ext_is_plain_conv(gpu):
    """fr_op_conv2d is fr_op_conv2d_ex with no ext; an all-zero ext is the same call (every kernel family)."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 14, 14, 128, generator=g).to(torch.bfloat16).to(gpu)  # (one of BAND_CASES' shapes)
    w = torch.randn(256, 128, 3, 3, generator=g) / math.sqrt(128 * 9)
    bias = torch.randn(256, generator=g) * 0.1
    res = torch.randn(2, 14, 14, 256, generator=g).to(torch.bfloat16).to(gpu)
    for kw in (dict(tile=None), dict(tile=0, split_k=3), dict(tile=N.FR_TILE_WRING), dict(tile=N.FR_TILE_SMALL, split_k=4),
               dict(tile=N.FR_TILE_BAND)):
        kw = dict(kw, pad=(1, 1), bias=bias, res=res, act=1)
        assert torch.equal(conv_op(x, w, ex=True, **kw), conv_op(x, w, **kw)), kw


# ---------------------------------------------------------------------------------- in-launch split-K reduction
INLAUNCH_CASES = [
    # B, H, W, Cin, Cout, kh, kw, pad
    (2, 7, 7, 512, 512, 3, 3, (1, 1)),   # layer4: nkt = 72
    (3, 5, 5, 192, 192, 1, 3, (0, 1)),   # M = 75 ragged, nkt = 9: not divisible by 2, 5 or 7 (split 7: empty chunks)
]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("tile", [0, 2, 3, 17, 19])
@pytest.mark.parametrize("case", INLAUNCH_CASES)
def test_splitk_inlaunch_equals_two_launch(gpu, case, tile, dtype):
    """The last workgroup of each tile sums the partials in split order: the two-launch reduction's bits, at every
    forced tile and split (ragged K chunks, empty chunks), for bias + residual + ReLU and border-class bias + PReLU.
    The tile counters are zero again afterwards, and a second call on the same counters and workspace repeats the
    bits.  The workspace starts as NaN, so a slab that was summed without having been written shows."""
    B, H, W, Cin, Cout, kh, kw_, pad = case
    g = torch.Generator().manual_seed(sum(case[:7]) + tile)
    dt = TORCH_DT[dtype]
    x = torch.randn(B, H, W, Cin, generator=g).to(dt).to(gpu)
    w = torch.randn(Cout, Cin, kh, kw_, generator=g) / math.sqrt(Cin * kh * kw_)
    bias = torch.randn(Cout, generator=g) * 0.1
    b9 = torch.randn(9, Cout, generator=g) * 0.1
    slope = torch.rand(Cout, generator=g) * 0.5
    res = torch.randn(B, H, W, Cout, generator=g).to(dt).to(gpu)
    epis = [dict(bias=bias, res=res, act=1), dict(bias9=b9, act=2, slope=slope)]
    ref = conv_ref(x, w, pad=pad, bias=bias, res=res, act=1, dtype=dtype)
    npad = (Cout + 127) // 128 * 128
    for split in (2, 5, 7):
        cnt = torch.zeros(256, dtype=torch.int32, device=gpu)
        assert ((B * H * W + 31) // 32) * (npad // 64) <= cnt.numel()
        part = torch.full((split * B * H * W * npad,), float("nan"), device=gpu)
        for i, ep in enumerate(epis):
            kw = dict(pad=pad, dtype=dtype, tile=tile, split_k=split, **ep)
            two = conv_op(x, w, **kw)
            if i == 0:
                _close(two, ref, tol=TOL[dtype])
            one = conv_op(x, w, inlaunch=True, cnt=cnt, partial=part, **kw)
            assert torch.equal(one, two), f"split {split} epilogue {i}: in-launch differs from the two-launch reduction"
            assert torch.count_nonzero(cnt).item() == 0, "a tile counter was left non-zero"
            again = conv_op(x, w, inlaunch=True, cnt=cnt, partial=part, **kw)
            assert torch.equal(again, two) and torch.count_nonzero(cnt).item() == 0


@pytest.mark.parametrize("slots", [1, 64])
@pytest.mark.parametrize("case", INLAUNCH_CASES)
def test_splitk_inlaunch_amax(gpu, case, slots):
    """y_amax from the in-launch reduction's epilogue: the maximum over the slots is max |y| of what it stored, before
    the output rounding (hence test_gpu_fp8.py's 1e-2 relative bound, bf16's 2^-8 inside it)."""
    B, H, W, Cin, Cout, kh, kw_, pad = case
    g = torch.Generator().manual_seed(slots + Cin)
    x = torch.randn(B, H, W, Cin, generator=g).to(torch.bfloat16).to(gpu)
    w = torch.randn(Cout, Cin, kh, kw_, generator=g) / math.sqrt(Cin * kh * kw_)
    bias = torch.randn(Cout, generator=g) * 0.1
    slope = torch.rand(Cout, generator=g) * 0.5
    for tile, split in ((0, 2), (17, 5), (19, 7)):
        for inl in (True, False):
            ya = torch.zeros(slots, device=gpu)
            y = conv_op(x, w, pad=pad, bias=bias, act=2, slope=slope, tile=tile, split_k=split, inlaunch=inl, y_amax=ya,
                        amax_slots=slots)
            got, want = ya.max().item(), y.float().abs().max().item()
            assert want > 0 and abs(got - want) <= 1e-2 * got, (tile, split, inl, got, want)


# ---------------------------------------------------------------------------------- f16 in, bf16 out
YBF16_CASES = [
    # (B, H, W, Cin, Cout, kh, kw, stride, pad), kernels   -- one shape from each kernel's own case list
    ((2, 8, 8, 256, 896, 1, 1, 1, 0), [0, 17, N.FR_TILE_WRING, N.FR_TILE_SMALL, N.FR_TILE_DIRECT]),  # DIRECT_CASES: all five
    ((3, 7, 7, 512, 512, 3, 3, 1, 1), [0, 17, N.FR_TILE_WRING, N.FR_TILE_SMALL]),                    # WRING_CASES
    ((1, 28, 28, 128, 256, 3, 3, 2, 1), [0, 17, N.FR_TILE_WRING, N.FR_TILE_SMALL]),                  # SMALL_CASES
    ((2, 41, 41, 8, 32, 3, 3, 2, 0), [0, 17, N.FR_TILE_DIRECT]),                                     # DIRECT_CASES: Cin = 8
]


@pytest.mark.parametrize("case,tiles", YBF16_CASES)
def test_y_bf16_boundary_store(gpu, case, tiles):
    """An f16 conv storing bf16 (each kernel's own pack line): the f32 result rounded once to bf16, so within the bf16
    tolerance of the f32 reference (and of its bf16 rounding -- not equal to it: the f32 sums differ in order), and
    the same bits from every kernel, which all sum K in tile 0's order."""
    B, H, W, Cin, Cout, kh, kw_, st, pd = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(B, H, W, Cin, generator=g).to(torch.float16).to(gpu)
    w = torch.randn(Cout, Cin, kh, kw_, generator=g) / math.sqrt(Cin * kh * kw_)
    bias = torch.randn(Cout, generator=g) * 0.1
    slope = torch.rand(Cout, generator=g) * 0.5
    for ep in (dict(act=1), dict(act=2, slope=slope)):
        kw = dict(stride=(st, st), pad=(pd, pd), bias=bias, dtype="f16", **ep)
        ref = conv_ref(x, w, **kw)
        outs = [conv_op(x, w, tile=t, y_bf16=True, **kw) for t in tiles]
        assert outs[0].dtype == torch.bfloat16
        _close(outs[0], ref, tol=1e-2)
        _close(outs[0], ref.to(torch.bfloat16), tol=1e-2)
        for t, o in zip(tiles[1:], outs[1:]):
            assert torch.equal(o, outs[0]), f"kernel {t} differs from tile 0"
        # the same f32 value v stored as f16 instead: |bf16(v) - f16(v)| <= |v| (2^-9 + 2^-12) (the two half-ulps),
        # plus half an f16 subnormal step (2^-25) near zero
        y16 = conv_op(x, w, tile=0, **kw).float()
        step = torch.maximum(outs[0].float().abs(), y16.abs()) * 2.0 ** -8 + 2.0 ** -24
        assert bool(((outs[0].float() - y16).abs() <= step).all())


def _f16_bits(bits):
    return torch.tensor(bits, dtype=torch.int16).view(torch.float16)


@pytest.mark.parametrize("k,s,p,H", [(3, 2, 1, 56), (3, 2, 0, 17)])
def test_maxpool_cvt_exact_with_ties(gpu, k, s, p, H):
    """maxpool3_kernel<true, true>: the f16 maximum rounded to bf16 once, to nearest even.  Planted window maxima
    whose f16 mantissa ends ..1100 / ..0100 lie exactly between two bf16 values (bf16 keeps 7 of f16's 10 mantissa
    bits): the first rounds up, the second down."""
    g = torch.Generator().manual_seed(H)
    x = torch.randn(2, H, H, 64, generator=g).to(torch.float16)
    # exponent 2^6 .. 2^7 (above every random value): sign 0 | exp 0x15 / 0x16 | mantissa
    ties = _f16_bits([0x5400 | 0x00C, 0x5400 | 0x004, 0x5800 | 0x3FC, 0x5800 | 0x014, 0x5400 | 0x1EC])
    spots = [(0, 0, 0, 0), (0, 1, 2, 5), (1, H - 1, H - 1, 63), (1, H // 2, H - 2, 17), (0, H - 1, 0, 8)]
    for v, (b, i, j, c) in zip(ties, spots):
        x[b, i, j, c] = v
    ref = F.max_pool2d(x.float().permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1).to(torch.bfloat16)
    up, down = ties.float() < ties.to(torch.bfloat16).float(), ties.float() > ties.to(torch.bfloat16).float()
    assert up.any() and down.any() and bool((up | down).all())  # the reference rounds them both ways: to even
    assert all(bool((ref.float() == t).any()) for t in ties.to(torch.bfloat16).float())  # and they reach the output
    Ho = (H + 2 * p - k) // s + 1
    y = torch.zeros(2, Ho, Ho, 128, dtype=torch.bfloat16, device=gpu)
    xd = x.to(gpu)
    N.check(N.lib().fr_op_maxpool_cvt(xd.data_ptr(), 2, H, H, 64, 0, 64, k, s, p, y.data_ptr(), 128, 64, Ho, Ho,
                                      N.stream_ptr()), "fr_op_maxpool_cvt")
    torch.cuda.synchronize()
    assert torch.equal(y[..., 64:].cpu(), ref)
    assert torch.count_nonzero(y[..., :64]) == 0
    with pytest.raises(RuntimeError, match="fr_op_maxpool_cvt"):
        N.check(N.lib().fr_op_maxpool_cvt(xd.data_ptr(), 2, H, H, 64, 0, 64, 2, 2, 0, y.data_ptr(), 128, 64, Ho, Ho,
                                          N.stream_ptr()), "fr_op_maxpool_cvt")


# ---------------------------------------------------------------------------------- head GEMV
GEMV_CASES = [
    # B, K, N, S
    (1, 25088, 512, 8),   # the real head
    (3, 2056, 512, 8),    # kchunk = 264, the last chunk 208; 3 probes in the NB = 4 variant
    (5, 4104, 200, 3),    # NB = 8 with 3 probes masked; N < Npad = 256
    (8, 40, 512, 8),      # chunks 5 .. 7 are empty: exact zeros
    (2, 1032, 512, 1),
    (4, 520, 512, 8),
]


def _head_gemv(x, wp, N_, npad, kpad, bias, norm, S, dtype):
    B, K = x.shape
    out = torch.full((B, N_), float("nan"), device=x.device)
    part = torch.full((S * B * npad,), float("nan"), device=x.device)
    N.check(N.lib().fr_op_head_gemv(x.data_ptr(), B, K, wp.data_ptr(), N_, npad, kpad, N.ptr(bias), norm, out.data_ptr(),
                                    S, part.data_ptr(), N.FR_DTYPE[dtype], N.stream_ptr()), "fr_op_head_gemv")
    torch.cuda.synchronize()
    return out.cpu(), part.cpu().view(S, B, npad)


def _head_close(out, ref):
    assert torch.allclose(out.double(), ref, rtol=1e-4, atol=1e-4 * ref.abs().max().item()), \
        f"max err {(out.double() - ref).abs().max().item():.3g} of {ref.abs().max().item():.3g}"


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", GEMV_CASES)
def test_head_gemv(gpu, case, dtype):
    """head_gemv_kernel + head_finalize against float64 x @ q16(w).T + b (test_linear_head's tolerance), with and
    without bias and normalize; `partial` and `out` start as NaN, so a chunk or a row nobody wrote shows."""
    B, K, N_, S = case
    g = torch.Generator().manual_seed(B + K)
    x = torch.randn(B, K, generator=g).to(TORCH_DT[dtype]).to(gpu)
    w = torch.randn(N_, K, generator=g) / math.sqrt(K)
    b = torch.randn(N_, generator=g) * 0.1
    wp, npad, kpad = pack_weight(w.view(N_, K, 1, 1), gpu, dtype)
    assert npad == (256 if N_ == 200 else 512)
    prod = x.cpu().double() @ q16(w, dtype).double().t()
    bd = b.to(gpu)
    for bias in (bd, None):
        for norm in (0, 1):
            ref = prod + (b.double() if bias is not None else 0.0)
            out, part = _head_gemv(x, wp, N_, npad, kpad, bias, norm, S, dtype)
            _head_close(out, F.normalize(ref, dim=1) if norm else ref)
    assert not torch.isnan(part).any()  # every (chunk, probe, row < Npad) was written
    kchunk = (K + 8 * S - 1) // (8 * S) * 8
    for s in range(S):
        if s * kchunk >= K:  # an empty chunk contributes exact zeros
            assert torch.count_nonzero(part[s]) == 0
    assert torch.count_nonzero(part[:, :, N_:]) == 0  # the padded weight rows are zero


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_head_gemv_rows_do_not_depend_on_batch(gpu, dtype):
    """A probe's row from the B = 1 instantiation and from inside B = 2, 3, 4, 5, 8 (the NB = 2 / 4 / 8 ones, masked
    where B < NB); B = 9 is refused."""
    K, N_, S = 2056, 512, 8
    g = torch.Generator().manual_seed(77)
    x = torch.randn(8, K, generator=g).to(TORCH_DT[dtype]).to(gpu)
    w = torch.randn(N_, K, generator=g) / math.sqrt(K)
    wp, npad, kpad = pack_weight(w.view(N_, K, 1, 1), gpu, dtype)
    ref = x.cpu().double() @ q16(w, dtype).double().t()
    atol = 1e-4 * ref.abs().max().item()
    single = torch.cat([_head_gemv(x[i:i + 1].contiguous(), wp, N_, npad, kpad, None, 0, S, dtype)[0] for i in range(8)])
    _head_close(single, ref)
    for B in (2, 3, 4, 5, 8):
        out, _ = _head_gemv(x[:B].contiguous(), wp, N_, npad, kpad, None, 0, S, dtype)
        assert torch.allclose(out, single[:B], rtol=1e-4, atol=atol), B
        _head_close(out, ref[:B])
    x9 = torch.zeros(9, K, dtype=TORCH_DT[dtype], device=gpu)
    with pytest.raises(RuntimeError, match="fr_op_head_gemv"):
        _head_gemv(x9, wp, N_, npad, kpad, None, 0, S, dtype)


# ---------------------------------------------------------------------------------- proj_l2, l2norm_rows, amax
@pytest.mark.parametrize("B,K,N_", [(4, 512, 512), (2, 1024, 520), (3, 8, 64), (1, 128, 1000)])
def test_proj_l2(gpu, B, K, N_):
    """FaceNet projection + F.normalize: N = 64 leaves three quarters of the block without a column, 520 and 1000
    are no multiple of the 256 threads; bias present and null, normalize 0 and 1; an all-zero row normalizes to
    zeros (eps clamp), not NaN; K = 1032 does not fit the kernel's LDS row and is refused."""
    g = torch.Generator().manual_seed(K + N_)
    x = torch.randn(B, K, generator=g)
    W = torch.randn(N_, K, generator=g) / math.sqrt(K)
    b = torch.randn(N_, generator=g) * 0.1
    xd, Wd, bd = x.to(gpu), W.to(gpu), b.to(gpu)
    for bias in (bd, None):
        for norm in (0, 1):
            out = torch.full((B, N_), float("nan"), device=gpu)
            N.check(N.lib().fr_op_proj_l2(xd.data_ptr(), B, K, Wd.data_ptr(), N.ptr(bias), N_, norm, out.data_ptr(),
                                          N.stream_ptr()), "fr_op_proj_l2")
            torch.cuda.synchronize()
            ref = x.double() @ W.double().t() + (b.double() if bias is not None else 0.0)
            _head_close(out.cpu(), F.normalize(ref, dim=1) if norm else ref)
    xz = xd.clone()
    xz[B - 1] = 0
    out = torch.full((B, N_), float("nan"), device=gpu)
    N.check(N.lib().fr_op_proj_l2(xz.data_ptr(), B, K, Wd.data_ptr(), None, N_, 1, out.data_ptr(), N.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.count_nonzero(out[B - 1]) == 0 and not torch.isnan(out).any()
    before = out.clone()
    with pytest.raises(RuntimeError, match="fr_op_proj_l2"):
        N.check(N.lib().fr_op_proj_l2(xd.data_ptr(), 1, 1032, Wd.data_ptr(), None, 1, 1, out.data_ptr(), N.stream_ptr()),
                "fr_op_proj_l2")
    assert torch.equal(out, before)


@pytest.mark.parametrize("D", [512, 8, 1000])
def test_l2norm_rows(gpu, D):
    g = torch.Generator().manual_seed(D)
    x = torch.randn(5, D, generator=g) * 3.0
    x[3] = 0  # eps clamp: zeros stay zeros
    xd = x.to(gpu)
    N.check(N.lib().fr_op_l2norm_rows(xd.data_ptr(), 5, D, N.stream_ptr()), "fr_op_l2norm_rows")
    torch.cuda.synchronize()
    ref = F.normalize(x.double(), dim=1)
    assert torch.allclose(xd.cpu().double(), ref, rtol=0, atol=1e-6)
    assert torch.count_nonzero(xd[3]) == 0


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("n", [8, 8 * 257, 8 * (1024 * 256 + 3)])
def test_amax(gpu, n, dtype):
    """amax_kernel: one vector, one block and a bit; 1024 blocks plus a 3-vector tail that only the grid-stride loop
    reaches.  The largest magnitude is negative, unique and among the last 8 elements.  16-bit -> f32 is exact, so
    the maximum over the slots equals x.abs().max() exactly; a slot holding a larger value keeps it."""
    g = torch.Generator().manual_seed(n % 1000)
    x = torch.randn(n, generator=g).to(TORCH_DT[dtype])
    top = -(x.float().abs().max() * 2 + 1).to(TORCH_DT[dtype])
    x[n - 3] = top
    assert (x.float().abs() == top.float().abs()).sum() == 1
    xd = x.to(gpu)
    dt = N.FR_DTYPE[dtype]
    for slots in (1, 64):
        am = torch.zeros(slots, device=gpu)
        N.check(N.lib().fr_op_amax(xd.data_ptr(), n, dt, am.data_ptr(), slots, N.stream_ptr()), "fr_op_amax")
        torch.cuda.synchronize()
        assert am.max().item() == top.float().abs().item()
        assert bool((am >= 0).all())
        am = torch.zeros(slots, device=gpu)
        am[0] = 1e9  # every slot the kernel raises holds max(old, new): the larger old value stays
        am[slots - 1] = 1e9
        N.check(N.lib().fr_op_amax(xd.data_ptr(), n, dt, am.data_ptr(), slots, N.stream_ptr()), "fr_op_amax")
        torch.cuda.synchronize()
        assert am[0].item() == 1e9 and am[slots - 1].item() == 1e9 and am.max().item() == 1e9
    am = torch.zeros(1, device=gpu)
    with pytest.raises(RuntimeError, match="fr_op_amax"):
        N.check(N.lib().fr_op_amax(xd.data_ptr(), 12, dt, am.data_ptr(), 1, N.stream_ptr()), "fr_op_amax")
    assert am.item() == 0
