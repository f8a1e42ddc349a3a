"""Float64 restatement of the e4m3 kernels (conv_fp8.hip, conv_stage8.hip), in the style of tests/stage_ref.py and on
its helpers (plain numpy / torch on the CPU; nothing here comes from a device output).  tests/test_fp8_ref.py checks
this file on the CPU, tests/test_gpu_fp8_exact.py uses it.

The activation scale.  act_exp(amax, clamp) is the smallest integer e with amax <= 448 2^e, from the exponent field
(math.frexp; no float logarithm), 0 for amax 0, clamped to the kernels' documented ranges: CLAMP_CONV = 60
(conv_fp8.hip), CLAMP_STAGE = 100 (conv_stage8.hip).

The activation quantisation.  quant(v, e) = e4m3(v / 2^e) 2^e through torch.float8_e4m3fn (round to nearest, ties
to even, subnormals below 2^-6, flush below 2^-10), for |v| <= 448 2^e; with the next e4m3 value below and above.

One conv (conv_ref), on the stored bf16 input I and the e4m3 weight values `codes` with their per-channel scale:

    v    = conv(quant(I, e), codes wscale) + bias [or bias9[class of the pixel]] + res
    ref  = act(v)                      act 0: none, 1: ReLU, 2: PReLU(slope)
    ref2 = ref aff_s + aff_b           (the second output; the kernel applies the affine to its f32 value, not to the
                                        stored one)

The bound follows stage_ref's derivation.  An e4m3 x e4m3 product has 8 significant bits and the power-of-two
activation scale is exact, so only the summation rounds: first order, a sum of K products in any order costs at most
(K + c) u_acc times the sum of the absolute terms L1, c = 4 for the weight scale, the bias, the residual and the
PReLU's product:

    acc_   = (K + 4) u_acc L1,  L1 = conv(|quant(I)|, |codes wscale|) + |bias| + |res|   (PReLU: times max(1, |slope|),
                                                                   so that a sign flip within the bound stays inside)
    bound  = acc_ + h (|ref| + acc_)                               h = 2^-8, half a bf16 unit in the last place
    acc2_  = |aff_s| acc_ + 2 u (|ref aff_s| + |aff_b|)            (the affine's product and sum), u = 2^-24
    bound2 = acc2_ + h (|ref2| + acc2_)

u_acc.  With one f32 rounding per addition u_acc would be u = 2^-24, and the CPU's float32 evaluations stay inside that
(tests/test_fp8_ref.py).  The 128-deep block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4) does not: measured on an
MI355X over the op cases of tests/fp8_op.py, the largest (|stored - ref| - h |ref|) / ((K + 4) L1) is 4.477 u (case
b-res-s64, K = 64, one MFMA per element: |error| 4.1e-5 on L1 = 1.57, 2^-15.2 of L1, where K u L1 is 6e-6) and 1.137 u
at K = 576 (b-relu-res-xs-over); every other case stays below u.  The excess has no structure: 7 of 1920 and 1 of 17496
elements, no two in one pixel or channel, 35 of 1920 stored values differ from the rounded float64 sum spread over 21
of 30 pixels and 26 of 64 channels, and the three tiles (other lanes, waves and workgroups for the same element) store
the same values bit for bit -- it is the instruction's own summation of the 128 products of a block, not a lane, tile,
pixel or K-step of the kernel.  No activation quantisation explains it (exponent e - 1 .. e + 2, ties away, flushed or
finer subnormals all fit worse than e4m3 RNE at e), and the converter table of test_gpu_fp8_exact.py is exact.  So, by
the rule "twice the worst measured figure", U_ACC = 2 x 4.477 u.  h is not widened.

Every assertion is |stored - ref| / bound <= 1 (stage_ref.ratio); no tolerance is chosen by hand.

The e4m3 stage (chain8, at the end of this file) is restated value for value instead: with synthetic weights every
f32 summation difference flips e4m3 roundings of conv1's output, which the kernel never stores, so a per-element bound
is useless there; with dyadic selection weights (stage8_state_dict) every sum has two terms and is exact.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import stage_ref as SR
from tests.stage_ref import HALF_ULP, U, pixel_class, ratio, rnd  # noqa: F401  (re-exported)

H8 = HALF_ULP[torch.bfloat16]
U_ACC = 2 * 4.477 * U  # the block-scaled MFMA's summation, measured (module docstring)
CLAMP_CONV, CLAMP_STAGE = 60, 100


# ----------------------------------------------------------------------------- the scale and the quantisation
def act_exp(amax, clamp):
    """The smallest integer e with amax <= 448 2^e (448 = 0.875 2^9), 0 for amax 0, clamped to +-clamp."""
    a = float(amax)
    if not a > 0:
        return 0
    if math.isinf(a):
        return clamp
    m, x = math.frexp(a)  # a = m 2^x, 0.5 <= m < 1
    e = x - 9 if m <= 0.875 else x - 8
    return max(-clamp, min(clamp, e))


def decode(codes_u8):
    """e4m3 bytes -> their values as float64 (NaN for 0x7f / 0xff)."""
    t = torch.from_numpy(np.ascontiguousarray(codes_u8, dtype=np.uint8))
    return t.view(torch.float8_e4m3fn).to(torch.float64).numpy()


def encode(v):
    """float values -> e4m3 bytes (round to nearest even)."""
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(torch.float8_e4m3fn)
    return t.view(torch.uint8).numpy()


# the 253 finite e4m3 values, ascending (-0 = +0)
GRID = np.unique(decode(np.array([c for c in range(256) if c & 0x7f != 0x7f], np.uint8)))


def quant(v, e):
    """(q, below, above): q = e4m3(v / 2^e) 2^e as float64, and the next e4m3 value (times 2^e) below and above q
    (q itself at +-448 2^e).  v is float32-representable with |v| <= 448 2^e; e a scalar or broadcastable."""
    v = np.asarray(v, np.float64)
    s = np.ldexp(1.0, np.asarray(e, np.int64))
    x = v / s
    assert np.all(np.abs(x) <= 448), "quant: |v| > 448 2^e"
    q = torch.from_numpy(np.ascontiguousarray(x)).to(torch.float32).to(torch.float8_e4m3fn).to(torch.float64).numpy()
    k = np.searchsorted(GRID, q)
    return q * s, GRID[np.maximum(k - 1, 0)] * s, GRID[np.minimum(k + 1, len(GRID) - 1)] * s


def quant_half_away(v, e):
    """The planted fault of test_fp8_ref.py: the same grid, ties rounded away from zero."""
    v = np.asarray(v, np.float64)
    s = np.ldexp(1.0, np.asarray(e, np.int64))
    x = np.abs(v / s)
    k = np.clip(np.searchsorted(GRID, x), 1, len(GRID) - 1)
    lo, hi = GRID[k - 1], GRID[k]
    return np.sign(v) * np.where(x - lo < hi - x, lo, hi) * s


# ----------------------------------------------------------------------------- one conv
def out_hw(H, W, kh, kw, stride, pad):
    return (H + 2 * pad[0] - kh) // stride[0] + 1, (W + 2 * pad[1] - kw) // stride[1] + 1


def conv_sum(I, w, stride, pad, compute=np.float64, perm=None):
    """stage_ref.conv_sum for any tap grid, stride pair and padding: I [B, H, W, C], w [N, kh, kw, C] ->
    [B, OH, OW, N].  The square, symmetric cases go through stage_ref.conv_sum itself; float32: per tap and 32
    channels one float64 sum rounded to float32, the steps accumulated in float32; `perm` permutes the channels and
    walks the taps backwards."""
    B, H, W, C = I.shape
    N, kh, kw = w.shape[:3]
    if kh == kw and stride[0] == stride[1] and tuple(pad) == (kh // 2, kh // 2):
        return SR.conv_sum(I, w, stride[0], compute, perm)
    if perm is not None:
        I, w = I[..., perm], w[..., perm]
    OH, OW = out_hw(H, W, kh, kw, stride, pad)
    Ip = np.zeros((B, H + 2 * pad[0], W + 2 * pad[1], C))
    Ip[:, pad[0]:pad[0] + H, pad[1]:pad[1] + W] = I
    cols = np.zeros((B * OH * OW, kh * kw, C))
    for r in range(kh):
        for s in range(kw):
            cols[:, r * kw + s] = Ip[:, r:r + (OH - 1) * stride[0] + 1:stride[0],
                                     s:s + (OW - 1) * stride[1] + 1:stride[1]].reshape(-1, C)
    wt = np.asarray(w, np.float64).reshape(N, kh * kw, C)
    if compute == np.float64:
        return (cols.reshape(len(cols), -1) @ wt.reshape(N, -1).T).reshape(B, OH, OW, N)
    assert compute == np.float32
    acc = np.zeros((len(cols), N), np.float32)
    taps = range(kh * kw) if perm is None else range(kh * kw - 1, -1, -1)
    for t in taps:
        for c in range(0, C, 32):
            acc = acc + (cols[:, t, c:c + 32] @ wt[:, t, c:c + 32].T).astype(np.float32)
    return acc.reshape(B, OH, OW, N)


def conv_ref(I, codes, wscale, e, stride, pad, bias=None, bias9=None, res=None, act=0, slope=None, aff=None,
             compute=np.float64, perm=None, quantize=quant):
    """The op on stored values: I [B, H, W, Cin] (the input's channel slice), codes [Cout, kh, kw, Cin] e4m3 values,
    wscale [Cout], e the activation exponent (act_exp of the amax the kernel is given), bias [Cout] or bias9
    [9, Cout], res [B, OH, OW, Cout] (the residual's slice), act 0 / 1 / 2 with slope [Cout], aff = (aff_s, aff_b).
    float64: (ref, bound), with aff (ref, bound, ref2, bound2), all unrounded.  compute=float32: the same arithmetic
    as a kernel may do it (the accumulation of conv_sum, the epilogue in float32), (v, v2 or None), no bounds.
    `quantize`: the activation quantisation (test_fp8_ref.py plants another)."""
    I = np.asarray(I, np.float64)
    codes = np.asarray(codes, np.float64)
    ws = np.asarray(wscale, np.float64)
    K = codes.shape[1] * codes.shape[2] * codes.shape[3]
    qI = quantize(I, e)
    qI = qI[0] if isinstance(qI, tuple) else qI
    f64 = compute == np.float64
    OH, OW = out_hw(I.shape[1], I.shape[2], codes.shape[1], codes.shape[2], stride, pad)
    if f64:
        v = conv_sum(qI, codes * ws[:, None, None, None], stride, pad)
    else:  # the kernel's order: the sum of q x code, times the channel's scale
        v = conv_sum(qI, codes, stride, pad, np.float32, perm) * ws.astype(np.float32)
    b = np.zeros((1, 1, 1, len(ws)))
    if bias9 is not None:
        assert tuple(stride) == (1, 1) and tuple(pad) == (1, 1) and codes.shape[1:3] == (3, 3)
        b = np.asarray(bias9, np.float64)[pixel_class(OH, OW)][None]
    elif bias is not None:
        b = np.asarray(bias, np.float64)[None, None, None, :]
    r = np.zeros((1, 1, 1, 1)) if res is None else np.asarray(res, np.float64)
    v = v + b.astype(compute) + r.astype(compute)
    sl = None if slope is None else np.asarray(slope, np.float64)
    if act == 1:
        ref = np.maximum(v, 0)
    elif act == 2:
        ref = np.where(v > 0, v, v * sl.astype(compute))
    else:
        ref = v
    ref2 = None
    if aff is not None:
        a_s, a_b = (np.asarray(t, np.float64) for t in aff)
        ref2 = ref * a_s.astype(compute) + a_b.astype(compute)
    if not f64:
        assert ref.dtype == np.float32
        return ref, ref2
    acc_ = (K + 4) * U_ACC * (conv_sum(np.abs(qI), np.abs(codes) * ws[:, None, None, None], stride, pad) + np.abs(b) + np.abs(r))
    if act == 2:
        acc_ = acc_ * np.maximum(1.0, np.abs(sl))
    bound = acc_ + H8 * (np.abs(ref) + acc_)
    if aff is None:
        return ref, bound
    acc2_ = np.abs(a_s) * acc_ + 2 * U * (np.abs(ref * a_s) + np.abs(a_b))
    return ref, bound, ref2, acc2_ + H8 * (np.abs(ref2) + acc2_)


# ----------------------------------------------------------------------------- the convs of the model
def model_convs():
    """[(conv, kind, input tensor, residual tensor or None, output tensor, stride, pad)] of IResNet100's blocks as
    the per-conv plan runs them; kind in {'conv1', 'conv2', 'downsample'}.  conv1: 3x3, b9, PReLU; the downsample of a
    .0 block: 1x1 stride 2 into a tensor of its own (an e4m3 conv2 has no K-concatenated projection), which is that
    block's residual."""
    out, x = [], "prelu"
    for layer, nblk in ((1, 3), (2, 13), (3, 30), (4, 3)):
        for i in range(nblk):
            pre = f"layer{layer}.{i}"
            out.append((pre + ".conv1", "conv1", x, None, pre + ".prelu", 1, 1))
            res = x
            if i == 0:
                out.append((pre + ".downsample", "downsample", x, None, pre + ".downsample", 2, 0))
                res = pre + ".downsample"
            out.append((pre + ".conv2", "conv2", pre + ".prelu", res, pre, 2 if i == 0 else 1, 1))
            x = pre
    return out


def model_conv_ref(I, q, conv, kind, e, stride, pad, X=None):
    """conv_ref for a conv of the model from the quantised folded weights q (weights.quantize_fp8)."""
    b9 = q.get(conv + ".b9") if kind == "conv1" else None
    return conv_ref(I, q[conv + ".w"], q[conv + ".wscale"], e, (stride, stride), (pad, pad),
                    bias=None if b9 is not None else q[conv + ".b"], bias9=b9, res=X,
                    act=2 if kind == "conv1" else 0, slope=q.get(conv + ".slope") if kind == "conv1" else None)


# ----------------------------------------------------------------------------- the e4m3 stage, value for value
STAGE8 = (16, 29)   # layer3.16 .. layer3.29: the blocks of weights.FP8_PLAN, which conv_stage8.hip runs
CAP = 1e-3          # the largest share of a tensor that the ambiguity rule may exclude


def stage8_magnitude(pre, member):
    """selection_state_dict's magnitudes for the e4m3 stage: 7/8 on conv1 and 7/32 on conv2 of layer3.16 .. 29."""
    if pre.startswith("layer3.") and STAGE8[0] <= int(pre.split(".")[1]) <= STAGE8[1]:
        return 0.875 if member == "conv1" else 0.21875
    return None


def stage8_state_dict(seed=0):
    return SR.selection_state_dict(seed, stage8_magnitude)


def _f32_below_above(v):
    """The float32 neighbours of float64 v: (largest float32 <= v, smallest float32 >= v), as float64."""
    r = v.astype(np.float32)
    lo = np.where(r.astype(np.float64) > v, np.nextafter(r, np.float32(-np.inf)), r).astype(np.float64)
    hi = np.where(r.astype(np.float64) < v, np.nextafter(r, np.float32(np.inf)), r).astype(np.float64)
    return lo, hi


def _image_exp(lo, hi):
    """Per image the stage's exponent from the interval [lo, hi] of every element: (e of the largest possible
    maximum, whether the smallest possible maximum gives another e)."""
    top = np.maximum(np.abs(lo), np.abs(hi)).reshape(len(lo), -1).max(axis=1)
    low = np.where((lo <= 0) & (hi >= 0), 0.0, np.minimum(np.abs(lo), np.abs(hi))).reshape(len(lo), -1).max(axis=1)
    e = np.array([act_exp(np.float32(a), CLAMP_STAGE) for a in top])
    return e, e != np.array([act_exp(np.float32(a), CLAMP_STAGE) for a in low])


def chain8(x, q, first=STAGE8[0], last=STAGE8[1], fault=None):
    """conv_stage8.hip restated free-running from x = layer3.(first - 1) [B, 14, 14, 256] (stored bf16 values) with
    selection weights q = quantize_fp8(fold(stage8_state_dict())): one e4m3 value 448 per output channel, scales 2^-9
    / 2^-11, PReLU slopes powers of two, no conv2 bias.  Per block, with a per-image exponent at each conv input:

        t = prelu(f32(0.875 quant(x, e1)[selected] + b9[class]))         kept in f32, never stored
        y = bf16(f32(0.21875 quant(t, e2)[selected] + x))                the block output, the next block's x

    Each sum has two dyadic terms and is exact in float64, but it may need more than 24 bits, and the MFMA's rounding
    of it is not specified.  So three chains run side by side: `lo` rounds every such sum to the float32 below, `hi`
    to the one above, the value itself to nearest.  Every step (a positive weight, quant, PReLU with a positive
    slope, the roundings) is monotone, so whatever the hardware rounds, its value lies in [lo, hi] while the exponents
    agree; an image whose exponent differs between the smallest and the largest possible maximum is excluded from
    there on.  Returns {tensor name: (value, excluded)}: excluded = lo != hi for the element, or its image lost its
    exponent -- exactly the elements whose e4m3 code (conv1), bf16 value (conv2) or exponent depends on the rounding
    of some sum, and what follows from them.
    `fault` (tests/test_fp8_ref.py): ('halo', conv, image): the conv reads the image's row 13 where the zero row -1
    belongs; ('exp', conv, image, from image): the image's exponent taken from another image."""
    x = np.asarray(x, np.float64)
    B = len(x)
    X = [x, x, x]  # lo, value, hi
    lost = np.zeros(B, bool)
    out = {}

    def conv(I, name, img_halo):
        w = np.asarray(q[name + ".w"], np.float64) * np.asarray(q[name + ".wscale"], np.float64)[:, None, None, None]
        assert (w >= 0).all() and (np.count_nonzero(w.reshape(len(w), -1), axis=1) <= 1).all(), "chain8 needs selection weights"
        y = SR.conv_sum(I, w)
        if img_halo is not None:  # a stale halo: row 13 of the image in the place of the zero row above row 0
            ext = np.concatenate([I[img_halo:img_halo + 1, 13:14], I[img_halo:img_halo + 1]], axis=1)
            y[img_halo, 0] = SR.conv_sum(ext, w)[0, 1]
        return y

    def exps(name, lo, hi):
        nonlocal lost
        e, amb = _image_exp(lo, hi)
        lost = lost | amb
        if fault and fault[0] == "exp" and fault[1] == name:
            e[fault[2]] = e[fault[3]]
        return e.reshape(B, 1, 1, 1)

    for i in range(first, last + 1):
        p = f"layer3.{i}"
        c1, c2 = p + ".conv1", p + ".conv2"
        slope = np.asarray(q[c1 + ".slope"], np.float64)
        assert (slope > 0).all() and (np.frexp(slope)[0] == 0.5).all() and not np.any(q[c2 + ".b"])
        b9 = np.asarray(q[c1 + ".b9"], np.float64)[pixel_class(14, 14)][None]
        halo = {c: fault[2] if fault and fault[0] == "halo" and fault[1] == c else None for c in (c1, c2)}
        e1 = exps(c1, X[0], X[2])
        S = [conv(quant(v, e1)[0], c1, halo[c1]) + b9 for v in X]
        T = [SR.prelu(_f32_below_above(S[0])[0], slope), SR.prelu(S[1].astype(np.float32).astype(np.float64), slope),
             SR.prelu(_f32_below_above(S[2])[1], slope)]
        e2 = exps(c2, T[0], T[2])
        S = [conv(quant(v, e2)[0], c2, halo[c2]) + xv for v, xv in zip(T, X)]
        X = [rnd(_f32_below_above(S[0])[0], torch.bfloat16), rnd(S[1].astype(np.float32).astype(np.float64), torch.bfloat16),
             rnd(_f32_below_above(S[2])[1], torch.bfloat16)]
        out[p] = (X[1], (X[0] != X[2]) | lost[:, None, None, None])
    return out
