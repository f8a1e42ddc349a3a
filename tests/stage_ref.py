"""Float64 restatement of the IResNet100 stage kernels (conv_stage.hip, conv_split_stage.hip with their tail convs,
conv_trans.hip), the float32 error bound of one stage conv, and exact "selection" weights (plain numpy / torch on
the CPU; nothing here comes from a device output).  tests/fused_ref.py is the same thing for the ResNet-50 /
InceptionResnetV1 kernels; tests/test_stage_ref.py checks this file on the CPU, tests/test_gpu_stage_exact.py uses it.

One conv of a stage.  The input is the stored 16-bit tensor I (NHWC, exact values), the weights are those of
weights.fold_state_dict("iresnet100", sd) rounded to the storage type, b9 / b / slope stay f32:

    conv1 of block i   ref = prelu(conv3x3(I, w) + b9[class of the pixel], slope)   I = layerL.(i-1) -> layerL.i.prelu
    conv2 of block i   ref = conv3x3(T, w) + b + X             T = layerL.i.prelu, X = layerL.(i-1) -> layerL.i
    tail               conv1 of layer3.0 on layer2.12 -> layer3.0.prelu, of layer4.0 on layer3.29 -> layer4.0.prelu
                       (3x3 C -> 2C with b9 and PReLU; computed by the stage kernel on its final patch)

The class of a pixel is 3 rc + cc, rc / cc = 0, 1, 2 for the first, an interior, the last row / column
(weights._fold_pre_bn_3x3).  The convolutions are float64 matrix products over conv_train_ref.im2col.

The bound (conv_ref's second result), as tests/conv_train_ref.py computes its own: with u = 2^-24, first order, a sum of n terms in
any order costs at most (n + c) u times the sum of the absolute terms.  n = 9 C products, c = 4 for the bias (the
residual), the PReLU's fma and its rounded (slope - 1):

    acc_  = (9 C + 4) u (conv3x3(|I|, |w|) + |bias| + |X|)      (PReLU side: times max(1, |slope|), so that a sign flip
                                                                  within the bound stays inside it)
    bound = acc_ + h (|ref| + acc_)                             h = half a unit in the last place of the storage type,
                                                                  relative: 2^-8 (bf16), 2^-11 (f16; + 2^-25 absolute for
                                                                  its subnormals)

Every assertion is |stored - ref| / bound <= 1 (ratio); no tolerance is chosen by hand.

The transition (layer1.0, conv_trans.hip) is restated like fused_ref._bottleneck: prelu -> conv1 (3x3, b9, PReLU),
rounded once to the storage type, -> conv2 3x3 stride 2 with the 1x1 stride-2 downsample in the same accumulation and
the two biases added in f32, rounded to the storage type.  `chain` restates a whole stage the same way (every conv
output rounded), free-running from the stage's input.  dtype=None: no rounding at all, of weights or activations
(the plain network, for the check against the oracle).  `compute` / `perm_seed`: the same arithmetic in another type
and with the input channels of every conv permuted (another summation order), for the detector checks.
"""
from __future__ import annotations

import numpy as np
import torch

from facerecognition_amd import weights as Wt
from tests.conv_train_ref import im2col, out_size
from tests.fused_ref import selected_position, slice_stats  # noqa: F401  (slice_stats is re-exported)

ARCH = "iresnet100"
U = 2.0 ** -24
HALF_ULP = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
# stage -> (layer, H = W, C, last block, block whose conv1 is the stage's tail or None)
STAGES = {"layer1": (1, 56, 64, 2, None), "layer2": (2, 28, 128, 12, "layer3.0"), "layer3": (3, 14, 256, 29, "layer4.0")}
# the stage's line of fr_debug_plan ends with its output tensor (tests/test_gpu_stage.py asserts the same)
PLAN_END = {"layer1": "layer1.2", "layer2": "layer2.12", "layer3": "layer3.29"}


def stage_convs(stage):
    """[(conv, kind, input tensor, residual tensor or None, output tensor)] in the order the kernel runs them;
    kind in {'conv1', 'conv2', 'tail'}."""
    L, _, _, last, tail = STAGES[stage]
    out = []
    for i in range(1, last + 1):
        p, q = f"layer{L}.{i}", f"layer{L}.{i - 1}"
        out.append((p + ".conv1", "conv1", q, None, p + ".prelu"))
        out.append((p + ".conv2", "conv2", p + ".prelu", q, p))
    if tail:
        out.append((tail + ".conv1", "tail", f"layer{L}.{last}", None, tail + ".prelu"))
    return out


def stage_tensors(stage):
    """Every tensor the stage reads or writes, the input first."""
    names = [f"layer{STAGES[stage][0]}.0"]
    for _, _, _, _, o in stage_convs(stage):
        names.append(o)
    return names


# ----------------------------------------------------------------------------- arithmetic
def rnd(v, dtype, compute=np.float64):
    """numpy v -> f32 -> the storage type -> compute (the kernels convert their f32 value); dtype None: v."""
    if dtype is None:
        return v
    return torch.from_numpy(np.ascontiguousarray(v)).to(torch.float32).to(dtype).to(torch.float64).numpy().astype(compute)


def weight(fw, name, dtype):
    """The conv's folded weights [Cout, k, k, Cin] as float64, rounded to the storage type."""
    return rnd(np.asarray(fw[name + ".w"], np.float64), dtype)


def pixel_class(H, W):
    """[H, W] border class 3 rc + cc of a 3x3 / stride 1 / pad 1 output pixel."""
    rc = np.ones(H, np.int64)
    rc[0], rc[-1] = 0, 2
    cc = np.ones(W, np.int64)
    cc[0], cc[-1] = 0, 2
    return 3 * rc[:, None] + cc[None, :]


def conv_sum(I, w, stride=1, compute=np.float64, perm=None):
    """I [B, H, W, C], w [N, k, k, C] -> [B, OH, OW, N].  float64: one matrix product over the im2col.  float32: as
    the MFMA kernels sum, K-step by K-step -- the 32 products of one tap and 32 channels summed in float64 and rounded
    to float32, the K-steps accumulated in float32 (one rounding each) -- which makes the result independent of the
    host's BLAS; `perm` permutes the input channels of both operands, which regroups the K-steps, and walks the taps
    backwards (another order of the same sum)."""
    B, H, W, C = I.shape
    N, k = w.shape[0], w.shape[1]
    if perm is not None:
        I, w = I[..., perm], w[..., perm]
    cols = im2col(np.asarray(I, np.float64), k, stride)
    shape = (B, out_size(H, k, stride), out_size(W, k, stride), N)
    if compute == np.float64:
        return (cols @ np.ascontiguousarray(w.reshape(N, -1).T)).reshape(shape)
    assert compute == np.float32
    cols, wt = cols.reshape(-1, k * k, C), w.reshape(N, k * k, C)
    acc = np.zeros((cols.shape[0], N), np.float32)
    taps = range(k * k) if perm is None else range(k * k - 1, -1, -1)
    for t in taps:
        for c in range(0, C, 32):
            acc = acc + (cols[:, t, c:c + 32] @ wt[:, t, c:c + 32].T).astype(np.float32)
    return acc.reshape(shape)


def prelu(v, slope):
    return np.where(v > 0, v, v * slope)


def conv_ref(I, fw, name, kind, dtype, X=None, with_bound=True, compute=np.float64, perm=None):
    """One stage conv on stored values: (ref, bound), both [B, H, W, Cout] and unrounded; bound None without
    with_bound.  kind 'conv1' / 'tail': b9 and PReLU; 'conv2': bias and the residual X."""
    I = np.asarray(I, np.float64)
    w = weight(fw, name, dtype)
    B, H, W, C = I.shape
    acc = conv_sum(I, w, 1, compute, perm)
    if kind == "conv2":
        bias = np.asarray(fw[name + ".b"], np.float64)[None, None, None, :]
        res = np.asarray(X, np.float64)
        ref = acc + bias.astype(compute) + res.astype(compute)
        slope_f = 1.0
    else:
        b9 = np.asarray(fw[name + ".b9"], np.float64)  # [9, Cout]
        bias = b9[pixel_class(H, W)][None]  # [1, H, W, Cout]
        slope = np.asarray(fw[name + ".slope"], np.float64)
        res = 0.0
        ref = prelu(acc + bias.astype(compute), slope.astype(compute))
        slope_f = np.maximum(1.0, np.abs(slope))
    if not with_bound:
        return ref, None
    assert compute == np.float64
    acc_ = (9 * C + 4) * U * (conv_sum(np.abs(I), np.abs(w)) + np.abs(bias) + np.abs(res)) * slope_f
    bound = acc_ + HALF_ULP[dtype] * (np.abs(ref) + acc_)
    if dtype == torch.float16:
        bound = bound + 2.0 ** -25
    return ref, bound


def ratio(stored, ref, bound):
    """|stored - ref| / bound, elementwise (0 where both vanish)."""
    err = np.abs(np.asarray(stored, np.float64) - ref)
    return np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))


def chain(stage, x, fw, dtype, compute=np.float64, perm_seed=None):
    """The whole stage from its input x = layerL.0 [B, H, W, C]: {tensor name: float64 [B, H, W, C']} of every conv
    output, each rounded to the storage type (dtype None: nothing rounded)."""
    rng = None if perm_seed is None else np.random.default_rng(perm_seed)
    out = {f"layer{STAGES[stage][0]}.0": np.asarray(x, np.float64)}
    for name, kind, tin, tres, tout in stage_convs(stage):
        I = out[tin]
        perm = None if rng is None else rng.permutation(I.shape[3])
        ref, _ = conv_ref(I, fw, name, kind, dtype, None if tres is None else out[tres], False, compute, perm)
        out[tout] = rnd(ref, dtype).astype(np.float64)
    return out


def transition(x, fw, dtype, compute=np.float64, perm_seed=None):
    """layer1.0 from the stem's output x = prelu [B, 112, 112, 64]: {'layer1.0.prelu': t, 'layer1.0': y}."""
    rng = None if perm_seed is None else np.random.default_rng(perm_seed)
    perm = (lambda n: None) if rng is None else rng.permutation
    p = "layer1.0"
    x = np.asarray(x, np.float64)
    ts, ys = [], []
    bsum = (np.asarray(fw[p + ".conv2.b"], np.float32) + np.asarray(fw[p + ".downsample.b"], np.float32)).astype(np.float32)
    w2, wd = weight(fw, p + ".conv2", dtype), weight(fw, p + ".downsample", dtype)
    for i in range(x.shape[0]):  # per image: the 112 x 112 im2col is 58 MB in float64
        xi = x[i:i + 1]
        t, _ = conv_ref(xi, fw, p + ".conv1", "conv1", dtype, None, False, compute, perm(64))
        t = rnd(t, dtype).astype(np.float64)
        # conv2 and the K-concatenated downsample: one accumulation (the order of the K-steps is the kernel's own)
        pm = perm(128)
        if pm is None:
            acc = conv_sum(t, w2, 2, compute) + conv_sum(xi, wd, 2, compute)
        else:  # one sum of 9 x 64 + 64 products in a permuted order: the downsample's join tap 4 of a 128-channel conv
            wj = np.zeros((64, 3, 3, 128))
            wj[..., :64] = w2
            wj[:, 1, 1, 64:] = wd[:, 0, 0, :]
            tj = np.concatenate([t, xi], axis=3)
            acc = conv_sum(tj, wj, 2, compute, pm)
        y = acc + bsum.astype(compute)[None, None, None, :]
        ts.append(t)
        ys.append(rnd(y, dtype).astype(np.float64))
    return {p + ".prelu": np.concatenate(ts), p: np.concatenate(ys)}


# ----------------------------------------------------------------------------- selection weights
def selection_convs():
    """[(block prefix, member, block index)], member in {'conv1', 'conv2', 'downsample'}: the convs of the four
    kernels.  conv1 takes the block's bn1 (pre-conv), bn2 and PReLU along, conv2 its bn3, the downsample its BN."""
    out, blk = [], 0
    for pre, members in ([("layer1.0", ("conv1", "conv2", "downsample"))] +
                         [(f"layer1.{i}", ("conv1", "conv2")) for i in (1, 2)] +
                         [(f"layer2.{i}", ("conv1", "conv2")) for i in range(1, 13)] +
                         [("layer3.0", ("conv1",))] +
                         [(f"layer3.{i}", ("conv1", "conv2")) for i in range(1, 30)] +
                         [("layer4.0", ("conv1",))]):
        out += [(pre, m, blk) for m in members]
        blk += 1
    return out


def unit_bn(eps, n=1 << 17):
    """(weight, running_var) as float32 whose eval-mode scale weight / sqrt(running_var + eps), evaluated in float64
    as weights._bn_affine does, is 1 to ~1e-12: the closest of n candidates.  (1, 1) gives 1 - 5e-6, and
    (f32(sqrt(1 + eps)), 1) is off by up to 2^-25: a shift that passes through such a scale (b9 = t2 + scale t1) would
    not fold to the exact f32 value.)"""
    rv = (np.float32(1) + np.arange(n, dtype=np.float64) * 2.0 ** -23).astype(np.float32)
    root = np.sqrt(rv.astype(np.float64) + eps)
    g = root.astype(np.float32)
    k = int(np.argmin(np.abs(g.astype(np.float64) / root - 1)))
    return g[k], rv[k]


def selection_state_dict(seed=0, magnitude=None):
    """synth_state_dict("iresnet100") with the convs of selection_convs replaced by selections:
      * every output channel n has one nonzero weight, at fused_ref.selected_position: 1 on conv1 and the downsample,
        2^-2 on conv2;
      * bn2, bn3 and the downsample BN fold to scale 1 (unit_bn); the conv2 and downsample biases are zero, the bn2
        shift t2 is a multiple of 1/16 in [-1/2, 1/2];
      * bn1 (the folded pre-conv BN) has scale 1 and a shift t1 that is a multiple of 1/16 with 9/16 <= |t1| <= 1, so
        that b9 = t2 + [the selected tap is inside the image] t1 is a nonzero multiple of 1/16 wherever t1 enters, and
        differs between border classes exactly where the selected tap leaves the image;
      * the PReLU slopes are 1/2, 1/4, 1/8, varying by channel.
    Every stored value of the four kernels is then (x + b9) or (x + b9) slope or (x + t / 4), correctly rounded: a
    sum of at most two exactly representable terms times a power of two, which no summation order can change.
    `magnitude`: a function (block prefix, member) -> the nonzero weight of that conv, or None for the value above
    (tests/fp8_ref.py: 0.875 and 0.21875 = 7/8 and 7/32, which weights.quantize_fp8 turns into the e4m3 value 448 with
    the scales 2^-9 and 2^-11 exactly; the folded pre-conv shift then enters b9 as 0.875 t1, still a short dyadic)."""
    sd = dict(Wt.synth_state_dict(ARCH))
    g, rv = unit_bn(Wt.BN_EPS[ARCH])

    def unit(bn, c, bias):
        sd[bn + ".weight"] = np.full(c, g, np.float32)
        sd[bn + ".running_var"] = np.full(c, rv, np.float32)
        sd[bn + ".running_mean"] = np.zeros(c, np.float32)
        sd[bn + ".bias"] = np.asarray(bias, np.float32)

    for pre, member, blk in selection_convs():
        key = pre + (".downsample.0.weight" if member == "downsample" else f".{member}.weight")
        shape = sd[key].shape
        cout, cin, kh, kw = shape
        tap, ci = selected_position(shape, blk)
        w = np.zeros((cout, cin, kh * kw), np.float32)
        mag = None if magnitude is None else magnitude(pre, member)
        w[np.arange(cout), ci, tap] = mag if mag is not None else (0.25 if member == "conv2" else 1.0)
        sd[key] = w.reshape(shape)
        if member == "conv2":
            unit(pre + ".bn3", cout, np.zeros(cout))
        elif member == "downsample":
            unit(pre + ".downsample.1", cout, np.zeros(cout))
        else:
            k = np.floor(Wt.splitmix_uniform(seed, "selection:" + pre + ".bn1", cin) * 16).clip(0, 15)
            unit(pre + ".bn1", cin, np.where(k < 8, 1.0, -1.0) * (9 + k % 8) / 16)
            u = Wt.splitmix_uniform(seed, "selection:" + pre + ".bn2", cout)
            unit(pre + ".bn2", cout, (np.floor(u * 17).clip(0, 16) - 8) / 16)
            sd[pre + ".prelu.weight"] = (2.0 ** -(1 + (7 * np.arange(cout) + blk) % 3)).astype(np.float32)
    return sd
