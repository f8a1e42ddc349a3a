"""Float64 restatements of the six fused ResNet-50 / InceptionResnetV1 groups (plain torch, CPU), the slice
statistics that compare a device tensor with them, and the exact "selection" weights.

One function per fused kind (include/frhip.h FR_OPT_FUSED_MASK).  Each takes the group's input tensor in NHWC,
holding exactly the stored 16-bit values (the stems: the u8 crops), and the folded weights of
weights.fold_state_dict, and returns {tensor name: NHWC float64 tensor} for the outputs the kernel stores:

    kind (mask bit)   input -> outputs                                      rounding points
    stem_r50 (64)     u8 crops -> backbone.maxpool                          conv1 + ReLU; the max-pool is exact
    bneck28 (32)      backbone.maxpool -> backbone.layer1.0 / .1 / .2       per block t1, t2, block output
    chain_r50 (16)    backbone.layer3.0 -> backbone.layer3.5                per block t1, t2, block output
    stem160 (2)       u8 crops -> model.conv2d_3b                           1a, 2a, 2b (max-pool exact), 3b
    chain35 (4)       model.conv2d_4b -> model.repeat_1.4                   per block t1, t2, b0, b1, t, b2, output
    chain17 (8)       model.mixed_6a -> model.repeat_2.9                    per block t1, t, b1, b0, output

`dtype` (torch.float16 / torch.bfloat16) is the storage type of the kernel's section: the weights are rounded to
it and every tensor named above is rounded to it where the kernel headers say the kernels round.  The kernels
accumulate in f32 and convert the f32 value, so a rounding point is f64 -> f32 -> 16 bit here too.  dtype=None:
no rounding at all, neither of weights nor of activations (the plain network, for the check against the oracle).
The two stems read (2u - 255) / 255 and the unrounded folded weights: the engine's hi/lo split of the stem
weights keeps ~16 mantissa bits, a residual common to both device paths and far below one storage rounding.

`compute` / `perm_seed` exist for the detector checks of test_fused_ref.py: the same chain evaluated in f32, with
the input channels of every conv permuted (another summation order)."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from facerecognition_amd import weights as Wt

KINDS = {  # kind -> (arch, mask bit, input tensor or None for the u8 crops, output tensors)
    "stem_r50": ("resnet50_arcface", 64, None, ("backbone.maxpool",)),
    "bneck28": ("resnet50_arcface", 32, "backbone.maxpool", ("backbone.layer1.0", "backbone.layer1.1", "backbone.layer1.2")),
    "chain_r50": ("resnet50_arcface", 16, "backbone.layer3.0", ("backbone.layer3.5",)),
    "stem160": ("irv1_facenet", 2, None, ("model.conv2d_3b",)),
    "chain35": ("irv1_facenet", 4, "model.conv2d_4b", ("model.repeat_1.4",)),
    "chain17": ("irv1_facenet", 8, "model.mixed_6a", ("model.repeat_2.9",)),
}
# a substring of the kind's fr_debug_plan line (tests/test_gpu_chain.py asserts the same ones)
PLAN_MARK = {"stem_r50": " 64 392 392 1 ", "bneck28": " 256 272 272 3 ", "chain_r50": " 1024 1088 1088 5 ",
             "stem160": "stem160 ", "chain35": " 256 300 300 5 ", "chain17": " 896 768 768 10 "}


class _Ctx:
    """Rounding and conv arithmetic of one restatement."""

    def __init__(self, dtype, compute=torch.float64, perm_seed=None):
        self.dtype, self.compute = dtype, compute
        self.rng = None if perm_seed is None else np.random.default_rng(perm_seed)

    def rnd(self, v):
        if self.dtype is None:
            return v
        return v.to(torch.float32).to(self.dtype).to(self.compute)

    def conv(self, x, fw, name, stride=1, pad=0, relu=True, res=None, round_w=True, extra_bias=None):
        """x NCHW; fw[name + '.w'] is [Cout, kh, kw, Cin] f32, '.b' [Cout] f32.  relu(conv + b (+ res)), unrounded."""
        w = torch.from_numpy(np.asarray(fw[name + ".w"])).permute(0, 3, 1, 2).to(self.compute)
        if round_w:
            w = self.rnd(w)
        b = np.asarray(fw[name + ".b"], np.float32)
        if extra_bias is not None:  # the engine adds the two f32 biases in f32
            b = (b + np.asarray(extra_bias, np.float32)).astype(np.float32)
        if self.rng is not None:
            p = torch.from_numpy(self.rng.permutation(x.shape[1]))
            x, w = x[:, p].contiguous(), w[:, p].contiguous()
        y = F.conv2d(x, w, torch.from_numpy(b).to(self.compute), stride=stride, padding=pad)
        if res is not None:
            y = y + res
        return torch.relu(y) if relu else y


def _nchw(x, compute=torch.float64):
    return torch.as_tensor(x).to(compute).permute(0, 3, 1, 2).contiguous()


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous().to(torch.float64)


def _crops(u8, compute):
    """ToTensor + Normalize(0.5, 0.5) of u8 crops: (2u - 255) / 255."""
    u = torch.as_tensor(np.asarray(u8)).to(compute)
    return ((2 * u - 255) / 255).permute(0, 3, 1, 2).contiguous()


# ----------------------------------------------------------------------------- ResNet-50
def stem_r50(u8, fw, dtype, compute=torch.float64, perm_seed=None):
    c = _Ctx(dtype, compute, perm_seed)
    y = c.rnd(c.conv(_crops(u8, compute), fw, "backbone.conv1", 2, 3, round_w=False))
    return {"backbone.maxpool": _nhwc(F.max_pool2d(y, 3, 2, 1))}


def _bottleneck(c, x, fw, pre, ds):
    t1 = c.rnd(c.conv(x, fw, pre + ".conv1"))
    t2 = c.rnd(c.conv(t1, fw, pre + ".conv2", 1, 1))
    if not ds:
        return c.rnd(c.conv(t2, fw, pre + ".conv3", res=x))
    # the downsample K-concatenated into conv3: one accumulation, the biases added
    d = c.conv(x, dict(fw, **{pre + ".downsample.b": np.zeros_like(fw[pre + ".downsample.b"])}), pre + ".downsample",
               relu=False)
    return c.rnd(c.conv(t2, fw, pre + ".conv3", res=d, extra_bias=fw[pre + ".downsample.b"]))


def bneck28(x, fw, dtype, compute=torch.float64, perm_seed=None):
    c = _Ctx(dtype, compute, perm_seed)
    x, out = _nchw(x, compute), {}
    for i in range(3):
        x = _bottleneck(c, x, fw, f"backbone.layer1.{i}", ds=i == 0)
        out[f"backbone.layer1.{i}"] = _nhwc(x)
    return out


def chain_r50(x, fw, dtype, compute=torch.float64, perm_seed=None):
    c = _Ctx(dtype, compute, perm_seed)
    x = _nchw(x, compute)
    for i in range(1, 6):
        x = _bottleneck(c, x, fw, f"backbone.layer3.{i}", ds=False)
    return {"backbone.layer3.5": _nhwc(x)}


# ----------------------------------------------------------------------------- InceptionResnetV1
def stem160(u8, fw, dtype, compute=torch.float64, perm_seed=None):
    c = _Ctx(dtype, compute, perm_seed)
    y = c.rnd(c.conv(_crops(u8, compute), fw, "model.conv2d_1a", 2, 0, round_w=False))
    y = c.rnd(c.conv(y, fw, "model.conv2d_2a"))
    y = c.rnd(c.conv(y, fw, "model.conv2d_2b", 1, 1))
    y = F.max_pool2d(y, 3, 2)
    return {"model.conv2d_3b": _nhwc(c.rnd(c.conv(y, fw, "model.conv2d_3b")))}


def _cat_conv2d(c, cat, fw, p, x):
    return c.rnd(c.conv(cat, fw, p + "conv2d", res=x))


def chain35(x, fw, dtype, compute=torch.float64, perm_seed=None, blocks=5):
    c = _Ctx(dtype, compute, perm_seed)
    x = _nchw(x, compute)
    for i in range(blocks):
        p = f"model.repeat_1.{i}."
        t1 = c.rnd(c.conv(x, fw, p + "branch1.0"))
        t2 = c.rnd(c.conv(x, fw, p + "branch2.0"))
        b0 = c.rnd(c.conv(x, fw, p + "branch0"))
        b1 = c.rnd(c.conv(t1, fw, p + "branch1.1", 1, 1))
        t = c.rnd(c.conv(t2, fw, p + "branch2.1", 1, 1))
        b2 = c.rnd(c.conv(t, fw, p + "branch2.2", 1, 1))
        x = _cat_conv2d(c, torch.cat((b0, b1, b2), 1), fw, p, x)
    return {f"model.repeat_1.{blocks - 1}": _nhwc(x)}


def chain17(x, fw, dtype, compute=torch.float64, perm_seed=None, blocks=10):
    c = _Ctx(dtype, compute, perm_seed)
    x = _nchw(x, compute)
    for i in range(blocks):
        p = f"model.repeat_2.{i}."
        t1 = c.rnd(c.conv(x, fw, p + "branch1.0"))
        t = c.rnd(c.conv(t1, fw, p + "branch1.1", 1, (0, 3)))
        b1 = c.rnd(c.conv(t, fw, p + "branch1.2", 1, (3, 0)))
        b0 = c.rnd(c.conv(x, fw, p + "branch0"))
        x = _cat_conv2d(c, torch.cat((b0, b1), 1), fw, p, x)
    return {f"model.repeat_2.{blocks - 1}": _nhwc(x)}


RESTATE = {"stem_r50": stem_r50, "bneck28": bneck28, "chain_r50": chain_r50, "stem160": stem160, "chain35": chain35,
           "chain17": chain17}


# ----------------------------------------------------------------------------- statistics
def slice_stats(y, ref):
    """y, ref [B, H, W, C].  Per image the error |y - ref| is divided by that image's RMS of ref; returns the worst
    value over the batch of (a) the largest single-element error, (b) the largest per-pixel RMS of the error over
    channels, (c) the largest per-channel RMS of the error over pixels."""
    y, ref = torch.as_tensor(y).to(torch.float64), torch.as_tensor(ref).to(torch.float64)
    assert y.shape == ref.shape and y.dim() == 4
    rms = ref.pow(2).mean(dim=(1, 2, 3), keepdim=True).sqrt()
    e = (y - ref) / rms
    elem = e.abs().amax()
    pix = e.pow(2).mean(dim=3).sqrt().amax()
    chan = e.pow(2).mean(dim=(1, 2)).sqrt().amax()
    return float(elem), float(pix), float(chan)


# ----------------------------------------------------------------------------- selection weights
# The member convs of the chain and Bottleneck groups (kinds 4, 8, 16, 32); value: (key of the conv weight, key
# prefix of its BN or None for a biased conv, kind of conv).  "res": the conv that adds the residual (or carries the
# K-concatenated downsample): weight 2^-2 after folding, no bias.
def selection_convs(arch):
    """[(conv weight key, BN prefix or None, role, block index)], role in {'plain', 'res', 'ds'}."""
    out = []
    if arch == "resnet50_arcface":
        for blk, pre in enumerate([f"backbone.layer1.{i}" for i in range(3)] + [f"backbone.layer3.{i}" for i in range(1, 6)]):
            out += [(pre + ".conv1.weight", pre + ".bn1", "plain", blk), (pre + ".conv2.weight", pre + ".bn2", "plain", blk),
                    (pre + ".conv3.weight", pre + ".bn3", "res", blk)]
            if pre.endswith("layer1.0"):
                out.append((pre + ".downsample.0.weight", pre + ".downsample.1", "ds", blk))
    elif arch == "irv1_facenet":
        for i in range(5):
            p = f"model.repeat_1.{i}."
            for br in ("branch0", "branch1.0", "branch1.1", "branch2.0", "branch2.1", "branch2.2"):
                out.append((p + br + ".conv.weight", p + br + ".bn", "plain", i))
            out.append((p + "conv2d.weight", None, "res", i))
        for i in range(10):
            p = f"model.repeat_2.{i}."
            for br in ("branch0", "branch1.0", "branch1.1", "branch1.2"):
                out.append((p + br + ".conv.weight", p + br + ".bn", "plain", i))
            out.append((p + "conv2d.weight", None, "res", i))
    else:
        raise ValueError(arch)
    return out


def _coprime_from(a, n):
    while np.gcd(a, n) != 1:
        a += 1
    return a


def selected_position(shape, block):
    """For a conv weight [Cout, Cin, kh, kw]: per output channel n the one selected (tap, cin):
    tap = n mod taps, cin = (a n + block) mod Cin with a >= 33 coprime to Cin, so that successive output channels
    walk through every tap and every 32-channel K-step."""
    cout, cin, kh, kw = shape
    n = np.arange(cout)
    a = _coprime_from(33, cin)
    return n % (kh * kw), (a * n + block) % cin


def selection_state_dict(arch, seed=0):
    """synth_state_dict(arch) with the member convs / BNs of the arch's chain and Bottleneck groups replaced by
    selections: every output channel has exactly one nonzero weight (1, or 2^-2 after folding on the conv that adds
    the residual), the BN scale folds to 1, the BN bias is a multiple of 1/16 in [-1/2, 1/2] (zero on the residual
    convs and the downsample).  Every stored value of those groups is then the correctly rounded sum of at most two
    terms that the storage type holds exactly: no f32 summation order can change it."""
    sd = dict(Wt.synth_state_dict(arch))
    eps = Wt.BN_EPS[arch]
    scale = {"repeat_1": 0.17, "repeat_2": 0.10}
    for key, bn, role, blk in selection_convs(arch):
        shape = sd[key].shape
        cout, cin, kh, kw = shape
        tap, ci = selected_position(shape, blk)
        val = 1.0
        if role == "res":
            val = 0.25 if bn is not None else 0.25 / scale[key.split(".")[1]]
        w = np.zeros((cout, cin, kh * kw), np.float32)
        w[np.arange(cout), ci, tap] = val
        sd[key] = w.reshape(shape)
        if bn is None:
            sd[key[:-len("weight")] + "bias"] = np.zeros(cout, np.float32)
            continue
        sd[bn + ".running_mean"] = np.zeros(cout, np.float32)
        sd[bn + ".running_var"] = np.ones(cout, np.float32)
        sd[bn + ".weight"] = np.full(cout, np.sqrt(1.0 + eps), np.float32)
        if role == "plain":
            u = Wt.splitmix_uniform(seed, "selection:" + bn, cout)
            sd[bn + ".bias"] = (np.floor(u * 17).clip(0, 16) - 8).astype(np.float32) / 16
        else:
            sd[bn + ".bias"] = np.zeros(cout, np.float32)
    return sd
