"""FR_DTYPE_FP8 (BASELINE config 5: "ArcFace fp8 weights (CDNA4 fp8 MFMA) bs=256, tolerance-checked vs
bf16").

Op level: conv_fp8_kernel (v_mfma_scale_f32_16x16x128_f8f6f4) against a torch fp32 fake-quant
reference of the same op -- e4m3 weights with per-channel scale, activations cast to e4m3 after the
per-tensor power-of-two scaling -- which is exact up to f32 summation order and the bf16 output
rounding.  Model level: IResNet100 with fp8 weights/MFMA vs the bf16 path and the fp32 oracle
(cosine tolerances below, measured and stated), identical top-1 on a planted gallery.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from facerecognition_amd import _native as N

pytestmark = pytest.mark.gpu

COS_VS_BF16 = 1e-3     # cosine(fp8, bf16) >= 0.999 per face
# Regression guard of the all-convs-e4m3 A/B plan (FR_FP8_PLAN=all): 1 - cos = 0.008 .. 0.011 against
# bf16 and the fp32 oracle; a broken fp8 path (wrong scale, lost K-block) lands at 0.1 .. 1.
FP8_GUARD = 2e-2
# the fp8 stage (conv_stage8.hip) vs its fake-quant reference (_fq_layer3), one block at a time from the
# stage's own block input: the only differences are e4m3 rounding flips where the f32 MFMA sum and the
# f64 reference straddle a rounding boundary (~1 element in 2e4 per conv, each 1/16 of its value),
# measured 4.7e-4 rel for one block.
STAGE8_BLOCK_REL = 2e-3
# ... and free-running over all 14 blocks: every flip perturbs the next conv's input, which moves other
# elements across e4m3 boundaries (quantization turns a perturbation d into flips of rms sqrt(d * ulp)),
# so the two fake-quant computations drift apart to ~2e-2 -- the same order as the fp8 noise itself
STAGE8_RUN_REL = 6e-2


def _fp8(t):
    return t.clamp(-448, 448).to(torch.float8_e4m3fn).float()


def _conv_fp8(x, w, *, stride, pad, bias=None, act=0, slope=None, res=None):
    """Run fr_op_conv2d with dtype FP8 (tests/fp8_op.py builds the descriptor). x: cuda bf16 NHWC; w: cpu f32
    [Cout,Cin,kh,kw]."""
    from tests import fp8_op
    dev = x.device
    B, H, W, Cx = x.shape
    cout, cin, kh, kw = w.shape
    K = kh * kw * cin
    w8, sc, codes = fp8_op.quantize_weights(w)
    s, q = sc[:cout], codes.reshape(cout, K)
    Ho = (H + 2 * pad[0] - kh) // stride[0] + 1
    Wo = (W + 2 * pad[1] - kw) // stride[1] + 1
    y = torch.zeros((B, Ho, Wo, cout), dtype=torch.bfloat16, device=dev)
    xa = x.float().abs().max().reshape(1).to(dev)
    ya = torch.zeros(1, device=dev)

    def dev32(t):
        return None if t is None else t.to(dev).float().contiguous()

    rc = fp8_op.launch(x, w8.to(dev), sc.to(dev), xa, y, Cin=cin, Cout=cout, kh=kh, kw=kw, stride=stride, pad=pad,
                       bias=dev32(bias), act=act, slope=dev32(slope), res=res, y_amax=ya)
    N.check(rc, "fr_op_conv2d fp8")
    torch.cuda.synchronize()
    # fake-quant reference: activations / 2^e -> e4m3 -> * 2^e ; weights q * s
    e = math.ceil(math.log2(xa.item() / 448.0)) if xa.item() > 0 else 0
    xq = _fp8(x.float().cpu() / 2.0 ** e) * 2.0 ** e
    wq = (q * s[:, None]).reshape(cout, kh, kw, cin).permute(0, 3, 1, 2)
    ref = F.conv2d(xq.permute(0, 3, 1, 2).double(), wq.double(), stride=stride, padding=pad)
    if bias is not None:
        ref = ref + bias.double()[None, :, None, None]
    ref = ref.permute(0, 2, 3, 1)
    if res is not None:
        ref = ref + res.float().cpu().double()
    if act == 1:
        ref = ref.clamp_min(0)
    elif act == 2:
        ref = torch.where(ref > 0, ref, ref * slope.double())
    return y.float().cpu(), ref.float(), ya.item()


FP8_CASES = [
    # B, H, W, Cin, Cout, kh, kw, stride, pad
    (2, 14, 14, 256, 256, 3, 3, (1, 1), (1, 1)),   # layer3 conv
    (2, 28, 28, 128, 128, 3, 3, (1, 1), (1, 1)),   # layer2 conv
    (2, 56, 56, 64, 64, 3, 3, (1, 1), (1, 1)),     # layer1 (K = 576: last K-step half padding)
    (2, 28, 28, 128, 256, 3, 3, (2, 2), (1, 1)),   # stride-2 block conv
    (3, 7, 7, 512, 512, 3, 3, (1, 1), (1, 1)),     # layer4
    (2, 16, 16, 64, 128, 1, 1, (2, 2), (0, 0)),    # 1x1 stride-2 downsample (K = 64 < 128)
]


@pytest.mark.parametrize("case", FP8_CASES)
def test_conv_fp8_vs_fake_quant(gpu, case):
    B, H, W, Cin, Cout, kh, kw, stride, pad = case
    g = torch.Generator().manual_seed(hash(case) & 0xFFFF)
    x = (torch.randn(B, H, W, Cin, generator=g) * 3).to(torch.bfloat16).to(gpu)
    w = torch.randn(Cout, Cin, kh, kw, generator=g) / np.sqrt(Cin * kh * kw)
    bias = torch.randn(Cout, generator=g) * 0.1
    slope = torch.rand(Cout, generator=g) * 0.3
    y, ref, ya = _conv_fp8(x, w, stride=stride, pad=pad, bias=bias, act=2, slope=slope)
    scale = ref.abs().max().item()
    err = (y - ref).abs()
    assert (err <= 1e-2 * (ref.abs() + scale / 8)).all(), f"max err {err.max().item():.4g} (scale {scale:.4g})"
    assert abs(ya - y.abs().max().item()) <= 1e-2 * ya  # epilogue amax = max |stored y| (before bf16 rounding)


def test_conv_fp8_large_activations_no_nan(gpu):
    """Activations far above the e4m3 range (448) are scaled by 2^e, never NaN."""
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(2, 14, 14, 256, generator=g) * 3000).to(torch.bfloat16).to(gpu)
    w = torch.randn(256, 256, 3, 3, generator=g) / 48
    y, ref, _ = _conv_fp8(x, w, stride=(1, 1), pad=(1, 1), res=None)
    assert torch.isfinite(y).all()
    assert ((y - ref).abs() <= 1e-2 * (ref.abs() + ref.abs().max() / 8)).all()


def _fp8_vs_bf16(u8):
    from facerecognition_amd.model import FRModel
    from facerecognition_amd.weights import synth_state_dict
    sd = synth_state_dict("iresnet100")
    m8 = FRModel("iresnet100", sd, dtype="fp8")
    mb = FRModel("iresnet100", sd, dtype="bf16")
    e8 = m8.embed(torch.from_numpy(u8)).cpu().numpy()
    eb = mb.embed(torch.from_numpy(u8)).cpu().numpy()
    m8.close()
    mb.close()
    return sd, e8, eb


def _fq_layer3(q, x, first, last):
    """Fake-quant reference of IResNet100 layer3 blocks first..last as the fp8 stage computes them: each
    conv's input in e4m3 with a per-image power-of-two scale (the smallest 2^e with amax / 2^e <= 448),
    e4m3 weights x the per-channel scale (the blob's .w / .wscale), f64 sums, the border-class bias of the
    folded bn1, PReLU; the residual stream rounded to bf16 per block (the next conv1 quantizes that
    bf16 value).  x: [B, 14, 14, 256] float (the stage input)."""
    r = torch.tensor([0] + [1] * 12 + [2])
    cls = (3 * r[:, None] + r[None, :]).reshape(-1)  # [196] border class 3 rc + cc

    def qa(v):
        amax = v.abs().reshape(v.shape[0], -1).amax(dim=1)
        e = torch.where(amax > 0, torch.ceil(torch.log2(amax / 448.0)), torch.zeros_like(amax))
        sc = torch.pow(2.0, e).view(-1, 1, 1, 1)
        return (v / sc).float().clamp(-448, 448).to(torch.float8_e4m3fn).double() * sc

    def conv(v, name):
        w = torch.from_numpy(q[name + ".w"]).double() * torch.from_numpy(q[name + ".wscale"]).double()[:, None, None, None]
        y = F.conv2d(qa(v).permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), padding=1)
        return y.permute(0, 2, 3, 1)

    res = x.double()          # the bf16 residual stream (also what the next conv1 quantizes)
    outs = {}
    for i in range(first, last + 1):
        p = f"layer3.{i}"
        b9 = torch.from_numpy(q[p + ".conv1.b9"]).double()[cls].view(1, 14, 14, -1)
        t = conv(res, p + ".conv1") + b9
        sl = torch.from_numpy(q[p + ".conv1.slope"]).double()
        t = torch.where(t > 0, t, t * sl)
        v = conv(t, p + ".conv2") + torch.from_numpy(q[p + ".conv2.b"]).double() + res
        res = v.to(torch.bfloat16).double()
        outs[p] = res.float()
    return outs


@pytest.mark.parametrize("B", [1, 3])
def test_fp8_stage_vs_fake_quant(gpu, B):
    """The e4m3 layer3 stage (blocks 16..29 of the mixed plan, one workgroup per image) against its
    fake-quant reference from the same stage input (the bf16 stage's layer3.15 output)."""
    from facerecognition_amd import weights as Wt
    from facerecognition_amd.model import FRModel
    from facerecognition_amd.synthetic import synthetic_crops
    from test_gpu_stage import _named
    sd = Wt.synth_state_dict("iresnet100")
    q = Wt.quantize_fp8(Wt.fold_state_dict("iresnet100", sd), convs=Wt.fp8_plan("iresnet100"))
    m = FRModel("iresnet100", sd, dtype="fp8")
    m.set_option(N.FR_OPT_KEEP_INTERMEDIATES, 1)
    m.set_option(N.FR_OPT_STAGE, 2)
    import ctypes
    buf = ctypes.create_string_buffer(1 << 16)
    N.check(N.lib().fr_debug_plan(m.handle, B, buf, len(buf)))
    assert "stage8 " in buf.value.decode(), buf.value.decode()
    m.embed(torch.from_numpy(synthetic_crops(B, 112, seed=13)))
    t = _named(m, B, {f"layer3.{i}" for i in range(15, 30)})
    m.close()
    worst = 0.0
    for i in range(16, 30):  # each block from the stage's own input of that block
        n = f"layer3.{i}"
        ref = _fq_layer3(q, t[f"layer3.{i - 1}"], i, i)[n]
        rel = ((t[n] - ref).norm() / ref.norm()).item()
        worst = max(worst, rel)
        assert rel < STAGE8_BLOCK_REL, f"{n}: fp8 stage vs fake-quant rel err {rel:.3e}"
    run = _fq_layer3(q, t["layer3.15"], 16, 29)["layer3.29"]
    rel_run = ((t["layer3.29"] - run).norm() / run.norm()).item()
    print(f"\nfp8 stage vs fake-quant: worst block rel err {worst:.3e}, free-running 14 blocks {rel_run:.3e}")
    assert rel_run < STAGE8_RUN_REL


def test_iresnet100_fp8_meets_config5_bar(gpu):
    from facerecognition_amd.synthetic import synthetic_crops
    _, e8, eb = _fp8_vs_bf16(synthetic_crops(6, 112, seed=4))
    c_b = np.sum(e8 * eb, axis=1)
    print(f"\nfp8 vs bf16 1-cos: {1 - c_b}")
    assert np.all(1 - c_b <= COS_VS_BF16), f"fp8 vs bf16: 1-cos = {1 - c_b}"


def test_iresnet100_fp8_guard_and_top1(gpu):
    """Regression guard (FP8_GUARD, see above) against bf16 and the fp32 oracle, and identical top-1 on a
    planted gallery."""
    from facerecognition_amd.synthetic import synthetic_crops
    from oracle import models as M
    u8 = synthetic_crops(6, 112, seed=4)
    sd, e8, eb = _fp8_vs_bf16(u8)
    ref = M.embed(M.build_model("iresnet100", sd), "iresnet100", u8)
    c_b = np.sum(e8 * eb, axis=1)
    c_o = np.sum(e8 * ref, axis=1) / np.linalg.norm(ref, axis=1)
    print(f"\nfp8 vs bf16 1-cos: {1 - c_b}\nfp8 vs oracle 1-cos: {1 - c_o}")
    assert np.all(np.isfinite(e8))
    assert np.all(1 - c_b <= FP8_GUARD), f"fp8 vs bf16: 1-cos = {1 - c_b}"
    assert np.all(1 - c_o <= FP8_GUARD), f"fp8 vs oracle: 1-cos = {1 - c_o}"
    # identical top-1 on a planted gallery (rows = normalize(ref + 0.05 noise) + distractors)
    rng = np.random.default_rng(11)
    G = rng.standard_normal((1000, 512)).astype(np.float32)
    G[:6] = ref + 0.05 * rng.standard_normal(ref.shape).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    from facerecognition_amd.gallery import DeviceGallery
    gal = DeviceGallery(G)
    _, i8 = gal.search(e8, 1)
    _, ib = gal.search(eb, 1)
    assert np.array_equal(i8[:, 0], np.arange(6)) and np.array_equal(ib[:, 0], np.arange(6))
    gal.close()


def test_iresnet100_fp8_bs256(gpu):
    """BASELINE config-5 size (IResNet100 fp8, bs = 256, the autotuner's bs=256 tiles): deterministic replay,
    finite unit-norm rows, every face's 1-cos against bf16 at the same batch within the config-5 bar (1e-3;
    median / p99 / max printed), an oracle sample, and identical top-1 on a planted 10k gallery."""
    from facerecognition_amd.gallery import DeviceGallery
    from facerecognition_amd.model import FRModel
    from facerecognition_amd.synthetic import synthetic_crops
    from facerecognition_amd.weights import synth_state_dict
    from oracle import models as M
    sd = synth_state_dict("iresnet100")
    u8 = synthetic_crops(256, 112, seed=41)
    m8 = FRModel("iresnet100", sd, dtype="fp8")
    a = m8.embed(torch.from_numpy(u8)).cpu()
    b = m8.embed(torch.from_numpy(u8)).cpu()
    assert torch.equal(a, b), "fp8 forward is not deterministic at bs=256"
    assert torch.isfinite(a).all() and torch.allclose(a.norm(dim=1), torch.ones(256), atol=1e-5)
    m8.close()
    mb = FRModel("iresnet100", sd, dtype="bf16")
    eb = mb.embed(torch.from_numpy(u8)).cpu().numpy()
    mb.close()
    d = 1 - np.sum(a.numpy() * eb, axis=1)
    print(f"\nfp8 vs bf16 at bs=256: 1-cos median {np.median(d):.4g}, p99 {np.quantile(d, 0.99):.4g}, max {d.max():.4g}, "
          f"share <= 1e-3: {np.mean(d <= COS_VS_BF16):.3f}")
    assert d.max() <= COS_VS_BF16, f"config-5 bar: {int((d > COS_VS_BF16).sum())} faces above 1e-3, max {d.max():.4g}"
    ref = M.embed(M.build_model("iresnet100", sd), "iresnet100", u8[:3])
    c_o = (a[:3].numpy() * ref).sum(1) / np.linalg.norm(ref, axis=1)
    assert float((1 - c_o).max()) <= FP8_GUARD, 1 - c_o
    rng = np.random.default_rng(42)
    G = rng.standard_normal((10000, 512)).astype(np.float32)
    perm = rng.permutation(10000)[:256]
    G[perm] = a.numpy() + 0.03 * rng.standard_normal((256, 512)).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    gal = DeviceGallery(G)
    _, idx = gal.search(a.numpy(), 5)
    assert np.array_equal(idx[:, 0], perm)
    gal.close()
    # non-planted: a 10k gallery of bf16 embeddings of OTHER faces; does the fp8 query pick the same
    # nearest identity as the bf16 query of the same face?
    mb = FRModel("iresnet100", sd, dtype="bf16")
    G = np.concatenate([mb.embed(torch.from_numpy(synthetic_crops(2000, 112, seed=100 + k))).cpu().numpy()
                        for k in range(5)])
    mb.close()
    gal = DeviceGallery(G)
    s8, i8 = gal.search(a.numpy(), 5)
    sb, ib = gal.search(eb, 5)
    gal.close()
    agree = float(np.mean(i8[:, 0] == ib[:, 0]))
    top5 = float(np.mean([len(set(x) & set(y)) / 5 for x, y in zip(i8, ib)]))
    margin = sb[:, 0] - sb[:, 1]
    flips = i8[:, 0] != ib[:, 0]
    print(f"non-planted 10k gallery: top-1 agreement {agree:.4f}, top-5 overlap {top5:.4f}, "
          f"bf16 top1-top2 margin median {np.median(margin):.4g}, flipped-query margins {margin[flips]}")
    # a top-1 may only differ where bf16's own top-1 / top-2 margin is within the fp8 drift: the scores of the two
    # gallery rows g1 (bf16's top-1) and g2 (fp8's) move by at most ||a8 - ab|| * ||g1 - g2|| between the queries
    drift = np.linalg.norm(a.numpy() - eb, axis=1)
    g12 = np.linalg.norm(G[ib[:, 0]] - G[i8[:, 0]], axis=1)
    swing = drift * g12
    assert np.all(sb[flips, 0] - (G[i8[flips, 0]] * eb[flips]).sum(1) <= swing[flips] + 1e-5), (margin[flips], swing[flips])
    # (r05: with every gallery row a real embedding -- before, 2000-face batches read past 2 GiB and a third of
    # the rows were garbage -- the agreement is 0.94 at a 1e-3 drift on a 10k synthetic-face gallery)
    assert agree >= 0.9


def test_iresnet100_fp8_all_plan_guard(gpu, monkeypatch):
    """FR_FP8_PLAN=all (every eligible conv in e4m3; the A/B plan): the e4m3 layer3 stage's output feeds
    the per-conv e4m3 layer4.0 convs, whose activation scale needs that tensor's amax -- the stages have
    no amax epilogue, so the engine runs one reduction pass after the stage.  Bounded by
    FP8_GUARD against bf16 and the fp32 oracle; without the amax pass layer4 ran unscaled."""
    import ctypes
    from facerecognition_amd.model import FRModel
    from facerecognition_amd.synthetic import synthetic_crops
    from facerecognition_amd.weights import synth_state_dict
    from oracle import models as M
    monkeypatch.setenv("FR_FP8_PLAN", "all")
    sd = synth_state_dict("iresnet100")
    u8 = synthetic_crops(4, 112, seed=44)
    m8 = FRModel("iresnet100", sd, dtype="fp8")
    buf = ctypes.create_string_buffer(1 << 16)
    N.check(N.lib().fr_debug_plan(m8.handle, 4, buf, len(buf)))
    e8 = m8.embed(torch.from_numpy(u8)).cpu().numpy()
    m8.close()
    monkeypatch.delenv("FR_FP8_PLAN")
    mb = FRModel("iresnet100", sd, dtype="bf16")
    eb = mb.embed(torch.from_numpy(u8)).cpu().numpy()
    mb.close()
    ref = M.embed(M.build_model("iresnet100", sd), "iresnet100", u8)
    c_b = np.sum(e8 * eb, axis=1)
    c_o = np.sum(e8 * ref, axis=1) / np.linalg.norm(ref, axis=1)
    print(f"\nFR_FP8_PLAN=all: 1-cos vs bf16 {1 - c_b}, vs oracle {1 - c_o}")
    assert np.all(np.isfinite(e8))
    assert np.all(1 - c_b <= FP8_GUARD) and np.all(1 - c_o <= FP8_GUARD)
