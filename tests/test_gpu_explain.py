"""Explanations on the device (csrc/explain.hip, fr_explain): the op-level kernels against float64 on identical
inputs, fr_explain against the closed form on its own inputs, the end-to-end maps against the reference-pinned
fixture, batch independence and the Python surface.

Error bounds (u = 2^-24, the f32 unit roundoff; every device sum is f32, any order):
  head gradient  |V - V64| <= N u sum_n |g_n w_nk|                                 (the standard summation bound)
  channel weight wgt = mean_p grad: the bound of its inputs averaged, plus (P + 1) u mean_p |grad|
  low            delta_p = sum_c err(wgt_c) |A_pc| + (C + 1) u sum_c mean_p|grad_c| |A_pc|
  cam            4 max_p delta_p / (max - min) + 1e-6: ReLU and the bilinear weights (a convex combination) do
                 not amplify, (c - min) / (max - min) carries the errors of c, min (numerator) and max, min
                 (denominator); 1e-6 covers the f32 interpolation weights and the final division.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from facerecognition_amd import _native as N
from facerecognition_amd import explainability as X
from facerecognition_amd.synthetic import synthetic_crops
from facerecognition_amd.weights import fold_state_dict, synth_state_dict

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "explain_golden.npz")
MODES = {"pooled": 0, "flat": 1, "activation": 2}


# ----------------------------------------------------------------------------- op wrappers
def head_grad(g, w16, K, dtype, v):
    B, n = g.shape
    N.check(N.lib().fr_op_head_grad(g.data_ptr(), B, n, w16.data_ptr(), K, w16.shape[1], N.FR_DTYPE[dtype],
                                    v.data_ptr(), N.stream_ptr()), "fr_op_head_grad")
    torch.cuda.synchronize()
    return v


def cam_op(act16, v, mode, S, dtype):
    B, h, w, C = act16.shape
    cam = torch.full((B, S, S), -7.0, dtype=torch.float32, device="cuda")
    low = torch.full((B, h, w), -7.0, dtype=torch.float32, device="cuda")
    N.check(N.lib().fr_op_cam(act16.data_ptr(), B, h, w, C, N.FR_DTYPE[dtype], N.ptr(v), MODES[mode], S,
                              cam.data_ptr(), low.data_ptr(), N.stream_ptr()), "fr_op_cam")
    torch.cuda.synchronize()
    return cam.cpu().numpy().astype(np.float64), low.cpu().numpy().astype(np.float64)


def low_bound(A, V, errV, mode):
    """delta [B, h, w] of the module docstring; A f64 [B,h,w,C], V / errV f64 [B,K] (None: activation)."""
    B, h, w, C = A.shape
    P = h * w
    if mode == "activation":
        return C * U * np.abs(A).sum(-1)
    if mode == "pooled":
        gabs, gerr = np.abs(V) / P, errV / P + U * np.abs(V) / P
        gabs, gerr = gabs[:, None, None, :], gerr[:, None, None, :]
        wabs, werr = gabs, gerr
    else:
        gabs, gerr = np.abs(V).reshape(B, h, w, C), errV.reshape(B, h, w, C)
        wabs = gabs.mean(axis=(1, 2), keepdims=True)
        werr = gerr.mean(axis=(1, 2), keepdims=True) + (P + 1) * U * wabs
    return (werr * np.abs(A)).sum(-1) + (C + 1) * U * (wabs * np.abs(A)).sum(-1)


def check_maps(cam, low, A, V, errV, mode, S, what=""):
    """The device maps against float64 on the same inputs, within the bounds of the module docstring."""
    ref_cam, ref_low = X.cam_from_gradient(A, V, mode, S)
    delta = low_bound(A, V, errV, mode)
    e_low = np.abs(low - ref_low)
    worst = float((e_low / np.maximum(delta, 1e-300)).max())
    print(f"  {what} low: max err {e_low.max():.3e}, worst err / bound {worst:.3f}")
    assert (e_low <= delta).all(), (what, "low", float(e_low.max()))
    for b in range(A.shape[0]):
        up = X.upsample_bilinear(ref_low[b] if mode == "activation" else np.maximum(ref_low[b], 0), S)
        rng = up.max() - up.min()
        if rng > 0:
            bound = 4 * delta[b].max() / rng + 1e-6
        else:  # a constant map is stored as it is
            bound = delta[b].max() + 1e-6 * max(1.0, abs(up.max()))
        err = float(np.abs(cam[b] - ref_cam[b]).max())
        print(f"  {what} cam[{b}]: max err {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (what, "cam", b, err, bound)


# ----------------------------------------------------------------------------- 1. head gradient
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", [(1, 512, 2048, 2048), (3, 512, 25088, 25088), (9, 24, 200, 256),
                                   (17, 512, 1792, 1792)])
def test_head_grad_vs_float64(gpu, shape, dtype):
    B, n, K, Kpad = shape
    gen = torch.Generator().manual_seed(B * 1000 + K)
    w16 = (torch.randn((n, Kpad), generator=gen) * 0.05).to(TDT[dtype]).cuda()  # the padding holds values too
    g = torch.randn((B, n), generator=gen).cuda()
    v = torch.full((B, Kpad), 12345.0, dtype=torch.float32, device="cuda")
    head_grad(g, w16, K, dtype, v)
    g64, w64 = g.cpu().double().numpy(), w16.cpu().double().numpy()[:, :K]
    got = v.cpu().double().numpy()
    err = np.abs(got[:, :K] - g64 @ w64)
    bound = n * U * (np.abs(g64) @ np.abs(w64))
    print(f"\n  head_grad {shape} {dtype}: max err {err.max():.3e}, worst err / bound {(err / bound).max():.4f}")
    assert (err <= bound).all()
    assert (got[:, K:] == 12345.0).all(), "padding columns were written"
    # the sum over n has a fixed order per output: an image's row is the same bits alone and in the batch
    last = torch.full((1, Kpad), 12345.0, dtype=torch.float32, device="cuda")
    head_grad(g[B - 1:].contiguous(), w16, K, dtype, last)
    assert torch.equal(last[0], v[B - 1])


def test_head_grad_refuses_bad_shapes(gpu):
    L = N.lib()
    t = torch.zeros(4096, dtype=torch.float32, device="cuda")
    p = t.data_ptr()
    for (B, n, K, Kpad) in ((1, 2048, 64, 64), (1, 8, 60, 64), (1, 8, 64, 60), (1, 8, 128, 64), (0, 8, 64, 64)):
        assert L.fr_op_head_grad(p, B, n, p, K, Kpad, 0, p, None) == -1
    assert L.fr_op_head_grad(None, 1, 8, p, 64, 64, 0, p, None) == -1
    assert L.fr_op_cam(p, 1, 17, 17, 8, 0, p, 0, 8, p, None, None) == -1  # 289 positions
    assert L.fr_op_cam(p, 1, 2, 2, 12, 0, p, 0, 8, p, None, None) == -1   # C % 8
    assert L.fr_op_cam(p, 1, 2, 2, 8, 0, None, 1, 8, p, None, None) == -1  # a gradient layout without v
    assert L.fr_op_cam(p, 1, 2, 2, 8, 0, p, 0, 8, None, None, None) == -1  # cam NULL


# ----------------------------------------------------------------------------- 2. map kernel
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("case", [(4, 4, 2048, 112, "pooled"), (7, 7, 512, 112, "flat"),
                                  (3, 3, 1792, 160, "activation"), (2, 3, 72, 10, "flat")])
def test_cam_vs_float64(gpu, case, B, dtype):
    h, w, C, S, mode = case
    gen = torch.Generator().manual_seed(h * 100 + C + B)
    act = torch.randn((B, h, w, C), generator=gen).to(TDT[dtype]).cuda()
    v = None
    if mode != "activation":
        v = torch.randn((B, C if mode == "pooled" else h * w * C), generator=gen).cuda()
    cam, low = cam_op(act, v, mode, S, dtype)
    A = act.cpu().double().numpy()
    V = None if v is None else v.cpu().double().numpy()
    print()
    check_maps(cam, low, A, V, None if V is None else np.zeros_like(V), mode, S, f"{case} B={B} {dtype}")
    assert cam.min() >= 0.0 and cam.max() <= 1.0


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_cam_crafted_images(gpu, dtype):
    """Small integers: every sum is exact in f32, so the device must equal float64 to the final rounding."""
    h, w, C, S = 3, 4, 16, 20
    P = h * w
    base = torch.arange(1, C + 1, dtype=torch.float32).repeat(h * w, 1).reshape(1, h, w, C)
    pos = torch.arange(P, dtype=torch.float32).reshape(1, h, w, 1)
    # image 0: every low negative; 1: the same positive low at every position; 2: one positive position
    a_neg, a_const = base + pos, base.clone()
    a_one = -base.clone()
    a_one[0, 1, 2, :] = base[0, 0, 0, :]
    act = torch.cat([a_neg, a_const, a_one]).to(TDT[dtype]).cuda()
    v = torch.full((3, C), float(P), dtype=torch.float32, device="cuda")  # wgt = v / P = 1
    v[0] = -float(P)
    cam, low = cam_op(act, v, "pooled", S, dtype)
    ref_cam, ref_low = X.cam_from_gradient(act.cpu().double().numpy(), v.cpu().double().numpy(), "pooled", S)
    assert np.array_equal(low, ref_low)
    assert (low[0] < 0).all() and (cam[0] == 0).all()
    L = float(C * (C + 1) // 2)
    assert (low[1] == L).all() and (cam[1] == L).all(), "a constant map must be stored unnormalised"
    assert (low[2] > 0).sum() == 1 and low[2, 1, 2] == L
    assert np.abs(cam[2] - ref_cam[2]).max() <= 1e-6 and cam[2].max() == 1.0 and cam[2].min() == 0.0
    # the peak lies where position (1, 2) maps to, not at its transpose
    py, px = np.unravel_index(cam[2].argmax(), cam[2].shape)
    assert abs((py + 0.5) * h / S - 1.5) <= 0.5 and abs((px + 0.5) * w / S - 2.5) <= 0.5
    # the activation map of a constant tensor is zeros
    cam_a, low_a = cam_op(a_const.to(TDT[dtype]).cuda(), None, "activation", S, dtype)
    assert (low_a == L).all() and (cam_a == 0).all()


# ----------------------------------------------------------------------------- models
_MODELS = {}


def model(arch):
    from facerecognition_amd.model import FRModel
    if arch not in _MODELS:
        sd = synth_state_dict(arch, num_classes=100) if arch == "resnet50_arcface" else synth_state_dict(arch)
        _MODELS[arch] = (FRModel(arch, sd, max_batch=8), sd)
    return _MODELS[arch]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for m, _ in _MODELS.values():
        m.close()
    _MODELS.clear()


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def named_tensor(m, name, B):
    L = N.lib()
    for t in range(L.fr_debug_tensor_count(m.handle)):
        if L.fr_debug_tensor_name(m.handle, t).decode() == name:
            H, W, C = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            N.check(L.fr_debug_tensor_shape(m.handle, t, ctypes.byref(H), ctypes.byref(W), ctypes.byref(C)))
            dt = torch.float16 if L.fr_debug_tensor_dtype(m.handle, t) == N.FR_DTYPE_F16 else torch.bfloat16
            buf = torch.empty((B, H.value, W.value, C.value), dtype=dt, device="cuda")
            N.check(L.fr_debug_copy_tensor(m.handle, t, B, buf.data_ptr(), N.stream_ptr()))
            torch.cuda.synchronize()
            return buf.cpu().double().numpy()
    raise KeyError(name)


TARGET_LAYER = {"resnet50_arcface": "backbone.layer4.2", "iresnet100": "layer4.2"}


def probes(arch, n):
    return synthetic_crops(8, 112, seed=0)[:n] if arch != "irv1_facenet" else synthetic_crops(2, 160, seed=0)[:n]


# ----------------------------------------------------------------------------- 3. fr_explain on its own inputs
@pytest.mark.parametrize("with_target", [False, True])
@pytest.mark.parametrize("arch", ["resnet50_arcface", "iresnet100"])
def test_explain_against_its_own_inputs(gpu, arch, with_target):
    """The explained tensor and the raw embeddings of the same forward, head.w rounded as uploaded: the maps
    must be the closed form's within the bounds of tests 1-2 (g = d score / d emb is evaluated in f32: 2 e is
    exact; the cosine gradient's two terms carry the rounding of three f32 dot products over D and a few
    operations, taken as (D + 16) u of each term's magnitude)."""
    m, sd = model(arch)
    B, mode = 3, X.EXPLAIN_MODE[arch]
    gen = torch.Generator().manual_seed(5)
    target = torch.nn.functional.normalize(torch.randn((B, 512), generator=gen), dim=1) if with_target else None
    cam, emb, low = m.explain(torch.from_numpy(probes(arch, B)), target=target, return_low=True)
    torch.cuda.synchronize()
    assert m.explain_shape() == {"resnet50_arcface": (4, 4, 2048), "iresnet100": (7, 7, 512)}[arch]
    A = named_tensor(m, TARGET_LAYER[arch], B)
    hw = torch.from_numpy(fold_state_dict(arch, sd)["head.w"]).to(torch.bfloat16).double().numpy()
    e = emb.cpu().double().numpy()
    t = None if target is None else target.double().numpy()
    g = X.score_gradient(e, t)
    D = e.shape[1]
    if t is None:
        gerr = np.zeros_like(g)
    else:
        ne, nt = np.linalg.norm(e, axis=1, keepdims=True), np.linalg.norm(t, axis=1, keepdims=True)
        gerr = (D + 16) * U * (np.abs(t) / (ne * nt) + np.abs(e) * (np.abs(e) * np.abs(t)).sum(1, keepdims=True) /
                               (ne ** 3 * nt))
    V = g @ hw
    errV = D * U * (np.abs(g) @ np.abs(hw)) + gerr @ np.abs(hw)
    print()
    check_maps(cam.cpu().double().numpy(), low.cpu().double().numpy(), A, V, errV, mode, 112,
               f"{arch} target={with_target}")


# ----------------------------------------------------------------------------- 4. end to end vs the fixture
def test_end_to_end_r50_vs_reference_gradcam(gpu, gold):
    """The reference's own GradCAM (f32 autograd) on the 8 golden probes.  Bound: twice the deviation of the
    same quantity under CPU bf16 autocast (the fixture's dev_autocast: the same order of perturbation as the
    device's bf16 forward, other rounding points).  Target mode compares the map before ReLU: the ReLU zeroes
    some target-mode maps entirely in the f32 reference too, and maps near that boundary are ill-conditioned."""
    m, _ = model("resnet50_arcface")
    u8 = torch.from_numpy(probes("resnet50_arcface", 8))
    cam, _, low = m.explain(u8, return_low=True)
    d_cam = float(np.abs(cam.cpu().numpy()[:4] - gold["r50_cam_self"]).max())
    d_low = float(np.abs(low.cpu().numpy() - gold["r50_low_self"]).max() / np.abs(gold["r50_low_self"]).max())
    _, _, low_t = m.explain(u8, target=torch.from_numpy(gold["r50_target"]), return_low=True)
    d_lowt = float(np.abs(low_t.cpu().numpy() - gold["r50_low_tgt"]).max() / np.abs(gold["r50_low_tgt"]).max())
    print(f"\n  r50 device vs reference: cam self {d_cam:.4f} (yardstick {float(gold['dev_autocast_r50_cam_self']):.4f}), "
          f"low self {d_low:.4f} ({float(gold['dev_autocast_r50_low_self']):.4f}), "
          f"low target {d_lowt:.4f} ({float(gold['dev_autocast_r50_low_tgt']):.4f})")
    assert d_cam <= 2 * float(gold["dev_autocast_r50_cam_self"])
    assert d_lowt <= 2 * float(gold["dev_autocast_r50_low_tgt"])
    assert d_low <= 2 * float(gold["dev_autocast_r50_low_self"])


def test_end_to_end_iresnet100_vs_oracle_autograd(gpu, gold):
    m, _ = model("iresnet100")
    u8 = torch.from_numpy(probes("iresnet100", 2))
    cam, _, low = m.explain(u8, return_low=True)
    d_cam = float(np.abs(cam.cpu().numpy() - gold["ir100_cam_self"]).max())
    d_low = float(np.abs(low.cpu().numpy() - gold["ir100_low_self"]).max() / np.abs(gold["ir100_low_self"]).max())
    _, _, low_t = m.explain(u8, target=torch.from_numpy(gold["ir100_target"]), return_low=True)
    d_lowt = float(np.abs(low_t.cpu().numpy() - gold["ir100_low_tgt"]).max() / np.abs(gold["ir100_low_tgt"]).max())
    print(f"\n  iresnet100 device vs oracle: cam self {d_cam:.4f} (yardstick "
          f"{float(gold['dev_autocast_ir100_cam_self']):.4f}), low self {d_low:.4f} "
          f"({float(gold['dev_autocast_ir100_low_self']):.4f}), low target {d_lowt:.4f} "
          f"({float(gold['dev_autocast_ir100_low_tgt']):.4f})")
    assert d_cam <= 2 * float(gold["dev_autocast_ir100_cam_self"])
    assert d_lowt <= 2 * float(gold["dev_autocast_ir100_low_tgt"])
    assert d_low <= 2 * float(gold["dev_autocast_ir100_low_self"])


def test_end_to_end_irv1_vs_oracle_activation_map(gpu, gold):
    m, _ = model("irv1_facenet")
    assert m.explain_shape() == (3, 3, 1792)
    cam, _, low = m.explain(torch.from_numpy(probes("irv1_facenet", 2)), return_low=True)
    d_cam = float(np.abs(cam.cpu().numpy() - gold["irv1_cam"]).max())
    d_low = float(np.abs(low.cpu().numpy() - gold["irv1_low"]).max() / np.abs(gold["irv1_low"]).max())
    print(f"\n  irv1 device vs oracle: cam {d_cam:.4f} (yardstick {float(gold['dev_autocast_irv1_cam']):.4f}), "
          f"low {d_low:.4f} ({float(gold['dev_autocast_irv1_low']):.4f})")
    assert d_cam <= 2 * float(gold["dev_autocast_irv1_cam"])
    assert d_low <= 2 * float(gold["dev_autocast_irv1_low"])


# ----------------------------------------------------------------------------- 5. batch independence
def test_batch_independence_and_explain_batch(gpu):
    m, _ = model("resnet50_arcface")
    m.set_option(N.FR_OPT_BATCH_INVARIANT, 1)
    try:
        u8 = probes("resnet50_arcface", 3)
        gen = torch.Generator().manual_seed(9)
        t = torch.nn.functional.normalize(torch.randn((3, 512), generator=gen), dim=1)
        for tgt in (None, t):
            cam3, emb3, low3 = m.explain(torch.from_numpy(u8), target=tgt, return_low=True)
            for i in (0, 2):
                cam1, emb1, low1 = m.explain(torch.from_numpy(u8[i:i + 1]), target=None if tgt is None else tgt[i:i + 1],
                                             return_low=True)
                assert torch.equal(emb1[0], emb3[i]) and torch.equal(low1[0], low3[i]) and torch.equal(cam1[0], cam3[i])
        eng = X.ExplainabilityEngine(m, face_detector=None)
        eng.face_detector = None  # (no detector weights in the test tree: the plain-resize fallback)
        batch = eng.explain_batch([u8[0], u8[1], u8[2]], target_embeddings=t)
        for i in range(3):
            one = eng.explain(u8[i], target_embedding=t[i])
            for k in ("cam", "heatmap", "overlay", "original"):
                assert np.array_equal(one[k], batch[i][k]), (i, k)
    finally:
        m.set_option(N.FR_OPT_BATCH_INVARIANT, 0)


# ----------------------------------------------------------------------------- 6. Python surface, argument checks
def test_python_surface(gpu):
    from PIL import Image
    m, _ = model("resnet50_arcface")
    eng = X.ExplainabilityEngine(m, face_detector=None)
    eng.face_detector = None
    img = Image.fromarray(synthetic_crops(1, 200, seed=3)[0])  # not the input size: the resize fallback
    r = eng.explain(img)
    assert set(r) == {"cam", "heatmap", "overlay", "original"}
    assert r["cam"].shape == (112, 112) and r["cam"].dtype == np.float32
    assert 0.0 <= r["cam"].min() and r["cam"].max() <= 1.0
    for k in ("heatmap", "overlay", "original"):
        assert r[k].shape == (112, 112, 3) and r[k].dtype == np.uint8
    assert eng.explain("/nonexistent/file.jpg") == {"error": "Cannot read image"}
    mf, _ = model("irv1_facenet")
    fe = X.FaceNetExplainabilityEngine(mf, face_detector=None)
    fe.face_detector = None
    a = fe.explain(img)
    b = fe.explain(img, target_embedding=torch.ones(512))
    assert a["cam"].shape == (160, 160) and a["original"].shape == (160, 160, 3)
    assert 0.0 <= a["cam"].min() and a["cam"].max() <= 1.0
    assert np.array_equal(a["cam"], b["cam"]), "IRV1 must ignore the target embedding"


def test_explain_argument_checks(gpu):
    from facerecognition_amd.model import FRModel
    L = N.lib()
    m, _ = model("resnet50_arcface")
    u8 = torch.from_numpy(probes("resnet50_arcface", 2)).cuda()
    cam = torch.empty((2, 112, 112), dtype=torch.float32, device="cuda")
    s = N.stream_ptr()
    assert L.fr_explain(m.handle, u8.data_ptr(), 0, 2, 112, 112, None, None, None, None, s) == -1  # cam NULL
    assert b"cam" in L.fr_last_error()
    big = 64  # above the batch reserved for this handle (8)
    assert L.fr_explain(m.handle, u8.data_ptr(), 0, big, 112, 112, None, cam.data_ptr(), None, None, s) == -1
    assert b"reserved" in L.fr_last_error()
    empty = FRModel("resnet50_arcface")  # no weights
    try:
        assert L.fr_explain(empty.handle, u8.data_ptr(), 0, 2, 112, 112, None, cam.data_ptr(), None, None, s) == -4
        h = ctypes.c_int()
        assert L.fr_explain_shape(empty.handle, ctypes.byref(h), ctypes.byref(h), ctypes.byref(h)) == -4
    finally:
        empty.close()
    torch.cuda.synchronize()
