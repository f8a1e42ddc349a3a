#!/usr/bin/env python3
"""Generate the explanation fixture tests/golden/explain_golden.npz (run where tools/gen_golden.py runs: it needs
the reference checkout; no test and no GPU run needs this tool).

ResNet-50 ArcFace: the reference's OWN ``GradCAM`` (inference/explainability.py:21-131: autograd with hooks on
``model.backbone.layer4``) on its own ``ArcFaceModel`` (models/arcface/arcface_model.py) with the synthetic
weights, over the 8 golden probes, through the shims of tools/gen_golden.py (the cv2 stub gains COLORMAP_JET,
which the reference module evaluates at import).  IResNet100 (autograd at ``layer4``) and IRV1 (a forward hook
on ``model.block8.conv2d``, the reference FaceNet engine's target) come from oracle.models, 2 probes each.

Per entry, ``dev_autocast_*`` is the deviation of the same quantity when the same model runs under CPU
``torch.autocast(bfloat16)``: the yardstick of the end-to-end device tolerances (tests/test_gpu_explain.py).
Maps: max |delta|; pre-ReLU maps ``low``: max |delta| / max |low|.

Output: data only (expected outputs and the targets used).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_golden as GG  # noqa: E402  (the shims, the reference's location)
from facerecognition_amd import weights as W  # noqa: E402
from facerecognition_amd.synthetic import synthetic_crops  # noqa: E402
from oracle import models as OM  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def gradcam_autograd(model, layer, x, target, autocast, call):
    """Grad-CAM of one image by autograd (the steps of GradCAM.generate), optionally under CPU bf16 autocast;
    returns (cam [S, S], low [h, w] = the map before ReLU, raw embedding [D]) as float32 numpy."""
    keep = {}
    hf = layer.register_forward_hook(lambda _m, _i, o: keep.__setitem__("a", o))
    try:
        model.zero_grad()
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            emb = call(model, x)
            score = (F.cosine_similarity(emb, target).sum() if target is not None else (emb ** 2).sum())
        (g,) = torch.autograd.grad(score, keep["a"])
    finally:
        hf.remove()
    a = keep["a"].detach().float()
    wgt = g.float().mean(dim=[2, 3], keepdim=True)
    low = (wgt * a).sum(dim=1, keepdim=True)
    cam = F.interpolate(F.relu(low), size=x.shape[2:], mode="bilinear", align_corners=False).squeeze().numpy()
    if cam.max() > cam.min():
        cam = (cam - cam.min()) / (cam.max() - cam.min())
    return cam.astype(np.float32), low.squeeze().numpy().astype(np.float32), emb.detach().float().numpy()[0]


def activation_map(model, layer, x, autocast):
    """FaceNetExplainabilityEngine.explain's map (explainability.py:482-501): (cam [S, S], low [h, w])."""
    keep = {}
    hf = layer.register_forward_hook(lambda _m, _i, o: keep.__setitem__("a", o.detach()))
    try:
        with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            model(x)
    finally:
        hf.remove()
    low = torch.abs(keep["a"].float()).sum(dim=1, keepdim=True)
    cam = F.interpolate(low, size=x.shape[2:], mode="bilinear", align_corners=False).squeeze().numpy()
    cam = (cam - cam.min()) / (cam.max() - cam.min()) if cam.max() > cam.min() else np.zeros_like(cam)
    return cam.astype(np.float32), low.squeeze().numpy().astype(np.float32)


def rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def main(out=os.path.join(ROOT, "tests", "golden", "explain_golden.npz")):
    REF = GG.REF
    if not os.path.isdir(REF):
        raise SystemExit(f"{REF} not present: goldens are generated where the reference checkout is")
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    GG.install_shims()
    sys.modules["cv2"].COLORMAP_JET = 2
    sys.path.insert(0, REF)
    am = _load("ref_arcface_model", os.path.join(REF, "models/arcface/arcface_model.py"))
    ex = _load("ref_explainability", os.path.join(REF, "inference/explainability.py"))
    res = {}

    # ---- ResNet-50 ArcFace: the reference's GradCAM
    sd = W.synth_state_dict("resnet50_arcface", num_classes=100)
    model = am.ArcFaceModel(num_classes=100, embedding_size=512, pretrained=False)
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    model.eval()
    probes = synthetic_crops(8, 112, seed=0)
    x = OM.preprocess_u8_nhwc(probes)
    with torch.no_grad():
        embn = F.normalize(model(x, labels=None), p=2, dim=1)
    target = torch.roll(embn, -1, 0)  # probe i is explained against probe i + 1's normalised embedding
    gc = ex.GradCAM(model)

    def ref_low():
        return ((gc.gradients.mean(dim=[2, 3], keepdim=True) * gc.activations).sum(dim=1)).squeeze(0).numpy()

    cam_self, low_self, low_tgt, cam_tgt = [], [], [], []
    for i in range(8):
        xi = x[i:i + 1].clone()
        cam_self.append(gc.generate(xi, None).astype(np.float32))
        low_self.append(ref_low().astype(np.float32))
        xi = x[i:i + 1].clone()
        cam_tgt.append(gc.generate(xi, target[i:i + 1]).astype(np.float32))
        low_tgt.append(ref_low().astype(np.float32))
    gc.remove_hooks()
    call = lambda m, xx: m(xx, labels=None)  # noqa: E731
    d_cam, d_low, d_lowt, chk = [], [], [], 0.0
    for i in range(8):
        c32, l32, _ = gradcam_autograd(model, model.backbone.layer4, x[i:i + 1], None, False, call)
        chk = max(chk, float(np.abs(c32 - cam_self[i]).max()), float(np.abs(l32 - low_self[i]).max()))
        cb, lb, _ = gradcam_autograd(model, model.backbone.layer4, x[i:i + 1], None, True, call)
        _, lt, _ = gradcam_autograd(model, model.backbone.layer4, x[i:i + 1], target[i:i + 1], True, call)
        d_cam.append(float(np.abs(cb - cam_self[i]).max()))
        d_low.append(rel(lb, low_self[i]))
        d_lowt.append(rel(lt, low_tgt[i]))
    print(f"r50: own autograd vs the reference's GradCAM (f32) max |d| {chk:.2e}")
    print("r50: target-mode maps that the ReLU zeroes entirely:", [i for i in range(8) if cam_tgt[i].max() == 0])
    res.update(r50_cam_self=np.stack(cam_self[:4]), r50_low_self=np.stack(low_self), r50_low_tgt=np.stack(low_tgt),
               r50_target=target.numpy().astype(np.float32),
               dev_autocast_r50_cam_self=np.float64(max(d_cam[:4])), dev_autocast_r50_low_self=np.float64(max(d_low)),
               dev_autocast_r50_low_tgt=np.float64(max(d_lowt)))

    # ---- IResNet100 (oracle): autograd at layer4
    m = OM.build_model("iresnet100", W.synth_state_dict("iresnet100"))
    x2 = x[:2]
    with torch.no_grad():
        t2 = torch.roll(F.normalize(m(x2), p=2, dim=1), -1, 0)
    call = lambda mm, xx: mm(xx)  # noqa: E731
    cs, ls, lt, dc, dl, dt = [], [], [], [], [], []
    for i in range(2):
        c, l, _ = gradcam_autograd(m, m.layer4, x2[i:i + 1], None, False, call)
        cb, lb, _ = gradcam_autograd(m, m.layer4, x2[i:i + 1], None, True, call)
        _, l_t, _ = gradcam_autograd(m, m.layer4, x2[i:i + 1], t2[i:i + 1], False, call)
        _, l_tb, _ = gradcam_autograd(m, m.layer4, x2[i:i + 1], t2[i:i + 1], True, call)
        cs.append(c), ls.append(l), lt.append(l_t)
        dc.append(float(np.abs(cb - c).max())), dl.append(rel(lb, l)), dt.append(rel(l_tb, l_t))
    res.update(ir100_cam_self=np.stack(cs), ir100_low_self=np.stack(ls), ir100_low_tgt=np.stack(lt),
               ir100_target=t2.numpy().astype(np.float32), dev_autocast_ir100_cam_self=np.float64(max(dc)),
               dev_autocast_ir100_low_self=np.float64(max(dl)), dev_autocast_ir100_low_tgt=np.float64(max(dt)))

    # ---- IRV1 FaceNet (oracle): forward hook on block8.conv2d
    m = OM.build_model("irv1_facenet", W.synth_state_dict("irv1_facenet"))
    x3 = OM.preprocess_u8_nhwc(synthetic_crops(2, 160, seed=0))
    cs, ls, dc, dl = [], [], [], []
    for i in range(2):
        c, l = activation_map(m, m.model.block8.conv2d, x3[i:i + 1], False)
        cb, lb = activation_map(m, m.model.block8.conv2d, x3[i:i + 1], True)
        cs.append(c), ls.append(l)
        dc.append(float(np.abs(cb - c).max())), dl.append(rel(lb, l))
    res.update(irv1_cam=np.stack(cs), irv1_low=np.stack(ls), dev_autocast_irv1_cam=np.float64(max(dc)),
               dev_autocast_irv1_low=np.float64(max(dl)))

    np.savez_compressed(out, probe_seed=np.array(0), **res)
    print(f"wrote {out} ({os.path.getsize(out) / 1024:.0f} KiB)")
    for k, v in res.items():
        if k.startswith("dev_autocast"):
            print(f"  {k} = {float(v):.4g}")


if __name__ == "__main__":
    main()
