"""Explanations, host side (CPU only): the float64 closed form against the reference-pinned fixture, the
colour map, the blend and the header.

tests/golden/explain_golden.npz was produced by tools/gen_golden_explain.py: the reference's own GradCAM
(inference/explainability.py, autograd with hooks on backbone.layer4) on its ArcFaceModel with the synthetic
weights for ResNet-50, and autograd / a forward hook on oracle.models for IResNet100 / IRV1.  Here
``cam_closed_form`` -- no backward pass: head.w^T g on the oracle's f32 activations -- must reproduce every map.
"""
import os

import numpy as np
import pytest
import torch

from facerecognition_amd import _native as N
from facerecognition_amd import explainability as X
from facerecognition_amd.synthetic import synthetic_crops
from facerecognition_amd.weights import fold_state_dict, synth_state_dict
from oracle import models as OM

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "explain_golden.npz")
TOL = 1e-5  # f32 autograd summation order against float64 (measured <= 1.4e-6)


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def oracle_run(arch, layer_name, u8):
    """(activation of `layer_name` NHWC f32, raw embeddings, folded head.w) of the CPU oracle."""
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    sd = synth_state_dict(arch, num_classes=100) if arch == "resnet50_arcface" else synth_state_dict(arch)
    m = OM.build_model(arch, sd)
    keep = {}
    h = m.get_submodule(layer_name).register_forward_hook(lambda _m, _i, o: keep.__setitem__("a", o.detach()))
    with torch.no_grad():
        x = OM.preprocess_u8_nhwc(u8)
        emb = m(x) if arch == "irv1_facenet" else m(x, labels=None)
    h.remove()
    return keep["a"].permute(0, 2, 3, 1).numpy(), emb.numpy(), fold_state_dict(arch, sd)["head.w"]


def close(got, want, what):
    """max |delta| <= TOL on the normalised maps; the maps before ReLU are not normalised, so theirs is taken
    relative to the map's largest magnitude."""
    scale = 1.0 if what.startswith("cam") else float(np.abs(want).max())
    err = float(np.abs(got - want).max()) / scale
    print(f"  {what}: max |d| / scale = {err:.2e} (scale {scale:.3g})")
    assert err <= TOL, (what, err)


def test_closed_form_reproduces_reference_gradcam_r50(gold):
    act, emb, hw = oracle_run("resnet50_arcface", "backbone.layer4", synthetic_crops(8, 112, seed=0))
    assert act.shape == (8, 4, 4, 2048) and hw.shape == (512, 2048)
    cam, low = X.cam_closed_form(act, hw, emb, None, "pooled", 112)
    close(cam[:4], gold["r50_cam_self"], "cam self")
    close(low, gold["r50_low_self"], "low self")
    _, low_t = X.cam_closed_form(act, hw, emb, gold["r50_target"], "pooled", 112)
    close(low_t, gold["r50_low_tgt"], "low target")


def test_closed_form_reproduces_autograd_iresnet100(gold):
    act, emb, hw = oracle_run("iresnet100", "layer4", synthetic_crops(8, 112, seed=0)[:2])  # the first two golden probes
    assert act.shape == (2, 7, 7, 512) and hw.shape == (512, 25088)
    cam, low = X.cam_closed_form(act, hw, emb, None, "flat", 112)
    close(cam, gold["ir100_cam_self"], "cam self")
    close(low, gold["ir100_low_self"], "low self")
    _, low_t = X.cam_closed_form(act, hw, emb, gold["ir100_target"], "flat", 112)
    close(low_t, gold["ir100_low_tgt"], "low target")


def test_closed_form_reproduces_activation_map_irv1(gold):
    act, _, _ = oracle_run("irv1_facenet", "model.block8.conv2d", synthetic_crops(2, 160, seed=0))
    assert act.shape == (2, 3, 3, 1792)
    cam, low = X.cam_closed_form(act, None, None, None, "activation", 160)
    close(cam, gold["irv1_cam"], "cam")
    close(low, gold["irv1_low"], "low")


def test_closed_form_degenerate_maps():
    a = np.ones((1, 2, 2, 8))
    hw = np.ones((4, 8))
    e = np.ones((1, 4))
    cam, low = X.cam_closed_form(-a, hw, e, None, "pooled", 6)   # every position negative: ReLU leaves zeros
    assert (low < 0).all() and (cam == 0).all()
    cam, low = X.cam_closed_form(a, hw, e, None, "pooled", 6)    # constant positive: stored unnormalised
    assert np.allclose(cam, low[0, 0, 0]) and low[0, 0, 0] > 1
    cam, _ = X.cam_closed_form(a, None, None, None, "activation", 6)  # constant activation map: zeros
    assert (cam == 0).all()


def test_upsample_matches_torch_rule():
    rng = np.random.default_rng(0)
    for h, w, S in ((4, 4, 112), (2, 3, 10), (7, 7, 112), (3, 3, 160)):
        low = rng.standard_normal((h, w))
        want = torch.nn.functional.interpolate(torch.from_numpy(low)[None, None], size=(S, S), mode="bilinear",
                                               align_corners=False)[0, 0].numpy()
        assert np.abs(X.upsample_bilinear(low, S) - want).max() < 1e-12


def test_jet_anchors_and_shape():
    cam = np.linspace(0, 1, 12 * 7).reshape(12, 7)
    hm = X.generate_heatmap(cam)
    assert hm.dtype == np.uint8 and hm.shape == (12, 7, 3)
    lut = X.generate_heatmap(np.arange(256).reshape(1, 256) / 255.0 + 1e-9)[0]
    assert tuple(lut[0]) == (128, 0, 0) and tuple(lut[255]) == (0, 0, 128)   # BGR
    # the interior is the piecewise-linear definition (parity with cv2 unpinned): blue peaks before green before red
    assert lut[:, 0].argmax() < lut[:, 1].argmax() < lut[:, 2].argmax()


def test_overlay_alpha_endpoints():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    hm = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    assert np.array_equal(X.overlay_heatmap(img, hm, alpha=0.0), img)
    assert np.array_equal(X.overlay_heatmap(img, hm, alpha=1.0), hm)
    mid = X.overlay_heatmap(img, hm, alpha=0.5)
    assert mid.dtype == np.uint8 and np.abs(mid.astype(int) - (img.astype(int) + hm) / 2).max() <= 0.5
    assert X.overlay_heatmap(img, hm[:4, :5], alpha=0.5).shape == img.shape  # the heat map is resized


def test_header_lists_explain_functions():
    fns = N.header_functions()
    for f in ("fr_explain_shape", "fr_explain", "fr_op_head_grad", "fr_op_cam"):
        assert f in fns and f in N._SIGS


def test_lazy_reexport():
    import facerecognition_amd as P
    assert P.ExplainabilityEngine is X.ExplainabilityEngine and P.cam_closed_form is X.cam_closed_form
