"""Explanations on the device: the reference's inference/explainability.py on ``FRModel.explain``.

The reference runs ``GradCAM.generate`` (forward + autograd backward with hooks on ``backbone.layer4``) per
image for ArcFace, and an activation map of ``block8.conv2d`` for FaceNet.  Here no torch module exists to
hook and none is needed: in eval mode everything after the explained tensor is affine and already folded into
``head.w`` (weights.fold_state_dict), so the gradient of the score with respect to the head input is
``head.w^T g`` with ``g = d score / d embedding`` in closed form.  libfrhip's ``fr_explain`` runs the forward,
that transposed product and the map kernel for a whole batch (csrc/explain.hip).

The public surface keeps the reference's names: ``ExplainabilityEngine``, ``FaceNetExplainabilityEngine``
(``explain`` -> dict with 'cam' / 'heatmap' / 'overlay' / 'original'), ``generate_heatmap``, ``overlay_heatmap``,
``explain_prediction``; ``explain_batch`` is new (one forward for all images).  cv2 is not a dependency: images
are numpy / PIL, RGB throughout.  The colour map, the heat-map resize and the blend restate OpenCV's
definitions; their parity with cv2 is unpinned, like the crop fallback's resize.

``cam_closed_form`` is the float64 numpy statement of the same map, from the definition; the tests and the
golden fixture check the device against it.
"""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

COLORMAP_JET = 2  # cv2.COLORMAP_JET's value; the only colour map here


# ----------------------------------------------------------------------------- the closed form (float64)
def _bilinear_axis(n_in: int, n_out: int):
    """torch F.interpolate(mode='bilinear', align_corners=False) along one axis: lower / upper source index and
    the upper weight per destination index.  src = max(0, (dst + 0.5) * in / out - 0.5), upper clamped to in - 1."""
    src = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, src - i0


def upsample_bilinear(low: np.ndarray, S: int) -> np.ndarray:
    """[..., h, w] -> [..., S, S] (float64), torch's align_corners=False rule."""
    low = np.asarray(low, dtype=np.float64)
    y0, y1, ly = _bilinear_axis(low.shape[-2], S)
    x0, x1, lx = _bilinear_axis(low.shape[-1], S)
    r0, r1 = low[..., y0, :], low[..., y1, :]
    top = r0[..., :, x0] + (r0[..., :, x1] - r0[..., :, x0]) * lx  # a + l (b - a): a constant map stays constant
    bot = r1[..., :, x0] + (r1[..., :, x1] - r1[..., :, x0]) * lx
    return top + (bot - top) * ly[:, None]


def score_gradient(emb: np.ndarray, target: Optional[np.ndarray]) -> np.ndarray:
    """d score / d emb [B, D] (float64): score = (emb ** 2).sum() (target None) or
    F.cosine_similarity(emb, target) with both norms clamped at 1e-8."""
    e = np.asarray(emb, dtype=np.float64)
    if target is None:
        return 2.0 * e
    t = np.broadcast_to(np.asarray(target, dtype=np.float64).reshape(-1, e.shape[-1]), e.shape)
    ne = np.maximum(np.linalg.norm(e, axis=-1, keepdims=True), 1e-8)
    nt = np.maximum(np.linalg.norm(t, axis=-1, keepdims=True), 1e-8)
    et = (e * t).sum(-1, keepdims=True)
    return t / (ne * nt) - et * e / (ne ** 3 * nt)


def cam_closed_form(act_nhwc, head_w, emb, target, mode: str, S: int) -> Tuple[np.ndarray, np.ndarray]:
    """The class-activation map in float64 numpy, from its definition.

    act_nhwc [B, h, w, C]: the explained tensor; head_w [D, K]: the folded head matrix (K = C for mode
    'pooled', where the head reads the average over positions; K = h*w*C in NHWC order for mode 'flat');
    emb [B, D]: the raw embeddings; target: None or [B, D] / [D]; mode 'activation' ignores head_w / emb /
    target and sums |act| over channels (no ReLU, zeros for a constant map).  Returns (cam [B, S, S], low
    [B, h, w] = the map before ReLU)."""
    if mode == "activation":
        return cam_from_gradient(act_nhwc, None, mode, S)
    B = np.asarray(act_nhwc).shape[0]
    V = score_gradient(np.asarray(emb).reshape(B, -1), target) @ np.asarray(head_w, dtype=np.float64)  # [B, K]
    return cam_from_gradient(act_nhwc, V, mode, S)


def cam_from_gradient(act_nhwc, V, mode: str, S: int) -> Tuple[np.ndarray, np.ndarray]:
    """cam_closed_form from the gradient V [B, K] of the score with respect to the head input."""
    A = np.asarray(act_nhwc, dtype=np.float64)
    B, h, w, C = A.shape
    if mode == "activation":
        low = np.abs(A).sum(-1)
        cam = upsample_bilinear(low, S)
    else:
        V = np.asarray(V, dtype=np.float64).reshape(B, -1)
        if mode == "pooled":
            grad = np.broadcast_to((V / (h * w))[:, None, None, :], A.shape)
        elif mode == "flat":
            grad = V.reshape(B, h, w, C)
        else:
            raise ValueError(f"mode must be 'pooled', 'flat' or 'activation', got {mode!r}")
        wgt = grad.mean(axis=(1, 2))                      # [B, C]
        low = (A * wgt[:, None, None, :]).sum(-1)         # [B, h, w]
        cam = upsample_bilinear(np.maximum(low, 0.0), S)
    out = np.empty_like(cam)
    for b in range(B):
        mn, mx = cam[b].min(), cam[b].max()
        if mx > mn:
            out[b] = (cam[b] - mn) / (mx - mn)
        else:
            out[b] = 0.0 if mode == "activation" else cam[b]
    return out, low


EXPLAIN_MODE = {"resnet50_arcface": "pooled", "iresnet100": "flat", "irv1_facenet": "activation"}


# ----------------------------------------------------------------------------- colour map, blend
def _jet_lut() -> np.ndarray:
    """OpenCV's COLORMAP_JET as a [256, 3] BGR u8 table, from its piecewise-linear definition: 64 control
    values per channel (red: 0 up to index 23, a ramp of 1/16 steps to 1 at 39, 1 to 55, down to 0.5 at 63;
    green: the same ramp 16 indices earlier and back down to 0 at 55; blue: red mirrored), interpolated
    linearly to 256 levels and scaled by 255 with round-half-to-even."""
    i = np.arange(64, dtype=np.float64)
    r = np.clip(np.minimum((i - 23) / 16, (71 - i) / 16), 0, 1)
    g = np.clip(np.minimum((i - 7) / 16, (55 - i) / 16), 0, 1)
    b = r[::-1]
    x, xs = np.linspace(0, 1, 256), np.linspace(0, 1, 64)
    lut = np.stack([np.interp(x, xs, c) for c in (b, g, r)], axis=1) * 255.0
    return np.rint(lut).astype(np.uint8)


_JET = _jet_lut()


def generate_heatmap(cam: np.ndarray, colormap: int = COLORMAP_JET) -> np.ndarray:
    """[H, W] in [0, 1] -> coloured heat map u8 [H, W, 3] BGR (np.uint8(255 * cam) through the JET table)."""
    if colormap != COLORMAP_JET:
        raise ValueError("only COLORMAP_JET is available")
    idx = np.uint8(255 * np.clip(np.asarray(cam, dtype=np.float64), 0.0, 1.0))
    return _JET[idx]


def _resize_u8(img: np.ndarray, width: int, height: int) -> np.ndarray:
    from PIL import Image
    if img.shape[1] == width and img.shape[0] == height:
        return img
    return np.asarray(Image.fromarray(img).resize((width, height), Image.BILINEAR))


def overlay_heatmap(image: np.ndarray, heatmap: np.ndarray, alpha: float = 0.5) -> np.ndarray:
    """image * (1 - alpha) + heatmap * alpha, rounded and saturated to u8 (cv2.addWeighted's definition); the
    heat map is resized to the image when their sizes differ."""
    image = np.asarray(image)
    if heatmap.shape[:2] != image.shape[:2]:
        heatmap = _resize_u8(np.asarray(heatmap), image.shape[1], image.shape[0])
    mix = image.astype(np.float64) * (1 - alpha) + heatmap.astype(np.float64) * alpha
    return np.clip(np.rint(mix), 0, 255).astype(np.uint8)


def _load_rgb(image_input) -> Optional[np.ndarray]:
    from PIL import Image
    try:
        if isinstance(image_input, str):
            return np.asarray(Image.open(image_input).convert("RGB"), dtype=np.uint8)
        if isinstance(image_input, Image.Image):
            return np.asarray(image_input.convert("RGB"), dtype=np.uint8)
        return np.ascontiguousarray(np.asarray(image_input, dtype=np.uint8))  # numpy RGB
    except Exception:
        return None


def _result(cam: np.ndarray, face_rgb: np.ndarray) -> dict:
    heat_rgb = np.ascontiguousarray(generate_heatmap(cam)[..., ::-1])
    heat_rgb = _resize_u8(heat_rgb, face_rgb.shape[1], face_rgb.shape[0])
    return {"cam": cam, "heatmap": heat_rgb, "overlay": overlay_heatmap(face_rgb, heat_rgb, alpha=0.5),
            "original": face_rgb}


# ----------------------------------------------------------------------------- engines
class ExplainabilityEngine:
    """Grad-CAM explanations for the ArcFace backbones (reference ExplainabilityEngine, explainability.py:235-392).

    model: an ``FRModel`` (resnet50_arcface: Grad-CAM on backbone.layer4, as the reference; iresnet100: on
    layer4.2, the input of the head).  transform is accepted for the reference's call shape and unused: the
    aligned u8 crop goes to the device as it is, ToTensor + Normalize are fused into the first kernel."""

    SIZE = 112
    MARGIN = 0.2
    ALIGN = True

    def __init__(self, model, transform=None, device: str = "cuda", face_detector=None,
                 mtcnn_weights: Optional[str] = None):
        self.model = model
        self.transform = transform
        self.device = device
        self.face_detector = face_detector
        if self.face_detector is None:
            try:
                from .face_detector import FaceDetector
                self.face_detector = FaceDetector(backend="mtcnn", device=device, confidence_threshold=0.9,
                                                  select_largest=True, weights_dir=mtcnn_weights)
                print("[Explainability] Face detector initialized")
            except Exception as e:  # reference :257-258
                print(f"[Explainability] Cannot init face detector: {e}")

    def _align_face(self, rgb: np.ndarray, landmarks: dict) -> Optional[np.ndarray]:
        import torch
        from .align import align_faces
        try:
            x = torch.as_tensor(np.ascontiguousarray(rgb))[None].to(self.model.device)
            crops, ok = align_faces(x, [landmarks], self.SIZE)
            return crops[0].cpu().numpy() if ok[0] else None
        except Exception as e:
            print(f"[Explainability] Alignment error: {e}")
            return None

    def _face(self, rgb: np.ndarray) -> np.ndarray:
        """Detect + align; else the margin crop; else the plain resize (reference :317-333)."""
        face = None
        if self.face_detector is not None:
            if self.ALIGN:
                det = self.face_detector.detect_rgb(rgb)
                if det and det.get("landmarks"):
                    face = self._align_face(rgb, det["landmarks"])
            if face is None:
                bgr = np.ascontiguousarray(rgb[..., ::-1])
                crop = self.face_detector.crop_face(bgr, margin=self.MARGIN, target_size=(self.SIZE, self.SIZE))
                if crop is not None and crop.size:
                    face = np.ascontiguousarray(crop[..., ::-1])
        if face is None:
            face = _resize_u8(rgb, self.SIZE, self.SIZE)
        return np.ascontiguousarray(face, dtype=np.uint8)

    def _targets(self, targets, n: int):
        if targets is None:
            return None
        import torch
        t = targets if torch.is_tensor(targets) else torch.as_tensor(np.asarray(targets, dtype=np.float32))
        t = t.float().reshape(-1, self.model.embedding_size)
        if t.shape[0] not in (1, n):
            raise ValueError(f"target embeddings must be [D] or [{n}, D], got {tuple(t.shape)}")
        return t

    def explain_batch(self, image_inputs: Sequence, target_embeddings=None) -> List[dict]:
        """explain() for a list of images with ONE forward (the reference runs forward + backward per image)."""
        rgbs = [_load_rgb(i) for i in image_inputs]
        good = [k for k, r in enumerate(rgbs) if r is not None]
        out: List[dict] = [{"error": "Cannot read image"} for _ in rgbs]
        if not good:
            return out
        faces = np.stack([self._face(rgbs[k]) for k in good])
        t = self._targets(target_embeddings, len(rgbs))
        if t is not None and t.shape[0] == len(rgbs):
            t = t[good]
        cams, _ = self.model.explain(faces, target=t)
        cams = cams.cpu().numpy()
        for j, k in enumerate(good):
            out[k] = _result(cams[j], faces[j])
        return out

    def explain(self, image_input, target_embedding=None) -> dict:
        """{'cam' [S, S] f32, 'heatmap' / 'overlay' / 'original' u8 [S, S, 3] RGB} or {'error': ...}."""
        return self.explain_batch([image_input], target_embedding)[0]

    def save_explanation(self, result: dict, output_path: str, mode: str = "overlay") -> None:
        from PIL import Image
        os.makedirs(os.path.dirname(output_path) if os.path.dirname(output_path) else ".", exist_ok=True)
        if mode == "heatmap":
            img = result["heatmap"]
        elif mode == "combined":
            img = np.concatenate([result["original"], result["heatmap"], result["overlay"]], axis=1)
        else:
            img = result["overlay"]
        Image.fromarray(np.ascontiguousarray(img)).save(output_path)
        print(f"Saved: {output_path}")


class FaceNetExplainabilityEngine(ExplainabilityEngine):
    """The FaceNet engine (explainability.py:395-515): the margin crop at 160 x 160 (no landmark alignment) and
    the activation map |block8.conv2d| summed over channels; target embeddings are ignored."""

    SIZE = 160
    MARGIN = 0.05
    ALIGN = False

    def _targets(self, targets, n: int):
        return None


def explain_prediction(model, image_path: str, transform=None, device: str = "cuda", target_embedding=None,
                       output_path: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(original, heat map, overlay), RGB u8 at the image's own size, for one image file resized to the model's
    input (reference explain_prediction, explainability.py:176-232: no detection)."""
    from PIL import Image
    original = _load_rgb(image_path)
    if original is None:
        raise ValueError(f"Cannot read image: {image_path}")
    S = model.input_size
    cam, _ = model.explain(_resize_u8(original, S, S)[None], target=target_embedding)
    heat = np.ascontiguousarray(generate_heatmap(cam[0].cpu().numpy())[..., ::-1])
    heat = _resize_u8(heat, original.shape[1], original.shape[0])
    overlay = overlay_heatmap(original, heat, alpha=0.5)
    if output_path:
        os.makedirs(os.path.dirname(output_path) if os.path.dirname(output_path) else ".", exist_ok=True)
        Image.fromarray(np.concatenate([original, heat, overlay], axis=1)).save(output_path)
        print(f"Saved explanation: {output_path}")
    return original, heat, overlay
