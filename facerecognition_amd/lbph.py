"""LBPH recognition on the device: the ``cv2.face.LBPHFaceRecognizer`` surface the reference uses
(models/lbphmodel/*) over the ``fr_lbph_*`` ops of libfrhip.so.

``LBPHFaceRecognizer`` restates OpenCV's published algorithm (extended LBP, spatial histograms,
HISTCMP_CHISQR_ALT nearest neighbour; DESIGN.md §4 LBPH).  ``cv2`` is not installed where this was written, so
the yardstick is a float32 / float64 numpy restatement of that algorithm (tests/lbph_ref.py); nobody has
compared it with a real ``cv2.face`` build.  Histograms live on the device as u16 counts (a ``torch.int16``
buffer read as u16); OpenCV's float32 histogram is ``count / P`` and is derived on request.  ``predict_batch``
runs one ``fr_lbph_hist`` and one ``fr_lbph_match`` for all probes, where OpenCV scans every training
histogram once per query.  There is no CPU path.

Below the class: restatements of the reference's train_lbph.py, inference_lbph.py, threshold_lbph.py and
train_lbph_script.py.  Model files are ``.npz`` (parameters, u16 counts, labels); OpenCV's XML / YAML model
files are neither read nor written.
"""
from __future__ import annotations

import os
import sys
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import _native as N

DBL_MAX = sys.float_info.max
_MAX_BATCH = 32768  # fr_lbph_match takes up to 65535 probes a call
IMAGE_EXTENSIONS = {'.jpg', '.jpeg', '.png', '.bmp', '.tiff', '.tif'}


def lbph_table(radius: int = 1, neighbors: int = 8):
    """fr_lbph_table: (offs int32 [n][4] = fx, fy, cx, cy; w float32 [n][4] = w1..w4).  Host only."""
    offs = np.zeros((max(neighbors, 1), 4), np.int32)
    w = np.zeros((max(neighbors, 1), 4), np.float32)
    N.check(N.lib().fr_lbph_table(radius, neighbors, offs.ctypes.data, w.ctypes.data), "fr_lbph_table")
    return offs, w


def lbph_hist(images, radius: int = 1, neighbors: int = 8, grid_x: int = 8, grid_y: int = 8):
    """fr_lbph_hist: cuda u8 [B, H, W] -> cuda int16 [B, D] holding the u16 cell counts."""
    import torch
    x = images.contiguous()
    if x.dtype != torch.uint8 or x.dim() != 3 or not x.is_cuda:
        raise ValueError("lbph_hist: images must be a cuda uint8 tensor [B, H, W]")
    B, H, W = x.shape
    D = grid_x * grid_y * (1 << neighbors) if 0 <= neighbors <= 8 and grid_x > 0 and grid_y > 0 else 1
    out = torch.empty((B, D), dtype=torch.int16, device=x.device)
    N.check(N.lib().fr_lbph_hist(N.ptr(x), B, H, W, radius, neighbors, grid_x, grid_y, N.ptr(out),
                                 N.stream_ptr(x.device)), "fr_lbph_hist")
    return out


def lbph_match(probes, gallery, cell_pixels: int, k: int = 1):
    """fr_lbph_match: count rows (cuda int16 [B, D] and [N, D]) -> (dist cuda f64 [B, k], idx cuda i32 [B, k]),
    ascending, equal distances by ascending row, +inf / -1 past N."""
    import torch
    q, g = probes.contiguous(), gallery.contiguous()
    if q.dtype != torch.int16 or g.dtype != torch.int16 or q.dim() != 2 or g.dim() != 2 or q.shape[1] != g.shape[1]:
        raise ValueError("lbph_match: probes and gallery must be int16 [B, D] and [N, D] count rows")
    B, D = q.shape
    n = g.shape[0]
    L = N.lib()
    nws = int(L.fr_lbph_match_workspace(B, n, D, k))
    if nws == 0:
        N.check(-1, "fr_lbph_match_workspace")
    ws = torch.empty((nws,), dtype=torch.uint8, device=q.device)
    dist = torch.empty((B, k), dtype=torch.float64, device=q.device)
    idx = torch.empty((B, k), dtype=torch.int32, device=q.device)
    N.check(L.fr_lbph_match(N.ptr(q), B, N.ptr(g), n, D, cell_pixels, k, N.ptr(dist), N.ptr(idx), N.ptr(ws), nws,
                            N.stream_ptr(q.device)), "fr_lbph_match")
    return dist, idx


class LBPHFaceRecognizer:
    """``cv2.face.LBPHFaceRecognizer`` as the reference uses it, on the device (see the module docstring: checked
    against a numpy restatement of OpenCV's algorithm, not against cv2 itself)."""

    def __init__(self, radius: int = 1, neighbors: int = 8, grid_x: int = 8, grid_y: int = 8,
                 threshold: float = DBL_MAX, device="cuda"):
        if not (1 <= radius <= 4 and 1 <= neighbors <= 8 and 1 <= grid_x <= 16 and 1 <= grid_y <= 16):
            raise ValueError("LBPH: radius 1..4, neighbors 1..8, grid_x and grid_y 1..16")
        self._radius, self._neighbors, self._grid_x, self._grid_y = int(radius), int(neighbors), int(grid_x), int(grid_y)
        self._threshold = float(threshold)
        self._device = device
        self._size: Optional[Tuple[int, int]] = None  # (H, W) of the training images
        self._counts = None                            # cuda int16 [N, D] (u16 counts)
        self._labels = np.zeros((0,), np.int32)

    # ---- parameters (cv2 names)
    def getRadius(self): return self._radius
    def getNeighbors(self): return self._neighbors
    def getGridX(self): return self._grid_x
    def getGridY(self): return self._grid_y
    def getThreshold(self): return self._threshold
    def setThreshold(self, val): self._threshold = float(val)
    def getLabels(self): return self._labels.copy()

    @property
    def cell_pixels(self) -> int:
        H, W = self._size
        return ((W - 2 * self._radius) // self._grid_x) * ((H - 2 * self._radius) // self._grid_y)

    def getHistograms(self) -> np.ndarray:
        """float32 [N, D]: count / (float)P, OpenCV's stored histograms."""
        if self._counts is None:
            return np.zeros((0, self._grid_x * self._grid_y * (1 << self._neighbors)), np.float32)
        c = self._counts.cpu().numpy().view(np.uint16)
        return c.astype(np.float32) / np.float32(self.cell_pixels)

    # ---- training
    def _stack(self, faces) -> np.ndarray:
        faces = [np.asarray(f) for f in faces]
        if not faces:
            raise ValueError("LBPH: empty training data")
        for f in faces:
            if f.ndim != 2 or f.dtype != np.uint8:
                raise ValueError("LBPH: images must be 2-D uint8 (gray)")
            if f.shape != faces[0].shape:
                raise ValueError(f"LBPH: all images of one model must have the same size "
                                 f"({f.shape} vs {faces[0].shape})")
        return np.ascontiguousarray(np.stack(faces))

    def _hist(self, stack: np.ndarray):
        import torch
        outs = []
        for s in range(0, len(stack), _MAX_BATCH):
            x = torch.from_numpy(stack[s:s + _MAX_BATCH]).to(self._device)
            outs.append(lbph_hist(x, self._radius, self._neighbors, self._grid_x, self._grid_y))
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    def _train(self, faces, labels, keep: bool):
        import torch
        stack = self._stack(faces)
        labels = np.asarray(labels).astype(np.int32).reshape(-1)
        if len(labels) != len(stack):
            raise ValueError(f"LBPH: {len(stack)} images but {len(labels)} labels")
        if keep and self._counts is not None and tuple(stack.shape[1:]) != self._size:
            raise ValueError(f"LBPH: update images are {stack.shape[1:]}, the model was trained on {self._size}")
        counts = self._hist(stack)
        if keep and self._counts is not None:
            self._counts = torch.cat([self._counts, counts])
            self._labels = np.concatenate([self._labels, labels])
        else:
            self._size = (int(stack.shape[1]), int(stack.shape[2]))
            self._counts, self._labels = counts, labels

    def train(self, faces, labels):
        self._train(faces, labels, keep=False)

    def update(self, faces, labels):
        """Appends to the training set (cv2's update)."""
        self._train(faces, labels, keep=True)

    # ---- prediction
    def predict_batch(self, imgs):
        """(labels int32 [B], confidences float64 [B]): the nearest training histogram of every probe, one
        fr_lbph_hist and one fr_lbph_match.  A probe whose smallest distance is not < threshold gives
        (-1, DBL_MAX), as cv2's predict."""
        if self._counts is None or len(self._labels) == 0:
            raise RuntimeError("LBPH: this model is not trained")
        stack = self._stack(imgs)
        if tuple(stack.shape[1:]) != self._size:
            raise ValueError(f"LBPH: probe images are {tuple(stack.shape[1:])}, the model was trained on {self._size}")
        q = self._hist(stack)
        dist = np.empty((len(stack),), np.float64)
        idx = np.empty((len(stack),), np.int64)
        for s in range(0, len(stack), _MAX_BATCH):
            d, i = lbph_match(q[s:s + _MAX_BATCH], self._counts, self.cell_pixels, 1)
            dist[s:s + _MAX_BATCH] = d[:, 0].cpu().numpy()
            idx[s:s + _MAX_BATCH] = i[:, 0].cpu().numpy()
        ok = dist < self._threshold
        labels = np.where(ok, self._labels[idx], -1).astype(np.int32)
        return labels, np.where(ok, dist, DBL_MAX)

    def predict(self, img):
        labels, conf = self.predict_batch([img])
        return int(labels[0]), float(conf[0])

    # ---- persistence
    def save(self, path: str):
        """.npz: the parameters, the image size, the u16 counts and the labels."""
        if self._counts is None:
            raise RuntimeError("LBPH: this model is not trained")
        with open(path, "wb") as f:
            np.savez(f, radius=self._radius, neighbors=self._neighbors, grid_x=self._grid_x, grid_y=self._grid_y,
                     threshold=self._threshold, size=np.asarray(self._size, np.int32),
                     counts=self._counts.cpu().numpy().view(np.uint16), labels=self._labels)

    @classmethod
    def load(cls, path: str, device="cuda") -> "LBPHFaceRecognizer":
        import torch
        with np.load(path) as z:
            m = cls(int(z["radius"]), int(z["neighbors"]), int(z["grid_x"]), int(z["grid_y"]), float(z["threshold"]),
                    device=device)
            counts, labels, size = z["counts"], z["labels"], z["size"]
        D = m._grid_x * m._grid_y * (1 << m._neighbors)
        if counts.dtype != np.uint16 or counts.ndim != 2 or counts.shape[1] != D or len(labels) != len(counts):
            raise ValueError(f"LBPH: {path} does not hold [N, {D}] uint16 counts with N labels")
        m._size = (int(size[0]), int(size[1]))
        m._counts = torch.from_numpy(np.ascontiguousarray(counts).view(np.int16)).to(device)
        m._labels = labels.astype(np.int32)
        return m


def LBPHFaceRecognizer_create(radius: int = 1, neighbors: int = 8, grid_x: int = 8, grid_y: int = 8,
                              threshold: float = DBL_MAX) -> LBPHFaceRecognizer:
    return LBPHFaceRecognizer(radius, neighbors, grid_x, grid_y, threshold)


# ------------------------------------------------------------------------ the reference's functions, restated
def train_lbph_model(faces, labels, radius=1, neighbors=8, grid_x=8, grid_y=8) -> LBPHFaceRecognizer:
    """train_lbph.py:4-36."""
    model = LBPHFaceRecognizer_create(radius=radius, neighbors=neighbors, grid_x=grid_x, grid_y=grid_y)
    if not isinstance(labels, np.ndarray):
        labels = np.array(labels, dtype=np.int32)
    model.train(faces, labels)
    return model


def recognize_face(model, face_img, threshold) -> Dict:
    """inference_lbph.py:4-18: known when conf < threshold."""
    pred, conf = model.predict(face_img)
    if conf < threshold:
        return {"label": pred, "confidence": conf, "status": "known"}
    return {"label": None, "confidence": conf, "status": "unknown"}


def find_optimal_threshold(model, faces, labels, min_coverage=0.3, threshold_range=None):
    """threshold_lbph.py:7-96 with ONE batched predict in place of a predict per validation image, then the
    reference's accuracy x coverage sweep; returns (best_threshold, best_score, [(thr, acc, coverage, score)])
    and falls back to (max(threshold_range), 0.0) when no threshold reaches min_coverage."""
    if threshold_range is None:
        threshold_range = range(40, 121, 5)
    labels = np.asarray(labels)
    print(f"[THRESHOLD] Predicting {len(faces)} validation samples...")
    if len(faces):
        predictions, confidences = model.predict_batch(faces)
    else:
        predictions, confidences = np.zeros((0,), np.int32), np.zeros((0,), np.float64)
    print(f"[THRESHOLD] Đang đánh giá {len(threshold_range)} thresholds...")
    best_threshold, best_score, threshold_results = None, -1, []
    for threshold in threshold_range:
        accepted_mask = confidences < threshold
        used = np.sum(accepted_mask)
        if used > 0:
            accuracy = np.sum(predictions[accepted_mask] == labels[accepted_mask]) / used
        else:
            accuracy = 0.0
        coverage = used / len(labels) if len(labels) > 0 else 0.0
        if coverage >= min_coverage:
            score = accuracy * coverage
            threshold_results.append((threshold, accuracy, coverage, score))
            if score > best_score:
                best_score, best_threshold = score, threshold
    print("[THRESHOLD] Đánh giá hoàn thành!")
    if best_threshold is None:
        print(f"[WARNING] Không có threshold nào đạt min_coverage={min_coverage}")
        best_threshold, best_score = max(threshold_range), 0.0
    return best_threshold, best_score, threshold_results


def create_label_map_from_directory(data_dir: str) -> Dict[int, str]:
    """train_lbph_script.py:22-47: label ids follow the reference's sort (numeric folder names first, then
    case-insensitive names)."""
    if not os.path.exists(data_dir):
        raise ValueError(f"Thư mục không tồn tại: {data_dir}")
    identities = sorted([d for d in os.listdir(data_dir) if os.path.isdir(os.path.join(data_dir, d))],
                        key=lambda x: (not x.isdigit(), x if x.isdigit() else x.lower()))
    if len(identities) == 0:
        raise ValueError(f"Không tìm thấy identity nào trong {data_dir}")
    label_map = {idx: identity for idx, identity in enumerate(identities)}
    print(f"[OK] Tạo label_map từ dataset: {len(label_map)} identities")
    return label_map


def _preprocess_image_for_lbph(image_path: str, detector, target_size: Tuple[int, int] = (100, 100)):
    """train_lbph_script.py:50-76 with PIL in place of cv2: load RGB, crop (detector) or resize to target_size
    (W, H) on the package's device resize (align.resize_u8, Pillow's BILINEAR), then gray = convert('L').
    Neither the gray conversion nor the resize is bit-checked against cv2 (cvtColor / cv2.resize INTER_LINEAR)."""
    try:
        import torch
        from PIL import Image

        from .align import resize_u8
        rgb = np.array(Image.open(image_path).convert("RGB"))
        cropped = None
        if detector is not None:
            bgr = detector.crop_face(np.ascontiguousarray(rgb[..., ::-1]), margin=0.2, target_size=target_size)
            if bgr is not None and bgr.size:
                cropped = np.ascontiguousarray(bgr[..., ::-1])
        if cropped is None:
            if (rgb.shape[1], rgb.shape[0]) == tuple(target_size):
                cropped = rgb
            else:
                t = torch.from_numpy(np.ascontiguousarray(rgb))[None].to("cuda")
                cropped = resize_u8(t, int(target_size[1]), int(target_size[0]))[0].cpu().numpy()
        return np.asarray(Image.fromarray(cropped).convert("L"))
    except Exception:
        return None


def _make_detector(use_face_detection: bool):
    if not use_face_detection:
        return None
    from .face_detector import FaceDetector
    return FaceDetector(backend='mtcnn', device='cuda', confidence_threshold=0.9, select_largest=True)


def _load_dir(data_dir: str, identity_to_label: Dict[str, int], identities, detector, target_size):
    faces: List[np.ndarray] = []
    labels: List[int] = []
    for identity in identities:
        identity_path = os.path.join(data_dir, identity)
        if not os.path.isdir(identity_path):
            continue
        for img_name in os.listdir(identity_path):
            if os.path.splitext(img_name.lower())[1] not in IMAGE_EXTENSIONS:
                continue
            img = _preprocess_image_for_lbph(os.path.join(identity_path, img_name), detector, target_size)
            if img is None:
                continue
            faces.append(img)
            labels.append(identity_to_label[identity])
    return faces, np.array(labels, dtype=np.int32)


def load_faces_and_labels(data_dir: str, label_map: Dict[int, str], use_face_detection: bool = True,
                          target_size: Tuple[int, int] = (100, 100)):
    """train_lbph_script.py:79-132: (faces, labels) of data_dir/identity/*.{jpg,png,...} by label_map.  Images are
    read with PIL; with use_face_detection the package's FaceDetector.crop_face crops (margin 0.2), falling back
    to a plain resize when no face is found.  Gray and resize are not bit-checked against cv2."""
    identity_to_label = {v: k for k, v in label_map.items()}
    return _load_dir(data_dir, identity_to_label, sorted(identity_to_label.keys()),
                     _make_detector(use_face_detection), target_size)


def npz_model_name(model_name: str) -> str:
    """The model file name with the extension this package writes: anything but .npz (the reference's default is
    lbph_model.xml, an OpenCV FileStorage this package does not write) is replaced."""
    stem, ext = os.path.splitext(model_name)
    return model_name if ext.lower() == ".npz" else stem + ".npz"


def train_lbph_from_directory(data_dir: str, output_dir: str = "models/checkpoints/LBHP",
                              model_name: str = "lbph_model.npz", radius: int = 1, neighbors: int = 8,
                              grid_x: int = 8, grid_y: int = 8, use_val_for_threshold: bool = False,
                              val_dir: Optional[str] = None, use_face_detection: bool = True,
                              target_size: Tuple[int, int] = (100, 100)):
    """train_lbph_script.py:135-322: trains from an identity-per-folder tree and writes the model (.npz),
    label_map.npy and, when use_val_for_threshold and val_dir are given, optimal_threshold.txt in the reference's
    layout.  Unlike the reference it rewrites no config file.  Returns (model, label_map)."""
    if data_dir is None or not os.path.exists(data_dir):
        raise ValueError(f"Thư mục train không tồn tại: {data_dir}")
    print(f"Model parameters: radius={radius}, neighbors={neighbors}, grid=({grid_x}, {grid_y})")
    print(f"Preprocess: face_detection={'on' if use_face_detection else 'off'}, target_size={target_size}")
    os.makedirs(output_dir, exist_ok=True)

    print("\n[1/4] Đang load training data...")
    label_map = create_label_map_from_directory(data_dir)
    faces, labels = load_faces_and_labels(data_dir, label_map, use_face_detection=use_face_detection,
                                          target_size=target_size)
    if len(faces) == 0:
        raise ValueError(f"Không tìm thấy ảnh nào trong {data_dir}")
    print(f"  Loaded: {len(faces)} faces, {len(np.unique(labels))} unique labels")

    print("\n[3/4] Đang train LBPH model...")
    model = train_lbph_model(faces=faces, labels=labels, radius=radius, neighbors=neighbors, grid_x=grid_x,
                             grid_y=grid_y)
    print("[OK] Training hoàn thành!")

    print("\n[4/4] Đang lưu model và label_map...")
    if npz_model_name(model_name) != model_name:
        print(f"  [INFO] model file is .npz, not OpenCV XML/YAML: {model_name} -> {npz_model_name(model_name)}")
        model_name = npz_model_name(model_name)
    model_path = os.path.join(output_dir, model_name)
    model.save(model_path)
    print(f"  Model saved: {model_path}")
    label_map_path = os.path.join(output_dir, "label_map.npy")
    np.save(label_map_path, label_map)
    print(f"  Label map saved: {label_map_path}")

    if use_val_for_threshold and val_dir:
        print("\n[OPTIONAL] Đang tìm threshold tối ưu trên validation set...")
        try:
            identity_to_label = {v: k for k, v in label_map.items()}
            val_faces, val_labels = _load_dir(val_dir, identity_to_label, list(identity_to_label.keys()),
                                              _make_detector(use_face_detection), target_size)
            print(f"  Validation samples: {len(val_faces)}")
            best_threshold, best_score, threshold_results = find_optimal_threshold(model, val_faces, val_labels)
            print(f"\n  Best threshold: {best_threshold}")
            print(f"  Best score (acc * coverage): {best_score:.4f}")
            threshold_path = os.path.join(output_dir, "optimal_threshold.txt")
            with open(threshold_path, 'w') as f:
                f.write(f"Optimal threshold: {best_threshold}\n")
                f.write(f"Score (accuracy * coverage): {best_score:.4f}\n\n")
                f.write("Threshold analysis:\n")
                f.write("Threshold | Accuracy | Coverage | Score\n")
                f.write("-" * 50 + "\n")
                for thr, acc, cov, score in threshold_results:
                    f.write(f"{thr:9d} | {acc:8.4f} | {cov:8.4f} | {score:.4f}\n")
            print(f"  Threshold analysis saved: {threshold_path}")
        except Exception as e:  # the reference keeps the trained model when the sweep fails
            print(f"[WARNING] Không thể tìm threshold tối ưu: {e}")

    print(f"Total identities: {len(label_map)}")
    print(f"Total training samples: {len(faces)}")
    return model, label_map
