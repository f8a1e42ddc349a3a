"""Training augmentations on the device: the reference's torchvision pipelines (models/arcface/arcface_dataloader.py
get_train_transforms, models/facenet/facenet_dataloader.py) as per-image op lists run by fr_augment, one workgroup per
image with the image resident in LDS (csrc/augment.hip; DESIGN.md §4 "Augmentation").

The random parameters are drawn on the host from a numpy ``Generator`` with torchvision's ``get_params`` distributions;
the same seed gives the same output bit for bit.  Matching torch's random stream is not a goal: a torch seed does not
reproduce the reference's draws.  Every matrix is made here in Python doubles (Pillow and torchvision make theirs with
Python's ``math``), the pixels are made on the device.  The albumentations variants of the reference
(``use_albumentations=True``) are out of scope.
"""
from __future__ import annotations

import math

import numpy as np

from . import _native as N

(OP_NOP, OP_FLIP_H, OP_AFFINE_NEAREST, OP_PERSPECTIVE_BILINEAR, OP_CROP_RESIZE, OP_BRIGHTNESS, OP_CONTRAST,
 OP_SATURATION, OP_HUE, OP_GRAYSCALE, OP_GAUSS_BLUR, OP_ERASE) = range(12)
MAX_OPS = 16  # FR_AUGMENT_MAX_OPS
NARGS = 8     # FR_AUGMENT_ARGS


# ---- matrices (host, Python doubles) ----

def rotation_matrix(angle: float, width: int, height: int):
    """The 6 inverse-map coefficients of PIL ``Image.rotate(angle)`` about the centre, no expand: Pillow's own preamble
    (angle modulo 360, ``round(cos, 15)``, the centre shift).  Pillow answers 0, 180 and (on a square image) 90 and 270
    degrees with a copy or a transpose; the fixed-point walk over this matrix gives the same pixels."""
    angle = angle % 360.0
    cx, cy = width / 2.0, height / 2.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def inverse_affine_matrix(center, angle: float, translate, scale: float, shear):
    """torchvision's ``_get_inverse_affine_matrix`` (torchvision is not installed: restated, parity with torchvision
    unpinned): the output-to-input map of a rotation by ``angle`` and a shear (degrees) about ``center``, a scale and a
    translation."""
    rot, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m = [x / scale for x in m]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def perspective_coeffs(startpoints, endpoints):
    """torchvision's ``_get_perspective_coeffs`` (restated, parity with torchvision unpinned): the 8 coefficients that
    map the end points to the start points, least squares in float64, rounded to float32 as torchvision returns them."""
    A = np.zeros((8, 8), np.float64)
    for i, (p1, p2) in enumerate(zip(endpoints, startpoints)):
        A[2 * i] = [p1[0], p1[1], 1, 0, 0, 0, -p2[0] * p1[0], -p2[0] * p1[1]]
        A[2 * i + 1] = [0, 0, 0, p1[0], p1[1], 1, -p2[1] * p1[0], -p2[1] * p1[1]]
    b = np.asarray(startpoints, np.float64).reshape(8)
    res = np.linalg.lstsq(A, b, rcond=None)[0]
    return [float(v) for v in res.astype(np.float32)]


def gaussian_kernel1d(k: int, sigma: float):
    """torchvision's ``_get_gaussian_kernel1d`` in float32 (numpy's exp, not torch's: parity unpinned)."""
    half = (k - 1) * 0.5
    x = np.linspace(-half, half, k, dtype=np.float32)
    pdf = np.exp(np.float32(-0.5) * (x / np.float32(sigma)) ** 2, dtype=np.float32)
    return (pdf / pdf.sum(dtype=np.float32)).astype(np.float32)


# ---- the sampler ----

def _jitter_range(x, center=1.0):
    return (max(0.0, center - x), center + x) if center else (-x, x)


class DeviceTransform:
    """One of the reference's transform lists, as a sampler of op lists plus the device call.

    ``steps`` is a list of tuples naming torchvision transforms in the reference's order:
    ("resized_crop", scale, ratio), ("flip", p), ("rotation", degrees), ("affine", degrees, translate, scale, shear),
    ("perspective", distortion_scale, p), ("jitter", brightness, contrast, saturation, hue), ("gray", p),
    ("blur", kernel_size, (sigma_lo, sigma_hi)), ("erase", p, scale, ratio).  ToTensor and Normalize(0.5, 0.5) always
    end the list (the erase comes after them, as in the reference)."""

    def __init__(self, image_size: int, steps=()):
        self.image_size = int(image_size)
        self.steps = list(steps)

    def __repr__(self):
        return f"DeviceTransform(image_size={self.image_size}, steps={self.steps})"

    def _sample_one(self, g):
        S = self.image_size
        W = H = S
        prog = []
        for st in self.steps:
            kind = st[0]
            if kind == "resized_crop":
                prog.append((OP_CROP_RESIZE, _resized_crop_box(g, H, W, st[1], st[2])))
            elif kind == "flip":
                if g.random() < st[1]:
                    prog.append((OP_FLIP_H, ()))
            elif kind == "rotation":
                prog.append((OP_AFFINE_NEAREST, rotation_matrix(float(g.uniform(-st[1], st[1])), W, H)))
            elif kind == "affine":
                _, degrees, translate, scale, shear = st
                angle = float(g.uniform(-degrees, degrees))
                tx = int(round(float(g.uniform(-translate[0] * W, translate[0] * W))))
                ty = int(round(float(g.uniform(-translate[1] * H, translate[1] * H))))
                sc = float(g.uniform(scale[0], scale[1]))
                shx = float(g.uniform(-shear, shear))
                prog.append((OP_AFFINE_NEAREST, inverse_affine_matrix((W * 0.5, H * 0.5), angle, (tx, ty), sc, (shx, 0.0))))
            elif kind == "perspective":
                if g.random() < st[2]:
                    dw, dh = int(st[1] * (W // 2)), int(st[1] * (H // 2))
                    tl = [int(g.integers(0, dw + 1)), int(g.integers(0, dh + 1))]
                    tr = [int(g.integers(W - dw - 1, W)), int(g.integers(0, dh + 1))]
                    br = [int(g.integers(W - dw - 1, W)), int(g.integers(H - dh - 1, H))]
                    bl = [int(g.integers(0, dw + 1)), int(g.integers(H - dh - 1, H))]
                    start = [[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]]
                    prog.append((OP_PERSPECTIVE_BILINEAR, perspective_coeffs(start, [tl, tr, br, bl])))
            elif kind == "jitter":
                order = g.permutation(4)
                ranges = [_jitter_range(st[1]), _jitter_range(st[2]), _jitter_range(st[3]),
                          _jitter_range(st[4], 0.0) if st[4] is not None else None]
                fac = [None if r is None else float(g.uniform(r[0], r[1])) for r in ranges]
                for fn in order:
                    if fac[fn] is not None:
                        prog.append(((OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE)[fn], (fac[fn],)))
            elif kind == "gray":
                if g.random() < st[1]:
                    prog.append((OP_GRAYSCALE, ()))
            elif kind == "blur":
                k = int(st[1])
                sigma = float(g.uniform(st[2][0], st[2][1]))
                prog.append((OP_GAUSS_BLUR, [float(k)] + [float(v) for v in gaussian_kernel1d(k, sigma)]))
            elif kind == "erase":
                if g.random() < st[1]:
                    box = _erase_box(g, H, W, st[2], st[3])
                    if box is not None:
                        prog.append((OP_ERASE, box))
            else:
                raise ValueError(f"unknown step {kind!r}")
        return prog

    def sample(self, B: int, generator=None):
        """Draw B programs: (ops int32 [B, 16], args float64 [B, 16, 8]), host arrays for ``apply``."""
        g = generator if isinstance(generator, np.random.Generator) else np.random.default_rng(generator)
        ops = np.zeros((B, MAX_OPS), np.int32)
        args = np.zeros((B, MAX_OPS, NARGS), np.float64)
        for b in range(B):
            prog = self._sample_one(g)
            if len(prog) > MAX_OPS:
                raise ValueError(f"a program of {len(prog)} ops exceeds the {MAX_OPS} fr_augment runs")
            for k, (op, a) in enumerate(prog):
                ops[b, k] = op
                args[b, k, :len(a)] = a
        return ops, args

    def apply(self, images, ops, args, return_u8: bool = False):
        """Run the programs on cuda u8 ``images`` [B, S, S, 3] -> cuda f32 [B, 3, image_size, image_size], normalised
        to [-1, 1] (``FRModel.features`` / ``embed`` take it as it is); with ``return_u8`` also the u8 images before
        the erase.  A size other than ``image_size`` goes through ``align.resize_u8`` first (the reference's leading
        Resize; the 'heavy' preset crops the resized image where the reference crops the original)."""
        return augment(self._sized(images), ops, args, return_u8=return_u8)

    def _sized(self, images):
        images = _check(images)
        S = self.image_size
        if images.shape[1] != S or images.shape[2] != S:
            from .align import resize_u8
            images = resize_u8(images, S, S)
        return images

    def __call__(self, images, generator=None):
        images = _check(images)
        ops, args = self.sample(images.shape[0], generator)
        return self.apply(images, ops, args)


def _resized_crop_box(g, H, W, scale, ratio):
    area = H * W
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(10):
        target = area * float(g.uniform(scale[0], scale[1]))
        aspect = math.exp(float(g.uniform(lo, hi)))
        w = int(round(math.sqrt(target * aspect)))
        h = int(round(math.sqrt(target / aspect)))
        if 0 < w <= W and 0 < h <= H:
            return [int(g.integers(0, H - h + 1)), int(g.integers(0, W - w + 1)), h, w]
    in_ratio = W / H  # torchvision's centre crop
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    return [(H - h) // 2, (W - w) // 2, h, w]


def _erase_box(g, H, W, scale, ratio):
    area = H * W
    lo, hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(10):
        target = area * float(g.uniform(scale[0], scale[1]))
        aspect = math.exp(float(g.uniform(lo, hi)))
        h = int(round(math.sqrt(target * aspect)))
        w = int(round(math.sqrt(target / aspect)))
        if not (h < H and w < W):
            continue
        if h < 1 or w < 1:
            return None  # an empty rectangle erases nothing
        return [int(g.integers(0, H - h + 1)), int(g.integers(0, W - w + 1)), h, w]
    return None


# ---- the device call ----

def _check(images):
    import torch
    if not (isinstance(images, torch.Tensor) and images.is_cuda):
        raise RuntimeError("augmentation needs ROCm GPU tensors; there is deliberately no CPU fallback")
    if images.dim() != 4 or images.shape[3] != 3 or images.dtype != torch.uint8:
        raise ValueError(f"augmentation: uint8 images [B, H, W, 3] expected, got {images.dtype} {tuple(images.shape)}")
    return images


def augment(images, ops, args, return_u8: bool = False, return_f32: bool = True):
    """fr_augment: cuda u8 ``images`` [B, H, W, 3], host ``ops`` int32 [B, n] and ``args`` float64 [B, n, 8] (n <= 16)
    -> cuda f32 [B, 3, H, W] and / or cuda u8 [B, H, W, 3]."""
    import torch
    x = _check(images).contiguous()
    B, H, W, _ = x.shape
    ops = np.ascontiguousarray(ops, dtype=np.int32)
    args = np.ascontiguousarray(args, dtype=np.float64)
    if ops.ndim != 2 or ops.shape[0] != B or args.shape != ops.shape + (NARGS,):
        raise ValueError(f"augmentation: ops [B, n] and args [B, n, {NARGS}] expected, got {ops.shape} and {args.shape}")
    if not (return_u8 or return_f32):
        raise ValueError("augmentation: nothing to return")
    n = ops.shape[1]
    L = N.lib()
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=x.device) if return_f32 else None
    out8 = torch.empty((B, H, W, 3), dtype=torch.uint8, device=x.device) if return_u8 else None
    nws = int(L.fr_augment_workspace(B, n))
    ws = torch.empty((max(nws, 16),), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        N.check(L.fr_augment(N.ptr(x), B, H, W, ops.ctypes.data, args.ctypes.data, n, N.ptr(out), N.ptr(out8), N.ptr(ws),
                             nws, N.stream_ptr(x.device)), "fr_augment")
    if return_u8 and return_f32:
        return out, out8
    return out if return_f32 else out8


# ---- the reference's presets ----

_ARCFACE = {
    "light": [("flip", 0.5), ("jitter", 0.1, 0.1, 0.05, 0.02)],
    "normal": [("flip", 0.5), ("rotation", 10), ("jitter", 0.2, 0.2, 0.1, 0.05)],
    "strong": [("flip", 0.5), ("rotation", 15), ("affine", 0, (0.1, 0.1), (0.9, 1.1), 5),
               ("jitter", 0.3, 0.3, 0.2, 0.1), ("gray", 0.1), ("blur", 3, (0.1, 2.0)),
               ("erase", 0.3, (0.02, 0.15), (0.3, 3.3))],
    "heavy": [("resized_crop", (0.85, 1.0), (0.95, 1.05)), ("flip", 0.5), ("rotation", 20),
              ("affine", 15, (0.1, 0.1), (0.85, 1.15), 8), ("perspective", 0.2, 0.3),
              ("jitter", 0.4, 0.4, 0.3, 0.1), ("gray", 0.15), ("blur", 5, (0.1, 3.0)),
              ("erase", 0.4, (0.05, 0.2), (0.3, 3.3))],
}


def get_train_transforms(image_size=112, use_albumentations=False, augment_strength='normal'):
    """The reference's ``get_train_transforms`` (torchvision lists): a ``DeviceTransform`` for 'light', 'normal',
    'strong' or 'heavy' (anything else is 'normal', as in the reference).  The albumentations lists are not built."""
    if use_albumentations:
        raise NotImplementedError("the albumentations variants are out of scope; use use_albumentations=False")
    return DeviceTransform(image_size, _ARCFACE.get(augment_strength, _ARCFACE["normal"]))


def get_val_transforms(image_size=112, use_albumentations=False):
    """The reference's ``get_val_transforms``: resize and normalise only."""
    if use_albumentations:
        raise NotImplementedError("the albumentations variants are out of scope; use use_albumentations=False")
    return DeviceTransform(image_size, [])


def facenet_train_transforms(image_size=160, online=False):
    """The augment=True lists of the FaceNet datasets: TripletFaceDataset (flip, jitter) and, with ``online``,
    OnlineTripletDataset (flip, jitter, rotation by up to 10 degrees)."""
    steps = [("flip", 0.5), ("jitter", 0.2, 0.2, 0.2, None)]
    if online:
        steps.append(("rotation", 10))
    return DeviceTransform(image_size, steps)


def mixup_data(x, y, alpha=0.2, generator=None):
    """The reference's ``mixup_data`` on device tensors: (mixed_x, y_a, y_b, lam).  ``generator``: a numpy Generator for
    lam and the permutation; None draws as the reference does (numpy's and torch's global streams).
    ``ArcMarginProduct.loss(..., label_b=y_b, lam=lam)`` takes the result."""
    import torch
    batch_size = x.size(0)
    if generator is None:
        lam = float(np.random.beta(alpha, alpha)) if alpha > 0 else 1.0
        index = torch.randperm(batch_size).to(x.device)
    else:
        lam = float(generator.beta(alpha, alpha)) if alpha > 0 else 1.0
        index = torch.from_numpy(generator.permutation(batch_size)).to(x.device)
    mixed_x = lam * x + (1 - lam) * x[index, :]
    return mixed_x, y, y[index], lam
