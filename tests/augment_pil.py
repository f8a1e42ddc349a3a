"""The reference pipeline of the augmentation tests: the same op lists run by Pillow (and, for the blur and the
normalisation, torch on the CPU) the way torchvision's PIL backend runs them.  Images are u8 [H][W][3]."""
import numpy as np
from PIL import Image, ImageEnhance

from tests import augment_ref as R


def pil_hue(im, f):
    """torchvision's PIL adjust_hue."""
    h, s, v = im.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    np_h += np.uint8(R.hue_shift(f))
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def torch_blur(img, k, w1d, dtype=None):
    """torchvision's tensor gaussian_blur of a u8 image with the given 1-D f32 kernel, on the CPU."""
    import torch
    import torch.nn.functional as F
    k = int(k)
    w = torch.from_numpy(np.asarray(w1d[:k], np.float64).astype(np.float32))
    k2 = torch.mm(w[:, None], w[None, :]).to(dtype or torch.float32)
    x = torch.from_numpy(np.array(img)).permute(2, 0, 1)[None].to(k2.dtype)
    x = F.pad(x, [k // 2] * 4, mode="reflect")
    y = F.conv2d(x, k2.expand(3, 1, k, k), groups=3)[0].permute(1, 2, 0)
    if dtype is not None:
        return y.numpy()
    return torch.round(y).to(torch.uint8).numpy()


def run_op(im, op, a):
    op = int(op)
    if op == R.FLIP_H:
        return im.transpose(Image.FLIP_LEFT_RIGHT)
    if op == R.AFFINE_NEAREST:
        return im.transform(im.size, Image.AFFINE, [float(v) for v in a[:6]], Image.NEAREST)
    if op == R.PERSPECTIVE_BILINEAR:
        return im.transform(im.size, Image.PERSPECTIVE, [float(v) for v in a[:8]], Image.BILINEAR)
    if op == R.CROP_RESIZE:
        i, j, h, w = (int(v) for v in a[:4])
        return im.crop((j, i, j + w, i + h)).resize(im.size, Image.BILINEAR)
    if op == R.BRIGHTNESS:
        return ImageEnhance.Brightness(im).enhance(float(a[0]))
    if op == R.CONTRAST:
        return ImageEnhance.Contrast(im).enhance(float(a[0]))
    if op == R.SATURATION:
        return ImageEnhance.Color(im).enhance(float(a[0]))
    if op == R.HUE:
        return pil_hue(im, float(a[0]))
    if op == R.GRAYSCALE:
        L = im.convert("L")
        return Image.merge("RGB", (L, L, L))
    if op == R.GAUSS_BLUR:
        return Image.fromarray(torch_blur(np.asarray(im), a[0], a[1:8]))
    raise ValueError(op)


def run_program(img, ops, args):
    """(u8 before erasing, f32 [3][H][W] after ToTensor, Normalize(0.5, 0.5) and the erase)."""
    import torch
    im = Image.fromarray(np.ascontiguousarray(img))
    erase = None
    for op, a in zip(ops, args):
        if int(op) == R.NOP:
            continue
        if int(op) == R.ERASE:
            erase = [int(v) for v in a[:4]]
            continue
        im = run_op(im, op, a)
    u8 = np.asarray(im).copy()
    t = torch.from_numpy(u8).permute(2, 0, 1).to(torch.float32).div(255)
    t = (t - 0.5) / 0.5
    if erase:
        i, j, h, w = erase
        t[:, i:i + h, j:j + w] = 0.0
    return u8, t.numpy()


def rand_image(rng, H, W):
    """Smooth ramps plus noise, so blends, hues and resampling see both flat and busy neighbourhoods."""
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(x * 255 // max(W - 1, 1)), (y * 255 // max(H - 1, 1)), ((x + y) * 7) % 256], -1)
    noise = rng.integers(-40, 41, (H, W, 3))
    img = np.clip(base + noise, 0, 255)
    if rng.random() < 0.2:
        img = rng.integers(0, 256, (H, W, 3))
    return img.astype(np.uint8)


def tie_rule(got, exact, what):
    """got (u8) against the float64 sums: equal to their rounding away from ties, within 1 near one."""
    near = np.abs(exact - np.floor(exact) - 0.5) <= 1e-3
    want = np.clip(np.rint(exact), 0, 255)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    assert np.all(diff[~near] == 0) and np.all(diff <= 1), (what, int(diff.max()), int((diff != 0).sum()))
