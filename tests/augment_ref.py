"""Numpy restatement of facerecognition_amd/csrc/augment.hip: every op of the augmentation interpreter and the
interpreter itself, in the arithmetic the kernel uses (integers, f32 and f64 exactly where Pillow / torchvision use
them, no fused multiply-add).  test_augment_ref.py checks each op against Pillow itself; test_gpu_augment.py checks the
device against this file bit for bit.  Images are u8 [H][W][3]."""
import math

import numpy as np

NOP, FLIP_H, AFFINE_NEAREST, PERSPECTIVE_BILINEAR, CROP_RESIZE, BRIGHTNESS, CONTRAST, SATURATION, HUE, GRAYSCALE, \
    GAUSS_BLUR, ERASE = range(12)
MAX_OPS, NARGS = 16, 8
PB = 22  # Pillow's PRECISION_BITS


def norm_table():
    """ToTensor then Normalize(0.5, 0.5) in f32, per byte."""
    u = np.arange(256, dtype=np.float32)
    return (u / np.float32(255) - np.float32(0.5)) / np.float32(0.5)


def flip_h(img):
    return img[:, ::-1].copy()


def _fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def affine_nearest(img, m):
    """Image.transform(size, AFFINE, m, NEAREST), fill 0: Pillow's 16.16 fixed-point walk (int32 wrap-around)."""
    H, W = img.shape[:2]
    m = [float(v) for v in m]
    a0, a1, a3, a4 = _fix(m[0]), _fix(m[1]), _fix(m[3]), _fix(m[4])
    a2 = _fix(m[2] + m[0] * 0.5 + m[1] * 0.5)
    a5 = _fix(m[5] + m[3] * 0.5 + m[4] * 0.5)
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)

    def wrap(v):
        return ((v + 2 ** 31) % 2 ** 32) - 2 ** 31

    sx = wrap(a2 + a1 * y + a0 * x) >> 16
    sy = wrap(a5 + a4 * y + a3 * x) >> 16
    ok = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    out = np.zeros_like(img)
    out[ok] = img[sy[ok], sx[ok]]
    return out


def perspective_bilinear(img, a):
    """Image.transform(size, PERSPECTIVE, a, BILINEAR), fill 0: double arithmetic, truncating store."""
    H, W = img.shape[:2]
    a = np.asarray(a, np.float64)
    y, x = np.mgrid[0:H, 0:W]
    xi, yi = x + 0.5, y + 0.5
    with np.errstate(all="ignore"):
        den = a[6] * xi + a[7] * yi + 1
        xin = (a[0] * xi + a[1] * yi + a[2]) / den
        yin = (a[3] * xi + a[4] * yi + a[5]) / den
        ok = (xin >= 0.0) & (xin < W) & (yin >= 0.0) & (yin < H)  # a NaN is outside
    xin = np.where(ok, xin, 0.5) - 0.5
    yin = np.where(ok, yin, 0.5) - 0.5
    fx, fy = np.floor(xin), np.floor(yin)
    dx, dy = (xin - fx)[..., None], (yin - fy)[..., None]
    fx, fy = fx.astype(np.int64), fy.astype(np.int64)
    x0, x1 = np.clip(fx, 0, W - 1), np.clip(fx + 1, 0, W - 1)
    y0 = np.clip(fy, 0, H - 1)
    im = img.astype(np.float64)
    p, q = im[y0, x0], im[y0, x1]
    v1 = p + (q - p) * dx
    has = (fy + 1 >= 0) & (fy + 1 < H)
    y1 = np.where(has, fy + 1, 0)
    p, q = im[y1, x0], im[y1, x1]
    v2 = np.where(has[..., None], p + (q - p) * dx, v1)
    v = v1 + (v2 - v1) * dy
    return np.where(ok[..., None], v.astype(np.int64), 0).astype(np.uint8)


def resample_coeffs(in_size, out_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for BILINEAR over the box [0, in_size], in_size <= out_size
    (a crop never exceeds the image, so the support is 1 and there are at most 3 taps): [(xmin, [k...])]."""
    scale = float(in_size) / out_size
    assert scale <= 1.0
    support, ss = 1.0, 1.0
    tab = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = []
        for x in range(xmax):
            t = abs((x + xmin - center + 0.5) * ss)
            k.append(1.0 - t if t < 1.0 else 0.0)
        ww = sum(k, 0.0)
        if ww != 0.0:
            k = [v / ww for v in k]
        tab.append((xmin, [int(0.5 + v * (1 << PB)) for v in k]))
    return tab


def _clip8(v):
    return np.clip(v >> PB, 0, 255).astype(np.uint8)


def crop_resize(img, i, j, h, w):
    """crop((j, i, j + w, i + h)).resize((W, H), BILINEAR): horizontal pass, then vertical; a pass whose size does not
    change is skipped, as Pillow skips it."""
    H, W = img.shape[:2]
    i, j, h, w = int(i), int(j), int(h), int(w)
    cur = img[i:i + h, j:j + w].astype(np.int64)
    if w != W:
        out = np.empty((h, W, 3), np.uint8)
        for x, (xmin, k) in enumerate(resample_coeffs(w, W)):
            s = np.full((h, 3), 1 << (PB - 1), np.int64)
            for t, kv in enumerate(k):
                s += cur[:, xmin + t] * kv
            out[:, x] = _clip8(s)
        cur = out.astype(np.int64)
    if h != H:
        out = np.empty((H, W, 3), np.uint8)
        for y, (ymin, k) in enumerate(resample_coeffs(h, H)):
            s = np.full((W, 3), 1 << (PB - 1), np.int64)
            for t, kv in enumerate(k):
                s += cur[ymin + t] * kv
            out[y] = _clip8(s)
        cur = out
    return cur.astype(np.uint8)


def luma(img):
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.uint8)


def blend(deg, src, f):
    """Image.blend(degenerate, image, f): t = deg + f32(f) (src - deg) in f32, every operation rounded."""
    f = np.float32(f)
    d = deg.astype(np.float32)
    t = d + f * (src.astype(np.float32) - d)
    if not (f >= 0 and f <= 1):
        t = np.clip(t, np.float32(0), np.float32(255))
    return t.astype(np.int32).astype(np.uint8)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def contrast(img, f):
    L = luma(img)
    n = L.size
    mean = (2 * int(L.sum(dtype=np.int64)) + n) // (2 * n)
    return blend(np.full_like(img, mean), img, f)


def saturation(img, f):
    return blend(np.repeat(luma(img)[..., None], 3, 2), img, f)


def grayscale(img):
    return np.repeat(luma(img)[..., None], 3, 2)


def rgb_to_hsv(img):
    """Pillow's convert("HSV"): f32 quotients, the hue sum in double rounded to f32 once, bytes by (int)(x 255.0)."""
    r, g, b = (img[..., c].astype(np.int32) for c in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    cr = np.where(grey, 1, maxc - minc).astype(np.float32)
    s = cr / np.where(grey, 1, maxc).astype(np.float32)
    rc, gc, bc = ((maxc - c).astype(np.float32) / cr for c in (r, g, b))
    rc64, gc64, bc64 = (c.astype(np.float64) for c in (rc, gc, bc))
    h = np.where(r == maxc, (bc - gc).astype(np.float64),
                 np.where(g == maxc, 2.0 + rc64 - bc64, 4.0 + gc64 - rc64)).astype(np.float32)
    x = h.astype(np.float64) / 6.0 + 1.0
    h = np.where(x >= 1.0, x - 1.0, x).astype(np.float32)  # fmod(x, 1.0) for x in [0.5, 2)
    uh = np.clip((h.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    us = np.clip((s.astype(np.float64) * 255.0).astype(np.int32), 0, 255)
    return np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], -1).astype(np.uint8)


def hsv_to_rgb(hsv):
    """Pillow's HSV -> RGB: colorsys with C round() on p, q and t, all in f32."""
    h, s, v = (hsv[..., c] for c in range(3))
    one = np.float32(1)
    fh = (h.astype(np.float64) * 6.0 / 255.0).astype(np.float32)
    i = np.floor(fh)
    f = fh - i
    fs = (s.astype(np.float64) / 255.0).astype(np.float32)
    vf = v.astype(np.float32)

    def rnd(x):  # non-negative: half away from zero
        fl = np.floor(x)
        return np.clip(np.where(x - fl >= np.float32(0.5), fl + one, fl), 0, 255).astype(np.uint8)

    p, q, t = rnd(vf * (one - fs)), rnd(vf * (one - fs * f)), rnd(vf * (one - fs * (one - f)))
    sel = i.astype(np.int32) % 6
    out = np.stack([np.choose(sel, [v, q, p, p, t, v]), np.choose(sel, [t, v, v, q, p, p]),
                    np.choose(sel, [p, p, t, v, v, q])], -1)
    return np.where((s == 0)[..., None], v[..., None], out).astype(np.uint8)


def hue_shift(f):
    """numpy's uint8(f 255): truncation towards zero, then the u8 wrap."""
    return int(float(f) * 255.0) & 255


def hue(img, f):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + hue_shift(f)) & 255
    return hsv_to_rgb(hsv)


def reflect(idx, n):
    idx = np.where(idx < 0, -idx, idx)
    return np.where(idx >= n, 2 * (n - 1) - idx, idx)


def gauss_blur(img, k, w1d, dtype=np.float32):
    """torchvision's tensor blur of a u8 image: w2[dy][dx] = w[dy] w[dx] (one f32 product), reflect padding, the sum
    in f32 in row-major tap order from 0, round half to even, clamp to a byte.  dtype=float64 returns the unrounded
    double sums over the same f32 taps (the tie rule of the tests)."""
    k = int(k)
    H, W = img.shape[:2]
    w = np.asarray(w1d[:k], np.float64).astype(np.float32)
    r = k // 2
    ys, xs = np.arange(H), np.arange(W)
    acc = np.zeros(img.shape, dtype)
    src = img.astype(dtype)
    for dy in range(k):
        yy = reflect(ys + dy - r, H)
        for dx in range(k):
            xx = reflect(xs + dx - r, W)
            w2 = dtype(w[dy] * w[dx])
            acc = acc + w2 * src[yy][:, xx]
    if dtype is np.float64:
        return acc
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def run_program(img, ops, args):
    """The interpreter on one image: (u8 [H][W][3] before erasing, f32 [3][H][W] normalised and erased)."""
    img = np.ascontiguousarray(img)
    H, W = img.shape[:2]
    erase = None
    for op, a in zip(ops, args):
        op = int(op)
        if op == NOP:
            continue
        assert erase is None, "ERASE must be the last op"
        if op == FLIP_H:
            img = flip_h(img)
        elif op == AFFINE_NEAREST:
            img = affine_nearest(img, a[:6])
        elif op == PERSPECTIVE_BILINEAR:
            img = perspective_bilinear(img, a[:8])
        elif op == CROP_RESIZE:
            img = crop_resize(img, *a[:4])
        elif op == BRIGHTNESS:
            img = brightness(img, a[0])
        elif op == CONTRAST:
            img = contrast(img, a[0])
        elif op == SATURATION:
            img = saturation(img, a[0])
        elif op == HUE:
            img = hue(img, a[0])
        elif op == GRAYSCALE:
            img = grayscale(img)
        elif op == GAUSS_BLUR:
            img = gauss_blur(img, a[0], a[1:8])
        elif op == ERASE:
            erase = [int(v) for v in a[:4]]
        else:
            raise ValueError(f"unknown opcode {op}")
    f32 = norm_table()[img].transpose(2, 0, 1).copy()
    if erase:
        i, j, h, w = erase
        f32[:, i:i + h, j:j + w] = 0.0
    return img, f32


def run_batch(images, ops, args):
    outs = [run_program(im, o, a) for im, o, a in zip(images, ops, args)]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
