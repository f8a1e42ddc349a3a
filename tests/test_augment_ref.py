"""tests/augment_ref.py (the numpy restatement of csrc/augment.hip) against Pillow itself, bit for bit, and the host
side of facerecognition_amd/augment.py: the matrix builders against Image.rotate, the sampler's distributions.  No
GPU.  The blur is checked against a float64 evaluation of the same taps and against torch's conv2d under the tie rule:
equal wherever the float64 sum is farther than 1e-3 from a half-integer, within 1 elsewhere.  The 1e-3: the products
w2 * pixel round by at most 2^-24 of themselves and sum to at most 255, 1.5e-5 in all; each of the at most 49 additions
rounds a partial sum <= 255 by at most 255 * 2^-24 = 1.5e-5, 7.5e-4 in all; so an f32 sum in any order lies within
7.7e-4 < 1e-3 of the float64 sum over the same f32 taps."""
import itertools
import math
import os

import numpy as np
import pytest
from PIL import Image, ImageEnhance

from facerecognition_amd import augment as A
from tests import augment_pil as P
from tests import augment_ref as R
from tests.augment_pil import rand_image, tie_rule

SIZES = [(20, 28), (37, 23), (1, 1), (3, 5), (16, 16)]  # (H, W)


def cases(n, seed):
    rng = np.random.default_rng(seed)
    for t in range(n):
        H, W = SIZES[t % len(SIZES)]
        yield rng, rand_image(rng, H, W)


def pil(img):
    return Image.fromarray(img)


def test_flip_and_grayscale():
    for rng, img in cases(20, 0):
        assert np.array_equal(R.flip_h(img), np.asarray(pil(img).transpose(Image.FLIP_LEFT_RIGHT)))
        assert np.array_equal(R.grayscale(img), np.asarray(P.run_op(pil(img), R.GRAYSCALE, ())))
        assert np.array_equal(R.luma(img), np.asarray(pil(img).convert("L")))


ANGLES = [0.0, 90.0, 180.0, 270.0, 1e-9, -1e-9, 20.0, -20.0, 360.0, -90.0]


def test_rotation_matrix_against_image_rotate():
    n = 0
    for t, (rng, img) in enumerate(cases(260, 1)):
        H, W = img.shape[:2]
        angle = ANGLES[t % len(ANGLES)] if t < 50 else float(rng.uniform(-180, 180))
        got = R.affine_nearest(img, A.rotation_matrix(angle, W, H))
        assert np.array_equal(got, np.asarray(pil(img).rotate(angle))), (angle, H, W)
        n += 1
    assert n >= 200


def test_affine_nearest_against_transform():
    for t, (rng, img) in enumerate(cases(300, 2)):
        H, W = img.shape[:2]
        angle, shear = float(rng.uniform(-30, 30)), float(rng.uniform(-10, 10))
        tx, ty = int(round(rng.uniform(-0.3 * W, 0.3 * W))), int(round(rng.uniform(-0.3 * H, 0.3 * H)))
        if t % 10 == 0:
            tx, ty = (W, 0) if t % 20 else (0, -H)  # the whole image moves out
            angle = shear = 0.0
        scale = 1.0 if t % 10 == 0 else float(rng.uniform(0.7, 1.3))
        m = A.inverse_affine_matrix((W * 0.5, H * 0.5), angle, (tx, ty), scale, (shear, 0.0))
        if m[1] == 0.0 and m[3] == 0.0:
            m[1] = 1e-12  # Pillow answers a pure scale from another routine; the op is the fixed-point walk
        want = np.asarray(pil(img).transform((W, H), Image.AFFINE, m, Image.NEAREST))
        assert np.array_equal(R.affine_nearest(img, m), want), (m, H, W)
        if t % 10 == 0:
            assert not want.any()


def test_perspective_bilinear_against_transform():
    ident = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    for t, (rng, img) in enumerate(cases(300, 3)):
        H, W = img.shape[:2]
        if t < 5:
            a = ident
        else:
            d = float(rng.uniform(0.0, 0.5))
            dw, dh = int(d * (W // 2)), int(d * (H // 2))
            end = [[rng.integers(0, dw + 1), rng.integers(0, dh + 1)], [rng.integers(W - dw - 1, W), rng.integers(0, dh + 1)],
                   [rng.integers(W - dw - 1, W), rng.integers(H - dh - 1, H)], [rng.integers(0, dw + 1), rng.integers(H - dh - 1, H)]]
            start = [[0, 0], [W - 1, 0], [W - 1, H - 1], [0, H - 1]]
            if W < 3 or H < 3:
                a = [1.0 + rng.uniform(-.2, .2), rng.uniform(-.2, .2), rng.uniform(-1, 1), rng.uniform(-.2, .2),
                     1.0 + rng.uniform(-.2, .2), rng.uniform(-1, 1), rng.uniform(-.01, .01), rng.uniform(-.01, .01)]
            else:
                a = A.perspective_coeffs(start, [[int(p[0]), int(p[1])] for p in end])
        want = np.asarray(pil(img).transform((W, H), Image.PERSPECTIVE, a, Image.BILINEAR))
        assert np.array_equal(R.perspective_bilinear(img, a), want), (a, H, W)
        if t < 5:
            assert np.array_equal(want, img)
    pts = [[0, 0], [9, 0], [9, 7], [0, 7]]
    assert np.allclose(A.perspective_coeffs(pts, pts), ident, rtol=0, atol=1e-6)


def test_crop_resize_against_crop_and_resize():
    for t, (rng, img) in enumerate(cases(300, 4)):
        H, W = img.shape[:2]
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        if t % 7 == 0:
            h, w = H, W  # the full image
        elif t % 7 == 1:
            h, w = 1, 1
        elif t % 7 == 2:
            h = H  # one pass only
        elif t % 7 == 3:
            w = W
        i, j = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        want = np.asarray(pil(img).crop((j, i, j + w, i + h)).resize((W, H), Image.BILINEAR))
        assert np.array_equal(R.crop_resize(img, i, j, h, w), want), (i, j, h, w, H, W)


@pytest.mark.parametrize("name,ref,enh", [("brightness", R.brightness, ImageEnhance.Brightness),
                                          ("contrast", R.contrast, ImageEnhance.Contrast),
                                          ("saturation", R.saturation, ImageEnhance.Color)])
def test_enhance_against_imageenhance(name, ref, enh):
    edge = [0.0, 1.0, 0.6, 1.4]
    for t, (rng, img) in enumerate(cases(240, 5)):
        f = edge[t % 4] if t < 40 else float(rng.uniform(0.0, 2.0))
        if t % 13 == 0:
            img = np.full_like(img, int(rng.integers(0, 256)))  # a constant image
        assert np.array_equal(ref(img, f), np.asarray(enh(pil(img)).enhance(f))), (name, f, img.shape)


def test_hue_against_pil_adjust_hue():
    edge = [0.0, 0.5, -0.5, 0.37, -0.01]
    for t, (rng, img) in enumerate(cases(220, 6)):
        f = edge[t % 5] if t < 40 else float(rng.uniform(-0.5, 0.5))
        assert np.array_equal(R.hue(img, f), np.asarray(P.pil_hue(pil(img), f))), f
    assert R.hue_shift(0.5) == 127 and R.hue_shift(-0.5) == 129 and R.hue_shift(-0.01) == 254 and R.hue_shift(0) == 0


def all_colours():
    i = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], 1).astype(np.uint8).reshape(4096, 4096, 3)


@pytest.mark.slow
def test_rgb_to_hsv_all_colours():
    c = all_colours()
    want = np.frombuffer(pil(c).convert("HSV").tobytes(), np.uint8).reshape(c.shape)
    assert np.array_equal(R.rgb_to_hsv(c), want)


@pytest.mark.slow
def test_hsv_to_rgb_all_colours():
    c = all_colours()
    want = np.asarray(Image.frombytes("HSV", (4096, 4096), c.tobytes()).convert("RGB"))
    assert np.array_equal(R.hsv_to_rgb(c), want)


BLURS = [(3, 0.1), (3, 2.0), (5, 0.1), (5, 3.0), (7, 0.1), (7, 3.0)]


def test_blur_against_float64_and_torch():
    import torch
    for t, (rng, img) in enumerate(cases(200, 7)):
        k, sigma = BLURS[t % 6] if t < 60 else (int(rng.choice([3, 5, 7])), float(rng.uniform(0.1, 3.0)))
        H, W = img.shape[:2]
        if min(H, W) <= k // 2:
            continue  # reflect padding needs more pixels than the pad
        w = A.gaussian_kernel1d(k, sigma)
        assert w.dtype == np.float32 and w.shape == (k,) and abs(float(w.sum()) - 1) < 1e-6
        got = R.gauss_blur(img, k, w)
        exact = R.gauss_blur(img, k, w, dtype=np.float64)
        tie_rule(got, exact, ("f64", k, sigma))
        assert np.allclose(P.torch_blur(img, k, w, torch.float64), exact, rtol=0, atol=1e-9)
        tie_rule(P.torch_blur(img, k, w), exact, ("torch", k, sigma))
    # 3x5 is the smallest image k = 3 pads; sigma 0.1 is the identity
    img = rand_image(np.random.default_rng(0), 3, 5)
    assert np.array_equal(R.gauss_blur(img, 3, A.gaussian_kernel1d(3, 0.1)), img)


def test_interpreter_all_colour_orders_and_erase():
    rng = np.random.default_rng(8)
    img = rand_image(rng, 20, 28)
    fac = {R.BRIGHTNESS: 1.3, R.CONTRAST: 0.7, R.SATURATION: 1.2, R.HUE: -0.07}
    for order in itertools.permutations(fac):
        ops = np.zeros(R.MAX_OPS, np.int32)
        args = np.zeros((R.MAX_OPS, R.NARGS))
        ops[:4] = order
        args[:4, 0] = [fac[o] for o in order]
        ops[4], args[4, :4] = R.ERASE, [0, 20, 5, 8]  # touches the top and the right border
        u8, f32 = R.run_program(img, ops, args)
        pu8, pf32 = P.run_program(img, ops, args)
        assert np.array_equal(u8, pu8) and np.array_equal(f32, pf32), order
        assert not f32[:, 0:5, 20:28].any() and f32.dtype == np.float32
    u8, f32 = R.run_program(img, np.zeros(R.MAX_OPS, np.int32), np.zeros((R.MAX_OPS, R.NARGS)))
    assert np.array_equal(u8, img)
    assert np.array_equal(f32, ((img.astype(np.float32) / np.float32(255) - np.float32(0.5)) / np.float32(0.5)).transpose(2, 0, 1))


def test_golden_file_is_what_the_restatement_makes():
    """tests/golden/augment_golden.npz (tools/gen_augment_golden.py: Pillow's and torch's outputs, recorded)."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "augment_golden.npz"))
    assert len(g["images"]) >= 12 and set(int(o) for o in g["ops"].ravel()) == set(range(12))  # every opcode
    u8, f32 = R.run_batch(g["images"], g["ops"], g["args"])
    assert np.array_equal(u8, g["out_u8"]) and np.array_equal(f32, g["out_f32"])


# ---- the sampler ----

def programs(t, B, seed):
    ops, args = t.sample(B, np.random.default_rng(seed))
    assert ops.shape == (B, A.MAX_OPS) and ops.dtype == np.int32
    assert args.shape == (B, A.MAX_OPS, A.NARGS) and args.dtype == np.float64 and np.isfinite(args).all()
    return ops, args


@pytest.mark.parametrize("strength", ["light", "normal", "strong", "heavy"])
def test_sampler_presets(strength):
    S, B = 112, 400
    t = A.get_train_transforms(S, augment_strength=strength)
    ops, args = programs(t, B, 11)
    ops2, args2 = programs(t, B, 11)
    assert np.array_equal(ops, ops2) and np.array_equal(args, args2)  # reproducible from a seed
    ops3, _ = programs(t, B, 12)
    assert not np.array_equal(ops, ops3)
    jit = {"light": (0.1, 0.1, 0.05, 0.02), "normal": (0.2, 0.2, 0.1, 0.05), "strong": (0.3, 0.3, 0.2, 0.1),
           "heavy": (0.4, 0.4, 0.3, 0.1)}[strength]
    orders = set()
    flips = 0
    for b in range(B):
        row = [int(o) for o in ops[b] if o != A.OP_NOP]
        assert row == [int(o) for o in ops[b, :len(row)]]  # no holes
        colour = [o for o in row if o in (A.OP_BRIGHTNESS, A.OP_CONTRAST, A.OP_SATURATION, A.OP_HUE)]
        assert sorted(colour) == [A.OP_BRIGHTNESS, A.OP_CONTRAST, A.OP_SATURATION, A.OP_HUE]
        orders.add(tuple(colour))
        flips += A.OP_FLIP_H in row
        assert row.count(A.OP_ERASE) <= 1 and (A.OP_ERASE not in row or row[-1] == A.OP_ERASE)
        for k, o in enumerate(row):
            a = args[b, k]
            if o in (A.OP_BRIGHTNESS, A.OP_CONTRAST, A.OP_SATURATION):
                x = jit[o - A.OP_BRIGHTNESS]
                assert max(0.0, 1 - x) <= a[0] <= 1 + x
            elif o == A.OP_HUE:
                assert -jit[3] <= a[0] <= jit[3]
            elif o in (A.OP_CROP_RESIZE, A.OP_ERASE):
                i, j, h, w = a[:4]
                assert all(float(v).is_integer() for v in a[:4])
                assert h >= 1 and w >= 1 and i >= 0 and j >= 0 and i + h <= S and j + w <= S
                if o == A.OP_ERASE:
                    assert h < S and w < S
            elif o == A.OP_GAUSS_BLUR:
                k_ = int(a[0])
                assert k_ == {"strong": 3, "heavy": 5}[strength] and abs(a[1:1 + k_].sum() - 1) < 1e-6
                assert np.array_equal(a[1:1 + k_], a[1:1 + k_].astype(np.float32)) and not a[1 + k_:].any()
    assert len(orders) == 24  # every permutation of the four colour ops turns up in 400 draws
    assert 0.35 * B < flips < 0.65 * B
    counts = {"light": (4, 5), "normal": (5, 6), "strong": (7, 10), "heavy": (8, 12)}[strength]
    n = (ops != 0).sum(1)
    assert n.min() >= counts[0] and n.max() <= counts[1] and n.max() <= A.MAX_OPS


def test_sampler_affine_translations_are_integers_and_rotation_range():
    S = 112
    t = A.DeviceTransform(S, [("affine", 0, (0.1, 0.1), (1.0, 1.0), 0)])  # translation only
    _, args = programs(t, 200, 3)
    tx, ty = -args[:, 0, 2], -args[:, 0, 5]  # m = [1, 0, -tx, 0, 1, -ty]
    assert np.array_equal(tx, np.rint(tx)) and np.array_equal(ty, np.rint(ty))
    assert np.abs(tx).max() <= round(0.1 * S) and np.abs(ty).max() <= round(0.1 * S) and len(set(tx)) > 5
    t = A.DeviceTransform(S, [("rotation", 10)])
    _, args = programs(t, 200, 4)
    ang = np.degrees(np.arctan2(args[:, 0, 1], args[:, 0, 0]))  # m[0] = cos, m[1] = sin(-angle)
    assert np.abs(ang).max() <= 10 + 1e-9 and ang.min() < -5 and ang.max() > 5


def test_sampler_facenet_and_val_and_perspective():
    ops, _ = programs(A.get_val_transforms(112), 5, 0)
    assert not ops.any()
    ops, _ = programs(A.facenet_train_transforms(160), 100, 0)
    assert A.OP_HUE not in ops and A.OP_AFFINE_NEAREST not in ops and (ops == A.OP_SATURATION).sum() == 100
    ops, _ = programs(A.facenet_train_transforms(160, online=True), 100, 0)
    last = [[int(o) for o in r if o][-1] for r in ops]
    assert last == [A.OP_AFFINE_NEAREST] * 100  # the rotation follows the jitter there
    t = A.DeviceTransform(112, [("perspective", 0.2, 1.0)])
    ops, args = programs(t, 50, 0)
    assert (ops[:, 0] == A.OP_PERSPECTIVE_BILINEAR).all()
    # the coefficients send each end point to its start point (f32-rounded coefficients: to 1e-2 of a pixel)
    start, end = [[0, 0], [111, 0], [111, 111], [0, 111]], [[7, 3], [104, 9], [101, 108], [11, 100]]
    a = A.perspective_coeffs(start, end)
    for (sx, sy), (ex, ey) in zip(start, end):
        den = a[6] * ex + a[7] * ey + 1
        assert abs((a[0] * ex + a[1] * ey + a[2]) / den - sx) < 1e-2 and abs((a[3] * ex + a[4] * ey + a[5]) / den - sy) < 1e-2


def test_sampled_presets_run_like_pillow():
    """A few sampled programs of every preset through the restatement and through Pillow / torch: equal, the blur's
    tie rule aside (there the two may differ by 1 where the float64 sum is within 1e-3 of a half-integer)."""
    rng = np.random.default_rng(21)
    for strength in ("light", "normal", "strong", "heavy"):
        S = 28
        t = A.get_train_transforms(S, augment_strength=strength)
        ops, args = t.sample(6, np.random.default_rng(5))
        for b in range(6):
            img = rand_image(rng, S, S)
            u8, f32 = R.run_program(img, ops[b], args[b])
            pu8, pf32 = P.run_program(img, ops[b], args[b])
            if strength in ("strong", "heavy"):
                d = np.abs(u8.astype(int) - pu8.astype(int))
                assert d.max() <= 1 and (d != 0).mean() < 0.01, (strength, b, d.max(), (d != 0).mean())
            else:
                assert np.array_equal(u8, pu8) and np.array_equal(f32, pf32), (strength, b)
