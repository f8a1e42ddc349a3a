"""fr_augment on the device against tests/augment_ref.py, exactly (both outputs, array_equal), and against Pillow
directly for every op the CPU test (test_augment_ref.py) shows exact: all of them but the blur, which is torchvision's
f32 convolution and is held to the tie rule against torch (equal wherever the float64 sum over the same taps is farther
than 1e-3 from a half-integer, within 1 elsewhere; the derivation is in test_augment_ref.py)."""
import functools
import itertools
import os

import numpy as np
import pytest

from facerecognition_amd import augment as A
from tests import augment_pil as P
from tests import augment_ref as R
from tests.augment_pil import rand_image, tie_rule

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 5), (20, 28), (112, 112), (160, 160)]  # (H, W); 160 x 160 is the LDS limit


@pytest.fixture(scope="module")
def dev(gpu):
    return gpu


def run_device(dev, images, ops, args):
    import torch
    x = torch.from_numpy(np.ascontiguousarray(images)).to(dev)
    f32, u8 = A.augment(x, ops, args, return_u8=True)
    torch.cuda.synchronize()
    return f32.cpu().numpy(), u8.cpu().numpy()


def pack(programs):
    ops = np.zeros((len(programs), R.MAX_OPS), np.int32)
    args = np.zeros((len(programs), R.MAX_OPS, R.NARGS), np.float64)
    for b, prog in enumerate(programs):
        for k, (op, *v) in enumerate(prog):
            ops[b, k] = op
            args[b, k, :len(v)] = v
    return ops, args


def edge_programs(H, W):
    """One-op programs with the edge values of every op, for an H x W image: [(name, program, pillow-exact)]."""
    out = []
    for angle in (0.0, 90.0, 180.0, 270.0, 1e-9, -1e-9, 20.0, -20.0):
        out.append((f"rotate {angle}", [(R.AFFINE_NEAREST, *A.rotation_matrix(angle, W, H))], True))
    c = (W * 0.5, H * 0.5)
    out.append(("affine", [(R.AFFINE_NEAREST, *A.inverse_affine_matrix(c, 12.0, (2, -1), 1.1, (6.0, 0.0)))], True))
    m = A.inverse_affine_matrix(c, 0.0, (W, 0), 1.0, (0.0, 0.0))
    m[1] = 1e-12  # not Pillow's pure-scale routine
    out.append(("affine out", [(R.AFFINE_NEAREST, *m)], True))
    out.append(("perspective identity", [(R.PERSPECTIVE_BILINEAR, 1, 0, 0, 0, 1, 0, 0, 0)], True))
    out.append(("perspective", [(R.PERSPECTIVE_BILINEAR, 1.05, 0.04, -1.5, -0.03, 0.95, 0.8, 2e-4, -3e-4)], True))
    out.append(("crop full", [(R.CROP_RESIZE, 0, 0, H, W)], True))
    out.append(("crop 1x1", [(R.CROP_RESIZE, H - 1, W - 1, 1, 1)], True))
    out.append(("crop", [(R.CROP_RESIZE, H // 5, W // 7, H - H // 3, W - W // 4)], True))
    out.append(("crop rows", [(R.CROP_RESIZE, H // 4, 0, H - H // 2, W)], True))
    out.append(("crop columns", [(R.CROP_RESIZE, 0, W // 4, H, W - W // 2)], True))
    for f in (0.0, 1.0, 0.6, 1.4):
        for op in (R.BRIGHTNESS, R.CONTRAST, R.SATURATION):
            out.append((f"enhance {op} {f}", [(op, f)], True))
    for f in (0.0, 0.5, -0.5, 0.37, -0.01):  # 0.37 and the negatives wrap the hue byte for part of the pixels
        out.append((f"hue {f}", [(R.HUE, f)], True))
    out.append(("gray", [(R.GRAYSCALE,)], True))
    out.append(("flip", [(R.FLIP_H,)], True))
    for k, sigmas in ((3, (0.1, 2.0)), (5, (0.1, 3.0)), (7, (0.1, 3.0))):
        if k // 2 < min(H, W):
            for s in sigmas:
                out.append((f"blur {k} {s}", [(R.GAUSS_BLUR, k, *A.gaussian_kernel1d(k, s))], False))
    out.append(("no erase", [], True))
    eh, ew = max(H // 3, 1), max(W // 3, 1)
    for name, box in (("top left", (0, 0, eh, ew)), ("bottom right", (H - eh, W - ew, eh, ew)),
                      ("top right", (0, W - ew, eh, ew)), ("bottom left", (H - eh, 0, eh, ew)), ("all", (0, 0, H, W))):
        out.append((f"erase {name}", [(R.FLIP_H,), (R.ERASE, *box)], True))
    return out


@functools.lru_cache(maxsize=None)
def edge_case(H, W):
    """Images, programs and the restatement's outputs for one size; computed once and shared."""
    rng = np.random.default_rng(H * 1000 + W)
    progs = edge_programs(H, W)
    images = np.stack([rand_image(rng, H, W) for _ in progs])
    const = [i for i, (n, _, _) in enumerate(progs) if n.startswith(f"enhance {R.CONTRAST}")]
    images[const[-1]] = 77  # contrast on a constant image
    ops, args = pack([p for _, p, _ in progs])
    u8, f32 = R.run_batch(images, ops, args)
    return progs, images, ops, args, u8, f32


@pytest.mark.parametrize("H,W", SIZES, ids=lambda v: str(v))
def test_every_op_and_edge_value(dev, H, W):
    progs, images, ops, args, want_u8, want_f32 = edge_case(H, W)
    f32, u8 = run_device(dev, images, ops, args)
    for b, (name, _, _) in enumerate(progs):
        assert np.array_equal(u8[b], want_u8[b]), (name, H, W, int(np.abs(u8[b].astype(int) - want_u8[b]).max()))
        assert np.array_equal(f32[b].view(np.uint32), want_f32[b].view(np.uint32)), (name, H, W)
    for b, (name, prog, exact) in enumerate(progs):  # and Pillow directly
        if exact:
            pu8, pf32 = P.run_program(images[b], ops[b], args[b])
            assert np.array_equal(u8[b], pu8) and np.array_equal(f32[b], pf32), (name, H, W)
        else:
            k, w = args[b, 0, 0], args[b, 0, 1:8]
            sums = R.gauss_blur(images[b], k, w, dtype=np.float64)
            tie_rule(u8[b], sums, name)
            tie_rule(P.torch_blur(images[b], k, w), sums, name + " (torch)")
    name_of = {n: b for b, (n, _, _) in enumerate(progs)}
    assert not u8[name_of["affine out"]].any()
    assert np.array_equal(u8[name_of["perspective identity"]], images[name_of["perspective identity"]])
    assert np.array_equal(u8[name_of["crop full"]], images[name_of["crop full"]])
    assert not f32[name_of["erase all"]].any() and u8[name_of["erase all"]].any() == images[name_of["erase all"]].any()


@pytest.mark.parametrize("B", [1, 3, 300])
def test_batches(dev, B):
    """B = 300 is more workgroups than CUs; every image runs a program of its own."""
    H, W = 20, 28
    progs, _, ops0, args0, _, _ = edge_case(H, W)
    rng = np.random.default_rng(B)
    images = np.stack([rand_image(rng, H, W) for _ in range(B)])
    pick = [(7 * b + 3) % len(progs) for b in range(B)]
    ops, args = ops0[pick], args0[pick]
    want_u8, want_f32 = R.run_batch(images, ops, args)
    f32, u8 = run_device(dev, images, ops, args)
    assert np.array_equal(u8, want_u8) and np.array_equal(f32.view(np.uint32), want_f32.view(np.uint32))


def test_empty_program_normalises_only(dev):
    import torch
    for H, W in SIZES:
        rng = np.random.default_rng(H)
        images = np.stack([rand_image(rng, H, W) for _ in range(3)])
        images[0].reshape(-1)[:256] = np.arange(256)[:images[0].size]  # every byte value where there is room
        ops, args = pack([[]] * 3)
        f32, u8 = run_device(dev, images, ops, args)
        want = (torch.from_numpy(images).permute(0, 3, 1, 2).to(torch.float32) / 255 - 0.5) / 0.5
        assert np.array_equal(u8, images) and np.array_equal(f32, want.numpy()), (H, W)
        # n_ops = 0 and one output alone
        x = torch.from_numpy(images).to(dev)
        only = A.augment(x, np.zeros((3, 0), np.int32), np.zeros((3, 0, 8)))
        assert np.array_equal(only.cpu().numpy(), want.numpy())
        only8 = A.augment(x, ops, args, return_u8=True, return_f32=False)
        assert only8.dtype == torch.uint8 and np.array_equal(only8.cpu().numpy(), images)


def test_golden_file(dev):
    """The recorded Pillow / torch outputs of tests/golden/augment_golden.npz, every opcode among them."""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "augment_golden.npz"))
    f32, u8 = run_device(dev, g["images"], g["ops"], g["args"])
    assert np.array_equal(u8, g["out_u8"]) and np.array_equal(f32, g["out_f32"])


def test_all_24_orders_of_the_colour_ops(dev):
    H, W = 20, 28
    img = rand_image(np.random.default_rng(24), H, W)
    fac = {R.BRIGHTNESS: 1.3, R.CONTRAST: 0.7, R.SATURATION: 1.2, R.HUE: -0.07}
    progs = [[(o, fac[o]) for o in order] for order in itertools.permutations(fac)]
    ops, args = pack(progs)
    images = np.stack([img] * 24)
    f32, u8 = run_device(dev, images, ops, args)
    want_u8, want_f32 = R.run_batch(images, ops, args)
    assert np.array_equal(u8, want_u8) and np.array_equal(f32, want_f32)
    for b in range(24):
        pu8, pf32 = P.run_program(img, ops[b], args[b])
        assert np.array_equal(u8[b], pu8) and np.array_equal(f32[b], pf32), progs[b]
    assert len({u8[b].tobytes() for b in range(24)}) > 12  # the order matters


def without(ops, args, drop):
    o, a = ops.copy(), args.copy()
    for d in drop:
        a[o == d] = 0
        o[o == d] = R.NOP
    return o, a


@pytest.mark.parametrize("preset", ["light", "normal", "strong", "heavy", "facenet", "facenet_online"])
def test_presets_against_the_pillow_pipeline(dev, preset):
    """64 sampled images per preset: the device equals the restatement exactly and the Pillow / torch pipeline run with
    the same parameters exactly; where the last u8 op is the blur ('strong', 'heavy'), everything before it is exact
    and the blur itself is held to the tie rule."""
    import torch
    B = 64
    S = 160 if preset.startswith("facenet") else 112
    t = A.facenet_train_transforms(S, online=preset.endswith("online")) if preset.startswith("facenet") else \
        A.get_train_transforms(S, augment_strength=preset)
    rng = np.random.default_rng(64)
    images = np.stack([rand_image(rng, S, S) for _ in range(B)])
    ops, args = t.sample(B, np.random.default_rng(2024))
    x = torch.from_numpy(images).to(dev)
    f32, u8 = t.apply(x, ops, args, return_u8=True)
    f32, u8 = f32.cpu().numpy(), u8.cpu().numpy()
    want_u8, want_f32 = R.run_batch(images, ops, args)
    assert np.array_equal(u8, want_u8) and np.array_equal(f32.view(np.uint32), want_f32.view(np.uint32))
    blurred = preset in ("strong", "heavy")
    ops_nb, args_nb = without(ops, args, [R.GAUSS_BLUR, R.ERASE]) if blurred else (ops, args)
    for b in range(B):
        pu8, pf32 = P.run_program(images[b], ops_nb[b], args_nb[b])
        if not blurred:
            assert np.array_equal(u8[b], pu8) and np.array_equal(f32[b], pf32), (preset, b)
            continue
        pre, _ = R.run_program(images[b], ops_nb[b], args_nb[b])
        assert np.array_equal(pre, pu8), (preset, b)  # up to the blur: exact
        k = int(np.flatnonzero(ops[b] == R.GAUSS_BLUR)[0])
        sums = R.gauss_blur(pu8, args[b, k, 0], args[b, k, 1:8], dtype=np.float64)
        tie_rule(u8[b], sums, (preset, b))
        tie_rule(P.torch_blur(pu8, args[b, k, 0], args[b, k, 1:8]), sums, (preset, b, "torch"))
    # the same seed gives the same output, bit for bit
    a1 = t(x, generator=np.random.default_rng(5)).cpu().numpy()
    a2 = t(x, generator=np.random.default_rng(5)).cpu().numpy()
    a3 = t(x, generator=np.random.default_rng(6)).cpu().numpy()
    assert np.array_equal(a1.view(np.uint32), a2.view(np.uint32)) and not np.array_equal(a1, a3)


def test_leading_resize_and_feeding_the_trunk(dev):
    """A crop of another size goes through align.resize_u8 first; the f32 output is what FRModel.features takes."""
    import torch

    from facerecognition_amd.align import resize_u8
    from facerecognition_amd.model import FRModel

    rng = np.random.default_rng(9)
    x = torch.from_numpy(np.stack([rand_image(rng, 128, 128) for _ in range(2)])).to(dev)
    val = A.get_val_transforms(112)
    out = val(x)
    assert out.shape == (2, 3, 112, 112) and out.dtype == torch.float32 and out.is_cuda
    # on the CPU: torch divides by a scalar on the device by multiplying with its reciprocal
    want = (resize_u8(x, 112, 112).cpu().permute(0, 3, 1, 2).to(torch.float32) / 255 - 0.5) / 0.5
    assert torch.equal(out.cpu(), want)
    model = FRModel.synthetic("resnet50_arcface")
    feat = model.features(A.get_train_transforms(112)(x, generator=np.random.default_rng(1)))
    assert feat.shape == (2, model.feature_dim) and feat.dtype == torch.float32 and bool(torch.isfinite(feat).all())


def test_mixup_on_the_device(dev):
    import torch
    x = torch.randn(8, 3, 4, 4, device=dev)
    y = torch.arange(8, device=dev)
    mixed, ya, yb, lam = A.mixup_data(x, y, 0.2, np.random.default_rng(0))
    g = np.random.default_rng(0)
    assert lam == float(g.beta(0.2, 0.2))
    idx = torch.from_numpy(g.permutation(8)).to(dev)
    assert mixed.is_cuda and torch.equal(mixed, lam * x + (1 - lam) * x[idx]) and torch.equal(yb, y[idx]) and ya is y
