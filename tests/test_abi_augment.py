"""The fr_augment entry points at the C-ABI boundary, without a GPU: declared, exported, bound, and every unsupported
argument refused with FR_ERR_ARG and a message naming the entry point before any HIP call (the device pointers below
are host memory and are never dereferenced; ops and args are host arrays by contract and are read).  Also the Python
face's names, defaults and its refusal of CPU tensors."""
import ctypes
import inspect
import re

import numpy as np
import pytest

from facerecognition_amd import _native as N
from facerecognition_amd import augment as A

NEW = {"fr_augment_workspace": 2, "fr_augment": 12}
INF, NAN = float("inf"), float("nan")


def _p():
    buf = (ctypes.c_uint64 * 64)()
    return buf, ctypes.addressof(buf)


def _other_message(L):
    L.fr_op_avgpool(None, 1, 1, 1, 8, None, 0, None)  # leaves another entry point's message behind


def _ids(kw):
    return ",".join(f"{k}={v}" for k, v in kw.items())


def test_augment_functions_are_declared_exported_and_bound():
    L = N.lib()
    for name, nargs in NEW.items():
        assert name in N.header_functions(), name
        assert hasattr(L, name) and name in N._SIGS, name
        assert len(N._SIGS[name][1]) == nargs, name
    assert N._SIGS["fr_augment_workspace"][0] is ctypes.c_size_t
    assert L.fr_abi_version() == 1  # additive change
    # the header's prototype has as many parameters as the binding
    src = open(N.HEADER_PATH).read()
    proto = re.sub(r"/\*.*?\*/", "", src[src.index("int fr_augment("):], flags=re.S)
    proto = proto[:proto.index(");")]
    assert proto.count(",") + 1 == NEW["fr_augment"]
    # the opcodes of the Python face are the header's
    for name in ("NOP", "FLIP_H", "AFFINE_NEAREST", "PERSPECTIVE_BILINEAR", "CROP_RESIZE", "BRIGHTNESS", "CONTRAST",
                 "SATURATION", "HUE", "GRAYSCALE", "GAUSS_BLUR", "ERASE"):
        assert f"#define FR_AUG_{name} {getattr(A, 'OP_' + name)}\n" in src, name
    assert f"#define FR_AUGMENT_MAX_OPS {A.MAX_OPS}\n" in src and f"#define FR_AUGMENT_ARGS {A.NARGS}\n" in src


def prog(*ops):
    """One row: (opcode, args...) tuples."""
    o = np.zeros((1, 16), np.int32)
    a = np.zeros((1, 16, 8), np.float64)
    for k, (op, *v) in enumerate(ops):
        o[0, k] = op
        a[0, k, :len(v)] = v
    return o, a


W3 = (0.25, 0.5, 0.25)
BAD_PROGRAMS = {
    "unknown_opcode": prog((12,)),
    "negative_opcode": prog((-1,)),
    "nan_argument": prog((A.OP_BRIGHTNESS, NAN)),
    "inf_argument": prog((A.OP_AFFINE_NEAREST, 1, 0, INF, 0, 1, 0)),
    "inf_in_an_unused_slot": prog((A.OP_FLIP_H, 0, 0, 0, 0, 0, 0, 0, INF)),
    "nan_under_a_nop": prog((A.OP_NOP, NAN)),
    "blur_k_4": prog((A.OP_GAUSS_BLUR, 4) + W3),
    "blur_k_9": prog((A.OP_GAUSS_BLUR, 9) + W3),
    "blur_k_1": prog((A.OP_GAUSS_BLUR, 1) + W3),
    "blur_k_3.5": prog((A.OP_GAUSS_BLUR, 3.5) + W3),
    "crop_empty": prog((A.OP_CROP_RESIZE, 0, 0, 0, 5)),
    "crop_past_the_bottom": prog((A.OP_CROP_RESIZE, 10, 0, 11, 5)),
    "crop_past_the_right": prog((A.OP_CROP_RESIZE, 0, 20, 5, 9)),
    "crop_negative_corner": prog((A.OP_CROP_RESIZE, -1, 0, 5, 5)),
    "crop_fractional": prog((A.OP_CROP_RESIZE, 0.5, 0, 5, 5)),
    "crop_huge": prog((A.OP_CROP_RESIZE, 0, 0, 2.0 ** 40, 5)),
    "erase_empty": prog((A.OP_ERASE, 0, 0, 5, 0)),
    "erase_outside": prog((A.OP_ERASE, 16, 0, 5, 5)),
    "erase_not_last": prog((A.OP_ERASE, 0, 0, 5, 5), (A.OP_FLIP_H,)),
    "erase_twice": prog((A.OP_ERASE, 0, 0, 5, 5), (A.OP_ERASE, 1, 1, 2, 2)),
    "erase_then_nop_then_op": prog((A.OP_ERASE, 0, 0, 5, 5), (A.OP_NOP,), (A.OP_GRAYSCALE,)),
    "affine_far_away": prog((A.OP_AFFINE_NEAREST, 1, 0, 40000, 0, 1, 0)),
    "affine_huge_scale": prog((A.OP_AFFINE_NEAREST, 1e6, 0, 0, 0, 1, 0)),
    "hue_out_of_range": prog((A.OP_HUE, 0.6)),
    "negative_factor": prog((A.OP_CONTRAST, -0.1)),
}


@pytest.mark.parametrize("name", list(BAD_PROGRAMS))
def test_augment_rejects_unsupported_programs(name):
    L = N.lib()
    _, p = _p()
    ops, args = BAD_PROGRAMS[name]
    ops = np.concatenate([prog()[0], ops])  # the bad row is the second image's
    args = np.concatenate([prog()[1], args])
    _other_message(L)
    rc = L.fr_augment(p, 2, 20, 28, ops.ctypes.data, args.ctypes.data, 16, p, p, p, 1 << 30, None)
    assert rc == -1 and b"fr_augment" in L.fr_last_error(), (name, rc, L.fr_last_error())
    assert b"image 1" in L.fr_last_error(), L.fr_last_error()


ARG_BAD = [dict(B=0), dict(B=-3), dict(B=2 ** 24 + 1), dict(H=0), dict(W=0), dict(H=-1), dict(H=161, W=160),
           dict(H=160, W=161), dict(H=1, W=25600), dict(H=2 ** 20, W=2 ** 20), dict(out_f32=None, out_u8=None),
           dict(inp=None), dict(ops=None), dict(args=None), dict(ws=None), dict(n_ops=17), dict(n_ops=-1),
           dict(ws_bytes=0), dict(ws_bytes=100)]


@pytest.mark.parametrize("kw", ARG_BAD, ids=_ids)
def test_augment_rejects_unsupported_arguments(kw):
    L = N.lib()
    _, p = _p()
    a = dict(B=1, H=20, W=28, n_ops=16, inp=p, ops=True, args=True, out_f32=p, out_u8=p, ws=p, ws_bytes=1 << 30)
    a.update(kw)
    ops, args = prog((A.OP_FLIP_H,))
    _other_message(L)
    rc = L.fr_augment(a["inp"], a["B"], a["H"], a["W"], ops.ctypes.data if a["ops"] else None,
                      args.ctypes.data if a["args"] else None, a["n_ops"], a["out_f32"], a["out_u8"], a["ws"],
                      a["ws_bytes"], None)
    assert rc == -1 and b"fr_augment" in L.fr_last_error(), (kw, rc, L.fr_last_error())


def test_workspace_sizes():
    L = N.lib()
    for B, n in ((1, 16), (3, 16), (300, 16), (256, 4), (5, 0)):
        ws = L.fr_augment_workspace(B, n)
        assert ws >= B * n * (8 * 8 + 4) + 1024 and ws % 8 == 0
    for B, n in ((0, 16), (-1, 16), (1, 17), (1, -1), (2 ** 24 + 1, 1)):
        _other_message(L)
        assert L.fr_augment_workspace(B, n) == 0
        assert b"fr_augment_workspace" in L.fr_last_error(), (B, n)


def test_python_face_names_defaults_and_no_cpu_fallback():
    import torch

    import facerecognition_amd as fra

    names = ("get_train_transforms", "get_val_transforms", "facenet_train_transforms", "DeviceTransform", "mixup_data")
    for name in names:
        assert getattr(fra, name) is getattr(A, name)
    sig = inspect.signature(A.get_train_transforms)  # the reference's names, order and defaults
    assert [(k, v.default) for k, v in sig.parameters.items()] == \
        [("image_size", 112), ("use_albumentations", False), ("augment_strength", "normal")]
    sig = inspect.signature(A.get_val_transforms)
    assert list(sig.parameters)[0] == "image_size"
    sig = inspect.signature(A.facenet_train_transforms)
    assert [(k, v.default) for k, v in sig.parameters.items()] == [("image_size", 160), ("online", False)]
    sig = inspect.signature(A.mixup_data)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [("y", inspect.Parameter.empty), ("alpha", 0.2),
                                                                       ("generator", None)]
    assert list(inspect.signature(A.DeviceTransform.sample).parameters) == ["self", "B", "generator"]
    assert list(inspect.signature(A.DeviceTransform.apply).parameters) == ["self", "images", "ops", "args", "return_u8"]
    assert inspect.signature(A.DeviceTransform.apply).parameters["return_u8"].default is False
    assert list(inspect.signature(A.DeviceTransform.__call__).parameters) == ["self", "images", "generator"]
    with pytest.raises(NotImplementedError, match="albumentations"):
        A.get_train_transforms(112, use_albumentations=True)
    for strength in ("light", "normal", "strong", "heavy"):
        t = A.get_train_transforms(augment_strength=strength)
        assert isinstance(t, A.DeviceTransform) and t.image_size == 112
    assert A.get_val_transforms(160).steps == [] and A.facenet_train_transforms().image_size == 160
    x = torch.zeros((2, 112, 112, 3), dtype=torch.uint8)
    t = A.get_train_transforms()
    ops, args = t.sample(2, np.random.default_rng(0))
    for call in (lambda: t(x), lambda: t.apply(x, ops, args), lambda: A.augment(x, ops, args)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_mixup_data_on_the_host():
    """mixup_data is plain torch: the reference's tuple, lam from Beta(alpha, alpha), a permutation of the batch."""
    import torch
    x = torch.arange(24, dtype=torch.float32).reshape(6, 4)
    y = torch.arange(6)
    mixed, ya, yb, lam = A.mixup_data(x, y, 0.2, np.random.default_rng(3))
    g = np.random.default_rng(3)
    want_lam = float(g.beta(0.2, 0.2))
    idx = torch.from_numpy(g.permutation(6))
    assert lam == want_lam and 0.0 <= lam <= 1.0 and ya is y and torch.equal(yb, y[idx])
    assert torch.equal(mixed, lam * x + (1 - lam) * x[idx])
    mixed, ya, yb, lam = A.mixup_data(x, y, 0.0)
    assert lam == 1.0 and torch.equal(mixed, x) and sorted(yb.tolist()) == y.tolist()
