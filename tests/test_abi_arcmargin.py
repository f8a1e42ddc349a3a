"""The fr_arcmargin_* entry points at the C-ABI boundary, without a GPU: declared, exported, bound, and every
unsupported argument refused with FR_ERR_ARG and a message naming the entry point before any HIP call (the pointers
below are host memory and are never dereferenced).  Also the module's constructor and state_dict contract."""
import ctypes
import math

import pytest

from facerecognition_amd import _native as N

NEW = {"fr_arcmargin_workspace": 3, "fr_arcmargin_forward": 20, "fr_arcmargin_backward": 22}
INF, NAN = float("inf"), float("nan")


def _p():
    buf = (ctypes.c_uint64 * 64)()
    return buf, ctypes.addressof(buf)


def _other_message(L):
    L.fr_op_avgpool(None, 1, 1, 1, 8, None, 0, None)  # leaves another entry point's message behind


def _ids(kw):
    return ",".join(f"{k}={v}" for k, v in kw.items())


def test_arcmargin_functions_are_declared_exported_and_bound():
    L = N.lib()
    for name, nargs in NEW.items():
        assert name in N.header_functions(), name
        assert hasattr(L, name) and name in N._SIGS, name
        assert len(N._SIGS[name][1]) == nargs, name
    assert N._SIGS["fr_arcmargin_workspace"][0] is ctypes.c_size_t
    assert L.fr_abi_version() == 1  # additive change


SHAPE_BAD = [dict(B=0), dict(B=-3), dict(C=1), dict(C=0), dict(C=-2), dict(D=0), dict(D=2), dict(D=-4), dict(D=6),
             dict(D=510), dict(B=2 ** 21, C=2 ** 20), dict(C=2 ** 30, D=2048), dict(B=2 ** 30, D=2048, C=2)]
SCALAR_BAD = [dict(scale=0.0), dict(scale=-64.0), dict(scale=INF), dict(scale=NAN), dict(margin=-0.1),
              dict(margin=math.pi), dict(margin=4.0), dict(margin=NAN), dict(lam=-0.01), dict(lam=1.01), dict(lam=NAN),
              dict(ls=-0.1), dict(ls=1.0), dict(ls=NAN)]
COMMON_BAD = SHAPE_BAD + SCALAR_BAD + [dict(E=None), dict(W=None), dict(label=None), dict(inv_e=None),
                                       dict(inv_w=None), dict(ws=None), dict(ws_bytes=8)]


def _args(kw):
    _, p = _p()
    a = dict(B=70, C=333, D=128, lam=0.3, scale=64.0, margin=0.5, easy=0, ls=0.1, E=p, W=p, label=p, label_b=p, loss=p,
             lse=p, inv_e=p, inv_w=p, logits=None, u=p, dlogits=None, dE=p, dW=p, ws=p, ws_bytes=1 << 50)
    a.update(kw)
    return a


@pytest.mark.parametrize("kw", COMMON_BAD + [dict(loss=None), dict(lse=None)], ids=_ids)
def test_forward_rejects_unsupported_arguments(kw):
    L = N.lib()
    a = _args(kw)
    _other_message(L)
    rc = L.fr_arcmargin_forward(a["E"], a["B"], a["D"], a["W"], a["C"], a["label"], a["label_b"], a["lam"], a["scale"],
                                a["margin"], a["easy"], a["ls"], a["loss"], a["lse"], a["inv_e"], a["inv_w"],
                                a["logits"], a["ws"], a["ws_bytes"], None)
    assert rc == -1 and b"fr_arcmargin_forward" in L.fr_last_error(), (kw, rc, L.fr_last_error())


BWD_BAD = COMMON_BAD + [dict(u=None), dict(dlogits=1), dict(dE=None, dW=None), dict(lse=None)]


@pytest.mark.parametrize("kw", BWD_BAD, ids=_ids)
def test_backward_rejects_unsupported_arguments(kw):
    L = N.lib()
    a = _args(kw)
    if a["dlogits"] == 1:  # both sources given
        a["dlogits"] = a["E"]
    _other_message(L)
    rc = L.fr_arcmargin_backward(a["E"], a["B"], a["D"], a["W"], a["C"], a["label"], a["label_b"], a["lam"],
                                 a["scale"], a["margin"], a["easy"], a["ls"], a["lse"], a["inv_e"], a["inv_w"], a["u"],
                                 a["dlogits"], a["dE"], a["dW"], a["ws"], a["ws_bytes"], None)
    assert rc == -1 and b"fr_arcmargin_backward" in L.fr_last_error(), (kw, rc, L.fr_last_error())


def test_workspace_is_no_logits_matrix():
    L = N.lib()
    B, C, D = 256, 1_000_000, 512
    ws = L.fr_arcmargin_workspace(B, C, D)
    assert 0 < ws < B * C * 4 // 16  # the "no logits matrix" condition
    for b, c, d in ((1, 2, 16), (70, 333, 128), (130, 4167, 512)):
        w = L.fr_arcmargin_workspace(b, c, d)
        assert w >= b * d * 4 and w % 4 == 0
    for kw in SHAPE_BAD:
        a = dict(B=70, C=333, D=128)
        a.update(kw)
        _other_message(L)
        assert L.fr_arcmargin_workspace(a["B"], a["C"], a["D"]) == 0
        assert b"fr_arcmargin_workspace" in L.fr_last_error(), kw


def test_module_constructor_and_state_dict():
    import torch

    import facerecognition_amd as fra
    from facerecognition_amd.arcmargin import ArcMarginProduct

    assert fra.ArcMarginProduct is ArcMarginProduct and callable(fra.arcface_loss) and callable(fra.class_accuracy)
    m = ArcMarginProduct(512, 9343)
    assert (m.in_features, m.out_features, m.scale, m.margin, m.easy_margin) == (512, 9343, 64.0, 0.5, False)
    assert m.cos_m == math.cos(0.5) and m.sin_m == math.sin(0.5)
    assert m.th == math.cos(math.pi - 0.5) and m.mm == math.sin(math.pi - 0.5) * 0.5
    assert list(m.state_dict().keys()) == ["weight"] and m.weight.shape == (9343, 512)
    bound = math.sqrt(6.0 / (512 + 9343))  # Xavier-uniform
    w0 = m.weight.detach()
    assert float(w0.abs().max()) <= bound and float(w0.std()) > 0.5 * bound
    w = torch.randn(9343, 512)
    m.load_state_dict({"weight": w})
    assert torch.equal(m.weight.detach(), w)
    m2 = ArcMarginProduct(16, 11, scale=30.0, margin=0.35, easy_margin=True)
    assert (m2.scale, m2.margin, m2.easy_margin) == (30.0, 0.35, True)
    with pytest.raises(RuntimeError):  # no CPU fallback
        m2(torch.randn(4, 16), torch.zeros(4, dtype=torch.long))
