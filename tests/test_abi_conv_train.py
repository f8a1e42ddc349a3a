"""The backbone-training entry points (fr_conv_train_*, fr_bn2d_train_stats, fr_bn_act_*, fr_features_at*) at the C-ABI
boundary, without a GPU: declared, exported, bound, and every unsupported argument refused with FR_ERR_ARG and a message
naming the entry point before any HIP call (the pointers below are host memory and are never dereferenced).  Also the
modules' constructors and ResNet50Layer4's key map."""
import ctypes

import numpy as np
import pytest

from facerecognition_amd import _native as N

NEW = {"fr_conv_train_workspace": 7, "fr_conv_train_forward": 16, "fr_conv_train_backward": 16, "fr_bn2d_train_stats": 15,
       "fr_bn_act_forward": 9, "fr_bn_act_backward": 16, "fr_features_at_shape": 5, "fr_features_at": 9}
INF, NAN = float("inf"), float("nan")


def _p():
    buf = (ctypes.c_uint64 * 64)()
    return buf, ctypes.addressof(buf)


_BUF, P = _p()
_BUF2, P2 = _p()


def _other_message(L):
    L.fr_op_avgpool(None, 1, 1, 1, 8, None, 0, None)  # leaves another entry point's message behind


def _ids(kw):
    def name(v):  # the buffers' addresses differ from run to run: a test id must not
        return "P" if v is P else "P2" if v is P2 else v
    return ",".join(f"{k}={name(v)}" for k, v in kw.items())


def test_functions_are_declared_exported_and_bound():
    L = N.lib()
    for name, nargs in NEW.items():
        assert name in N.header_functions(), name
        assert hasattr(L, name) and name in N._SIGS, name
        assert len(N._SIGS[name][1]) == nargs, name
    assert N._SIGS["fr_conv_train_workspace"][0] is ctypes.c_size_t
    assert (N.FR_CONV_IN_RELU, N.FR_BN_BATCH_STATS, N.FR_BN_RELU, N.FR_CUT_LAYER4_IN) == (1, 1, 2, 0)
    assert N.FR_BN_BATCH_STATS == N.FR_HEAD_BATCH_STATS
    assert L.fr_abi_version() == 1  # additive change


CONV_SHAPE_BAD = [dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=40000), dict(Cin=0), dict(Cin=2), dict(Cin=6),
                  dict(Cin=-4), dict(Cin=1 << 19), dict(Cout=0), dict(Cout=510), dict(Cout=1 << 19), dict(k=0), dict(k=2),
                  dict(k=5), dict(k=7), dict(stride=0), dict(stride=3), dict(B=1 << 20, H=64, W=64),
                  dict(B=1 << 16, H=128, W=128, Cin=1 << 12), dict(B=1 << 16, H=128, W=128, Cout=1 << 12, k=1, stride=1)]
CONV_BAD = CONV_SHAPE_BAD + [dict(flags=2), dict(flags=-1), dict(scale=None), dict(shift=None),
                             dict(scale=None, shift=None, flags=1), dict(X=None), dict(Wt=None)]


def _conv_args(kw):
    a = dict(X=P, B=2, H=7, W=7, Cin=1024, scale=P, shift=P, flags=1, Wt=P, Cout=512, k=3, stride=2, Z=P, ws=P,
             ws_bytes=1 << 50, dZ=P, dA=P, dW=P)
    a.update(kw)
    return a


def _conv_fwd(L, a):
    return L.fr_conv_train_forward(a["X"], a["B"], a["H"], a["W"], a["Cin"], a["scale"], a["shift"], a["flags"], a["Wt"],
                                   a["Cout"], a["k"], a["stride"], a["Z"], a["ws"], a["ws_bytes"], None)


def _conv_bwd(L, a):
    return L.fr_conv_train_backward(a["X"], a["B"], a["H"], a["W"], a["Cin"], a["scale"], a["shift"], a["flags"], a["Wt"],
                                    a["Cout"], a["k"], a["stride"], a["dZ"], a["dA"], a["dW"], None)


@pytest.mark.parametrize("kw", CONV_BAD + [dict(Z=None), dict(ws=None), dict(ws_bytes=8, B=2, H=4, W=4)], ids=_ids)
def test_conv_forward_rejects_unsupported_arguments(kw):
    L = N.lib()
    _other_message(L)
    rc = _conv_fwd(L, _conv_args(kw))
    assert rc == -1 and b"fr_conv_train_forward" in L.fr_last_error(), (kw, rc, L.fr_last_error())


@pytest.mark.parametrize("kw", CONV_BAD + [dict(dZ=None), dict(dA=None, dW=None)], ids=_ids)
def test_conv_backward_rejects_unsupported_arguments(kw):
    L = N.lib()
    _other_message(L)
    rc = _conv_bwd(L, _conv_args(kw))
    assert rc == -1 and b"fr_conv_train_backward" in L.fr_last_error(), (kw, rc, L.fr_last_error())


def test_conv_workspace():
    L = N.lib()
    # a large M needs no split (16 bytes, so that 0 stays the error value); a small one holds at most 64 partials
    assert L.fr_conv_train_workspace(256, 4, 4, 512, 512, 3, 1) == 16
    for shape in ((2, 4, 4, 512, 512, 3, 1), (2, 4, 4, 2048, 512, 1, 1), (32, 7, 7, 1024, 512, 1, 1)):
        B, H, W, Cin, Cout, k, s = shape
        w = L.fr_conv_train_workspace(*shape)
        m = B * ((H + 2 * (k // 2) - k) // s + 1) * ((W + 2 * (k // 2) - k) // s + 1)
        assert w % 4 == 0 and 2 * m * Cout * 4 <= w <= 64 * m * Cout * 4, shape
    for kw in CONV_SHAPE_BAD:
        a = _conv_args(kw)
        _other_message(L)
        assert L.fr_conv_train_workspace(a["B"], a["H"], a["W"], a["Cin"], a["Cout"], a["k"], a["stride"]) == 0
        assert b"fr_conv_train_workspace" in L.fr_last_error(), kw


BN_SHAPE_BAD = [dict(M=0), dict(M=-5), dict(M=(1 << 24) + 1), dict(C=0), dict(C=2), dict(C=6), dict(C=-4),
                dict(C=(1 << 24) + 4), dict(flags=4), dict(flags=-1)]


def _bn_args(kw):
    a = dict(M=98, C=512, flags=1, eps=1e-5, momentum=0.1)
    for name in ("Z", "gamma", "beta", "rm", "rv", "mean", "rstd", "scale", "shift", "Res", "Y", "dY", "dZ", "dgamma", "dbeta"):
        a[name] = P
    a["dRes"] = P2
    a.update(kw)
    return a


@pytest.mark.parametrize("kw", BN_SHAPE_BAD + [dict(flags=2), dict(flags=3), dict(M=1), dict(eps=0.0), dict(eps=-1.0),
                                              dict(eps=INF), dict(eps=NAN), dict(momentum=-0.1), dict(momentum=1.5),
                                              dict(momentum=NAN), dict(Z=None), dict(gamma=None), dict(beta=None),
                                              dict(rm=None), dict(rv=None), dict(rm=None, flags=0), dict(mean=None),
                                              dict(rstd=None), dict(scale=None), dict(shift=None)], ids=_ids)
def test_bn_stats_rejects_unsupported_arguments(kw):
    L = N.lib()
    a = _bn_args(kw)
    _other_message(L)
    rc = L.fr_bn2d_train_stats(a["Z"], a["M"], a["C"], a["gamma"], a["beta"], a["rm"], a["rv"], a["flags"], a["eps"],
                               a["momentum"], a["mean"], a["rstd"], a["scale"], a["shift"], None)
    assert rc == -1 and b"fr_bn2d_train_stats" in L.fr_last_error(), (kw, rc, L.fr_last_error())


@pytest.mark.parametrize("kw", BN_SHAPE_BAD + [dict(flags=1), dict(flags=3), dict(Z=None), dict(scale=None),
                                              dict(shift=None), dict(Y=None)], ids=_ids)
def test_bn_act_forward_rejects_unsupported_arguments(kw):
    L = N.lib()
    a = _bn_args(dict(flags=2))
    a.update(kw)
    _other_message(L)
    rc = L.fr_bn_act_forward(a["Z"], a["M"], a["C"], a["scale"], a["shift"], a["Res"], a["flags"], a["Y"], None)
    assert rc == -1 and b"fr_bn_act_forward" in L.fr_last_error(), (kw, rc, L.fr_last_error())


@pytest.mark.parametrize("kw", BN_SHAPE_BAD + [dict(M=1), dict(M=1, flags=3), dict(dY=None), dict(Z=None), dict(mean=None),
                                              dict(rstd=None), dict(gamma=None), dict(scale=None), dict(shift=None),
                                              dict(dZ=None, dRes=None, dgamma=None, dbeta=None), dict(Res=None),
                                              dict(dRes=P), dict(dY=P2)], ids=_ids)
def test_bn_act_backward_rejects_unsupported_arguments(kw):
    L = N.lib()
    a = _bn_args(dict(flags=3))
    a.update(kw)
    _other_message(L)
    rc = L.fr_bn_act_backward(a["dY"], a["Z"], a["M"], a["C"], a["mean"], a["rstd"], a["gamma"], a["scale"], a["shift"],
                              a["Res"], a["flags"], a["dZ"], a["dRes"], a["dgamma"], a["dbeta"], None)
    assert rc == -1 and b"fr_bn_act_backward" in L.fr_last_error(), (kw, rc, L.fr_last_error())


def test_features_at_rejects_a_null_handle():
    L = N.lib()
    h, w, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    _other_message(L)
    assert L.fr_features_at_shape(None, 0, ctypes.byref(h), ctypes.byref(w), ctypes.byref(c)) == -1
    assert b"fr_features_at_shape" in L.fr_last_error()
    _other_message(L)
    assert L.fr_features_at(None, P, 0, 1, 112, 112, 0, P, None) == -1 and b"fr_features_at:" in L.fr_last_error()


def test_module_constructors():
    import torch
    from torch import nn

    import facerecognition_amd as fra
    from facerecognition_amd.backbone_train import Bottleneck, ResNet50Layer4

    assert fra.Bottleneck is Bottleneck and fra.ResNet50Layer4 is ResNet50Layer4
    b = Bottleneck(24, 8, stride=2, downsample=True)
    names = dict(b.named_parameters())
    assert set(names) == {"conv1.weight", "bn1.weight", "bn1.bias", "conv2.weight", "bn2.weight", "bn2.bias", "conv3.weight",
                          "bn3.weight", "bn3.bias", "downsample.0.weight", "downsample.1.weight", "downsample.1.bias"}
    assert all(isinstance(v, nn.Parameter) for v in names.values())
    assert names["conv2.weight"].shape == (8, 8, 3, 3) and names["downsample.0.weight"].shape == (32, 24, 1, 1)
    assert names["conv2.weight"].is_contiguous(memory_format=torch.channels_last)
    assert names["conv2.weight"].permute(0, 2, 3, 1).is_contiguous()  # the device's [Cout][kh][kw][Cin]
    torch.optim.SGD(b.parameters(), lr=0.1)  # ordinary parameters
    with pytest.raises(ValueError):
        Bottleneck(24, 8, stride=2)
    with pytest.raises(ValueError):
        Bottleneck(24, 8)
    assert Bottleneck(32, 8).downsample is None
    assert b.train().batch_stats() and not b.eval().batch_stats()
    b.train().freeze_bn()
    assert not b.batch_stats() and not b.bn1.weight.requires_grad and not b.downsample[1].bias.requires_grad
    assert b.conv1.weight.requires_grad and b.training
    b.bn1.train()
    with pytest.raises(RuntimeError):
        b.batch_stats()
    with pytest.raises(RuntimeError):  # no CPU fallback
        Bottleneck(32, 8)(torch.zeros(2, 4, 4, 32))
    layer = ResNet50Layer4()
    assert [(k.inplanes, k.planes, k.stride, k.downsample is not None) for k in layer.blocks] == [
        (1024, 512, 2, True), (2048, 512, 1, False), (2048, 512, 1, False)]
    assert sum(1 for _ in layer.parameters()) == 30  # the reference's freeze_layers(0.8) leaves these 30 tensors trainable


def test_reference_key_map_round_trips():
    import torch

    from facerecognition_amd import weights as Wt
    from facerecognition_amd.backbone_train import ResNet50Layer4

    arch = "resnet50_arcface"
    layer = ResNet50Layer4()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for t in list(layer.parameters()) + [b for n, b in layer.named_buffers() if "num_batches" not in n]:
            t.copy_(torch.rand(t.shape, generator=g) + 0.5)
        layer.blocks[1].bn2.num_batches_tracked.fill_(7)
    sd = layer.reference_state_dict()
    specs = {k: shape for k, shape, _ in Wt.param_specs(arch)}
    want = [k for k in specs if k.startswith("backbone.layer4.")]
    assert set(sd) == set(want) and sum("num_batches_tracked" in k for k in sd) == 10
    for k, v in sd.items():  # the reference's own keys and shapes, plain contiguous tensors
        assert tuple(v.shape) == tuple(specs[k]) and v.is_contiguous(), k
    other = ResNet50Layer4.for_model(sd)
    for (n1, a), (n2, b) in zip(layer.state_dict().items(), other.state_dict().items()):
        assert n1 == n2 and torch.equal(a, b), n1
    assert other.blocks[0].conv2.weight.permute(0, 2, 3, 1).is_contiguous()  # still the device's layout after the load
    # a full reference state_dict: other keys are ignored, values arrive, and the engine's fold accepts the update
    full = Wt.synth_state_dict(arch)
    third = ResNet50Layer4.for_model(full)
    assert np.array_equal(third.blocks[0].downsample[0].weight.detach().numpy(),
                          np.asarray(full["backbone.layer4.0.downsample.0.weight"], np.float32))
    full.update(sd)
    folded = Wt.fold_state_dict(arch, full)
    assert all(np.all(np.isfinite(v)) for v in folded.values())
