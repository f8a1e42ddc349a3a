"""The fr_head_* and fr_features* entry points at the C-ABI boundary, without a GPU: declared, exported, bound, and every
unsupported argument refused with FR_ERR_ARG and a message naming the entry point before any HIP call (the pointers
below are host memory and are never dereferenced).  Also EmbeddingHead's constructor and its three key maps."""
import ctypes

import numpy as np
import pytest

from facerecognition_amd import _native as N

NEW = {"fr_head_workspace": 3, "fr_head_forward": 31, "fr_head_backward": 29, "fr_features_dim": 1, "fr_features": 8}
INF, NAN = float("inf"), float("nan")


def _p():
    buf = (ctypes.c_uint64 * 64)()
    return buf, ctypes.addressof(buf)


def _other_message(L):
    L.fr_op_avgpool(None, 1, 1, 1, 8, None, 0, None)  # leaves another entry point's message behind


def _ids(kw):
    return ",".join(f"{k}={v}" for k, v in kw.items())


def test_head_functions_are_declared_exported_and_bound():
    L = N.lib()
    for name, nargs in NEW.items():
        assert name in N.header_functions(), name
        assert hasattr(L, name) and name in N._SIGS, name
        assert len(N._SIGS[name][1]) == nargs, name
    assert N._SIGS["fr_head_workspace"][0] is ctypes.c_size_t
    assert (N.FR_HEAD_BATCH_STATS, N.FR_HEAD_DROPOUT) == (1, 2)
    assert L.fr_abi_version() == 1  # additive change


SHAPE_BAD = [dict(B=0), dict(B=-3), dict(K=0), dict(K=2), dict(K=-4), dict(K=6), dict(K=2050), dict(N=0), dict(N=2),
             dict(N=-8), dict(N=510), dict(B=2 ** 21, K=2 ** 20), dict(N=2 ** 20, K=2 ** 21), dict(B=2 ** 21, N=2 ** 20)]
COMMON_BAD = SHAPE_BAD + [dict(S=0), dict(S=-1), dict(S=3), dict(S=4096), dict(flags=4), dict(flags=-1), dict(flags=7),
                          dict(p=-0.1), dict(p=1.0), dict(p=1.5), dict(p=NAN), dict(gamma1=None), dict(beta1=None),
                          dict(B=1, flags=1), dict(B=1, flags=3), dict(B=1, flags=1, gamma1=None, beta1=None),
                          dict(X=None), dict(W=None), dict(gamma2=None), dict(mean2=None), dict(rstd2=None),
                          dict(Z=None), dict(ws=None), dict(ws_bytes=8), dict(mean1=None), dict(rstd1=None)]


def _args(kw):
    _, p = _p()
    a = dict(B=70, K=2048, S=1, N=512, flags=3, p=0.5, eps=1e-5, momentum=0.1, seed=1, offset=0, ws_bytes=1 << 50)
    for name in ("X", "W", "bias", "gamma1", "beta1", "rm1", "rv1", "gamma2", "beta2", "rm2", "rv2", "Y", "Z", "mean1",
                 "rstd1", "mean2", "rstd2", "A", "ws", "dY", "dX", "dW", "dbias", "dgamma1", "dbeta1", "dgamma2", "dbeta2"):
        a[name] = p
    a.update(kw)
    return a


def _forward(L, a):
    return L.fr_head_forward(a["X"], a["B"], a["K"], a["S"], a["W"], a["N"], a["bias"], a["gamma1"], a["beta1"],
                             a["rm1"], a["rv1"], a["gamma2"], a["beta2"], a["rm2"], a["rv2"], a["flags"], a["p"],
                             a["eps"], a["momentum"], a["seed"], a["offset"], a["Y"], a["Z"], a["mean1"], a["rstd1"],
                             a["mean2"], a["rstd2"], a["A"], a["ws"], a["ws_bytes"], None)


def _backward(L, a):
    return L.fr_head_backward(a["X"], a["B"], a["K"], a["S"], a["W"], a["N"], a["gamma1"], a["beta1"], a["gamma2"],
                              a["flags"], a["p"], a["seed"], a["offset"], a["mean1"], a["rstd1"], a["mean2"], a["rstd2"],
                              a["Z"], a["dY"], a["dX"], a["dW"], a["dbias"], a["dgamma1"], a["dbeta1"], a["dgamma2"],
                              a["dbeta2"], a["ws"], a["ws_bytes"], None)


FWD_BAD = COMMON_BAD + [dict(eps=0.0), dict(eps=-1e-5), dict(eps=INF), dict(eps=NAN), dict(momentum=-0.1),
                        dict(momentum=1.1), dict(momentum=NAN), dict(beta2=None), dict(Y=None), dict(rm1=None),
                        dict(rv1=None), dict(rm2=None), dict(rv2=None), dict(rm2=None, flags=0),
                        dict(rm1=None, flags=2), dict(B=1, S=1, flags=1)]


@pytest.mark.parametrize("kw", FWD_BAD, ids=_ids)
def test_forward_rejects_unsupported_arguments(kw):
    L = N.lib()
    _other_message(L)
    rc = _forward(L, _args(kw))
    assert rc == -1 and b"fr_head_forward" in L.fr_last_error(), (kw, rc, L.fr_last_error())


BWD_BAD = COMMON_BAD + [dict(dY=None), dict(dX=None, dW=None, dbias=None, dgamma1=None, dbeta1=None, dgamma2=None,
                                            dbeta2=None),
                        dict(gamma1=None, beta1=None, mean1=None, rstd1=None)]  # dgamma1 without the input BN


@pytest.mark.parametrize("kw", BWD_BAD, ids=_ids)
def test_backward_rejects_unsupported_arguments(kw):
    L = N.lib()
    _other_message(L)
    rc = _backward(L, _args(kw))
    assert rc == -1 and b"fr_head_backward" in L.fr_last_error(), (kw, rc, L.fr_last_error())


def test_workspace():
    L = N.lib()
    for b, k, n in ((2, 16, 4), (70, 332, 68), (256, 2048, 512), (256, 25088, 512)):
        w = L.fr_head_workspace(b, k, n)
        assert w >= b * n * 4 and w % 4 == 0
        assert w < 64 * b * n * 4 + 16 * (b + 64) * k  # split partials and column sums, never a B x K gradient per split
    for kw in SHAPE_BAD:
        a = dict(B=70, K=2048, N=512)
        a.update(kw)
        _other_message(L)
        assert L.fr_head_workspace(a["B"], a["K"], a["N"]) == 0
        assert b"fr_head_workspace" in L.fr_last_error(), kw


def test_features_reject_a_null_handle():
    L = N.lib()
    _, p = _p()
    _other_message(L)
    assert L.fr_features_dim(None) == -1 and b"fr_features_dim" in L.fr_last_error()
    _other_message(L)
    assert L.fr_features(None, p, 0, 1, 112, 112, p, None) == -1 and b"fr_features:" in L.fr_last_error()


def test_module_constructor():
    import torch
    from torch import nn

    import facerecognition_amd as fra
    from facerecognition_amd.head import EmbeddingHead

    assert fra.EmbeddingHead is EmbeddingHead
    h = EmbeddingHead(2048)
    assert (h.in_features, h.embedding_size, h.in_channels, h.spatial, h.dropout, h.eps, h.momentum) == (
        2048, 512, 2048, 1, 0.5, 1e-5, 0.1)
    names = dict(h.named_parameters())
    assert set(names) == {"bn_in.weight", "bn_in.bias", "fc.weight", "fc.bias", "bn_out.weight", "bn_out.bias"}
    assert all(isinstance(v, nn.Parameter) for v in names.values())
    assert {"bn_in.running_mean", "bn_in.running_var", "bn_in.num_batches_tracked", "bn_out.running_mean",
            "bn_out.running_var", "bn_out.num_batches_tracked"} == set(dict(h.named_buffers()))
    assert names["fc.weight"].shape == (512, 2048) and names["bn_in.weight"].shape == (2048,)
    torch.optim.SGD(h.parameters(), lr=0.1)  # ordinary parameters
    h2 = EmbeddingHead(25088, 512, in_channels=512, dropout=0.0)
    assert h2.spatial == 49 and h2.bn_in.weight.shape == (512,)
    h3 = EmbeddingHead(1792, 128, input_bn=False, bias=False, dropout=0.6, eps=1e-3, momentum=0.2)
    assert h3.bn_in is None and h3.fc.bias is None and (h3.eps, h3.momentum) == (1e-3, 0.2)
    assert set(dict(h3.named_parameters())) == {"fc.weight", "bn_out.weight", "bn_out.bias"}
    with pytest.raises(ValueError):
        EmbeddingHead(100, in_channels=7)
    with pytest.raises(ValueError):
        EmbeddingHead(64, dropout=1.0)
    # modes: nn.Module's train / eval, the reference's freeze_bn
    assert h.train().flags() == 3 and h.eval().flags() == 0
    h.train().freeze_bn()
    assert h.flags() == 2 and not h.bn_in.weight.requires_grad and not h.bn_out.bias.requires_grad
    assert h.fc.weight.requires_grad
    assert h2.train().flags() == 1  # p = 0: no dropout to run
    with pytest.raises(RuntimeError):  # no CPU fallback
        h3(torch.randn(4, 1792))


@pytest.mark.parametrize("arch", ["resnet50_arcface", "iresnet100", "irv1_facenet"])
def test_reference_key_maps_round_trip(arch):
    import torch

    from facerecognition_amd import weights as Wt
    from facerecognition_amd.head import EmbeddingHead

    head = EmbeddingHead.for_arch(arch)
    K, S, p, bn_in, bias = {"resnet50_arcface": (2048, 1, 0.5, True, True), "iresnet100": (25088, 49, 0.0, True, True),
                            "irv1_facenet": (1792, 1, 0.6, False, False)}[arch]
    assert (head.in_features, head.embedding_size, head.spatial, head.dropout, head.eps) == (K, 512, S, p, Wt.BN_EPS[arch])
    assert (head.bn_in is not None, head.fc.bias is not None) == (bn_in, bias)
    bn = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")
    want = {"resnet50_arcface": [f"bn1.{f}" for f in bn] + ["fc.weight", "fc.bias"] + [f"bn2.{f}" for f in bn],
            "iresnet100": [f"bn2.{f}" for f in bn] + ["fc.weight", "fc.bias"] + [f"features.{f}" for f in bn],
            "irv1_facenet": ["model.last_linear.weight"] + [f"model.last_bn.{f}" for f in bn]}[arch]
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for t in list(head.parameters()) + [b for n, b in head.named_buffers() if "num_batches" not in n]:
            t.copy_(torch.rand(t.shape, generator=g) + 0.5)
        head.bn_out.num_batches_tracked.fill_(7)
    sd = head.reference_state_dict()
    assert list(sd) == want
    specs = {k: shape for k, shape, _ in Wt.param_specs(arch)}
    for k, v in sd.items():  # the reference's own keys and shapes
        assert k in specs and tuple(v.shape) == tuple(specs[k]), k
    other = EmbeddingHead.for_arch(arch, sd)
    for (n1, a), (n2, b) in zip(head.state_dict().items(), other.state_dict().items()):
        assert n1 == n2 and torch.equal(a, b), n1
    # a full reference state_dict: other keys are ignored, values arrive, and the engine's fold accepts the update
    full = Wt.synth_state_dict(arch)
    third = EmbeddingHead.for_arch(arch, full)
    k_fc = want[0] if arch == "irv1_facenet" else "fc.weight"
    assert np.array_equal(third.fc.weight.detach().numpy(), np.asarray(full[k_fc], np.float32).reshape(512, K))
    full.update(sd)
    folded = Wt.fold_state_dict(arch, full)
    assert folded["head.w"].shape == (512, K) and np.all(np.isfinite(folded["head.w"]))
