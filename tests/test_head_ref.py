"""tests/head_ref.py (the float64 restatement of head training the GPU tests are measured against) checked on the
CPU: against torch float64 autograd over nn.BatchNorm1d / nn.BatchNorm2d(...).flatten / nn.Linear with the restated
mask multiplied in (1e-10 relative, every flag combination, the three head variants, the running statistics), its
Philox4x32-10 against Random123's known answers, the drop rate and the offset, eval mode against the folded
inference head of weights.fold_state_dict, and the committed golden case."""
import os

import numpy as np
import pytest

from tests.head_ref import (BATCH_STATS, DROPOUT, dropout_mask, dropout_threshold, head_ref, make_case, philox4x32_10,
                            ref_of)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_golden.npz")
# (input BN, bias, S): ArcFaceModel's head, IResNet100's, FaceNet's
VARIANTS = {"arcface": (True, True, 1), "iresnet": (True, True, 49), "facenet": (False, False, 1)}


def torch_head(case, S, flags, p, eps, mom, keep):
    """The same step in unfused torch float64 ops; returns numpy outputs named as head_ref's."""
    import torch
    from torch import nn

    t = lambda a: None if a is None else torch.tensor(np.asarray(a, np.float64))
    batch, drop = bool(flags & BATCH_STATS), bool(flags & DROPOUT) and np.float32(p) > 0
    eps, mom = float(np.float32(eps)), float(np.float32(mom))
    x = t(case["X"]).requires_grad_(True)
    B, K = x.shape
    N = case["W"].shape[0]
    out = {}
    h, bn1 = x, None
    if case["gamma1"] is not None:
        Cin = K // S
        side = int(round(S ** 0.5))
        two_d = S > 1 and side * side == S
        bn1 = (nn.BatchNorm2d if two_d else nn.BatchNorm1d)(Cin, eps=eps, momentum=mom).double()
        with torch.no_grad():
            bn1.weight.copy_(t(case["gamma1"])); bn1.bias.copy_(t(case["beta1"]))
            bn1.running_mean.copy_(t(case["rm1"])); bn1.running_var.copy_(t(case["rv1"]))
        bn1.train(batch)
        shaped = x.view(B, Cin, side, side) if two_d else (x.view(B, Cin, S) if S > 1 else x)
        h = bn1(shaped).flatten(1)
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if drop else 1.0
    a = h * t(keep.astype(np.float64)) * scale if drop else h
    fc = nn.Linear(K, N, bias=case["bias"] is not None).double()
    bn2 = nn.BatchNorm1d(N, eps=eps, momentum=mom).double()
    with torch.no_grad():
        fc.weight.copy_(t(case["W"]))
        if case["bias"] is not None:
            fc.bias.copy_(t(case["bias"]))
        bn2.weight.copy_(t(case["gamma2"])); bn2.bias.copy_(t(case["beta2"]))
        bn2.running_mean.copy_(t(case["rm2"])); bn2.running_var.copy_(t(case["rv2"]))
    bn2.train(batch)
    a.retain_grad() if a.requires_grad else None
    z = fc(a)
    y = bn2(z)
    y.backward(t(case["dY"]))
    n = lambda v: v.detach().numpy().copy()
    out.update(A=n(a), Z=n(z), Y=n(y), dX=n(x.grad), dW=n(fc.weight.grad), dgamma2=n(bn2.weight.grad),
               dbeta2=n(bn2.bias.grad), rm2=n(bn2.running_mean), rv2=n(bn2.running_var))
    if case["bias"] is not None:
        out["dbias"] = n(fc.bias.grad)
    if bn1 is not None:
        out.update(dgamma1=n(bn1.weight.grad), dbeta1=n(bn1.bias.grad), rm1=n(bn1.running_mean), rv1=n(bn1.running_var))
    return out


def assert_close(name, got, want, rel=1e-10):
    scale = max(1.0, float(np.max(np.abs(want))))
    assert np.max(np.abs(got - want)) <= rel * scale, (name, float(np.max(np.abs(got - want))), scale)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_restatement_equals_torch_float64(variant, flags):
    input_bn, bias, S = VARIANTS[variant]
    B, Cin, N = 6, 4, 8
    p, eps, mom, seed, offset = (0.6 if variant == "facenet" else 0.5), 1e-5, 0.1, 77, 5
    case = make_case(3, B, Cin, S, N, input_bn, bias)
    ref = ref_of(case, S, flags, p, eps, mom, seed, offset)
    assert np.array_equal(ref["keep"], dropout_mask(B, Cin * S, p, seed, offset) if flags & DROPOUT
                          else np.ones((B, Cin * S), bool))
    if flags & DROPOUT:
        assert 0 < ref["keep"].sum() < ref["keep"].size
    t = torch_head(case, S, flags, p, eps, mom, ref["keep"])
    for name, want in t.items():
        assert_close(name, ref[name], want)
    if not flags & BATCH_STATS:
        assert np.array_equal(ref["rm2"], case["rm2"]) and np.array_equal(ref["rv2"], case["rv2"])
    for name in ("Y", "A", "Z", "dW", "dX", "dgamma2", "dbeta2"):  # every bound exists, is finite and is not vacuous
        b = ref[name + "_"]
        assert b.shape == ref[name].shape and np.all(np.isfinite(b)) and np.all(b >= 0)
        assert np.median(b) <= 1e-2 * max(1.0, float(np.max(np.abs(ref[name])))), name


def test_philox_known_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        got = philox4x32_10(np.array(ctr, np.uint64), np.array(key, np.uint64))
        assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]
    got = philox4x32_10(np.array([k[0] for k in kat], np.uint64), np.array([k[1] for k in kat], np.uint64))  # batched
    assert [tuple(int(v) for v in row) for row in got] == [k[2] for k in kat]


@pytest.mark.parametrize("p", [0.5, 0.6])
def test_drop_rate_and_offset(p):
    B, K = 130, 2048
    T = dropout_threshold(p)
    assert T == int(np.floor(float(np.float32(p)) * 2.0 ** 32))
    q = T / 2.0 ** 32
    keep = dropout_mask(B, K, p, 2024, 0)
    n = B * K
    dropped = n - int(keep.sum())
    assert abs(dropped - n * q) <= 5 * np.sqrt(n * q * (1 - q)), (dropped, n * q)
    other = dropout_mask(B, K, p, 2024, 1)
    assert not np.array_equal(keep, other) and not np.array_equal(keep, dropout_mask(B, K, p, 2025, 0))
    assert np.array_equal(keep, dropout_mask(B, K, p, 2024, 0))
    assert np.array_equal(dropout_mask(B, K, p, 2024, 1 << 32), dropout_mask(B, K, p, 2024, 1 << 32))
    assert not np.array_equal(dropout_mask(B, K, p, 2024, 1 << 32), keep)  # the offset's high word counts


@pytest.mark.parametrize("arch", ["resnet50_arcface", "iresnet100", "irv1_facenet"])
def test_eval_mode_equals_the_folded_inference_head(arch):
    from facerecognition_amd import weights as Wt
    from facerecognition_amd.head import EmbeddingHead

    sd = Wt.synth_state_dict(arch)
    folded = Wt.fold_state_dict(arch, sd)
    head = EmbeddingHead.for_arch(arch, sd)
    K, S = head.in_features, head.spatial
    assert (K, S) == {"resnet50_arcface": (2048, 1), "iresnet100": (25088, 49), "irv1_facenet": (1792, 1)}[arch]
    X = np.random.default_rng(4).standard_normal((3, K))
    n = lambda t: None if t is None else t.detach().numpy().astype(np.float64)
    bi, bo = head.bn_in, head.bn_out
    ref = head_ref(X, S, n(head.fc.weight), n(head.fc.bias), *(
        (n(bi.weight), n(bi.bias), n(bi.running_mean), n(bi.running_var)) if bi is not None else (None,) * 4),
        n(bo.weight), n(bo.bias), n(bo.running_mean), n(bo.running_var), flags=0, eps=head.eps, round_scalars=False)
    w = folded["head.w"].astype(np.float64)
    if arch == "iresnet100":  # the engine reads NHWC (p * 512 + c), the head torch's flatten order (c * 49 + p)
        w = w.reshape(512, 49, 512).transpose(0, 2, 1).reshape(512, K)
    # fold_state_dict's own float64 fold (its formulas over its _bn_affine), before it rounds head.w / head.b to
    # float32: 1e-10; then the float32 arrays it returns: 2^-24 relative per product and on the bias
    k_in, k_fc, k_out = head.keys
    so, to = Wt._bn_affine(sd, k_out, head.eps)
    W64 = np.asarray(sd[k_fc + ".weight"], np.float64).reshape(512, K)
    b64 = np.asarray(sd[k_fc + ".bias"], np.float64) if head.fc.bias is not None else np.zeros(512)
    if k_in is not None:
        si, ti = (np.repeat(v, S) for v in Wt._bn_affine(sd, k_in, head.eps))
        w64, bias64 = so[:, None] * W64 * si[None, :], so * (W64 @ ti + b64) + to
    else:
        w64, bias64 = so[:, None] * W64, so * b64 + to
    assert np.array_equal(w64.astype(np.float32), w.astype(np.float32))  # the same fold
    want64 = X @ w64.T + bias64
    assert np.max(np.abs(ref["Y"] - want64)) <= 1e-10 * max(1.0, np.abs(want64).max())
    want = X @ w.T + folded["head.b"].astype(np.float64)
    tol = 2.0 ** -23 * (np.abs(X) @ np.abs(w).T + np.abs(folded["head.b"])) + 1e-10 * np.abs(want).max()
    assert np.all(np.abs(ref["Y"] - want) <= tol), float(np.max(np.abs(ref["Y"] - want) / tol))


def test_golden_case_pins_the_restatement():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) <= 100 * 1024
    case = {k: None for k in ("bias", "gamma1", "beta1", "rm1", "rv1")}
    case.update({k[3:]: g[k] for k in g.files if k.startswith("in_")})
    S, flags, p, eps, mom = g["scalars"]
    seed, offset = (int(v) for v in g["seed_offset"])
    ref = ref_of(case, int(S), int(flags), float(p), float(eps), float(mom), seed, offset)
    assert np.array_equal(ref["keep"], g["keep"])
    names = [k[4:] for k in g.files if k.startswith("out_")]
    assert {"Y", "A", "Z", "dX", "dW", "dbias", "dgamma1", "dbeta1", "dgamma2", "dbeta2", "rm1", "rv1", "rm2", "rv2"} <= set(names)
    for name in names:
        assert_close(name, ref[name], g["out_" + name])
