"""tests/conv_train_ref.py (the float64 restatement the GPU tests of backbone training are held against) against torch
float64 autograd on the CPU, to 1e-10 (max |difference| / max |value|), on every case the GPU tests use; and the ReLU
margins those cases assert when they are made."""
import numpy as np
import pytest

from tests import conv_train_ref as R

TOL = 1e-10


def _t(a, grad=False):
    import torch

    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("mode", ["plain", "affine", "relu"])
def test_convolution_against_torch_float64(case, mode):
    import torch
    import torch.nn.functional as F

    c = R.make_conv_case(R.CONV_SEEDS[case], *case)
    k, stride = c["k"], c["stride"]
    sc, sh = (None, None) if mode == "plain" else (c["scale"], c["shift"])
    ref = R.conv_ref(c["X"], c["Wt"], k, stride, sc, sh, R.IN_RELU if mode == "relu" else 0, c["dZ"])
    a = _t(c["X"])
    if sc is not None:
        a = a * _t(sc) + _t(sh)
        a = torch.relu(a) if mode == "relu" else a
    a = a.permute(0, 3, 1, 2).detach().requires_grad_(True)  # dA is the gradient by the transformed input
    w = _t(c["Wt"]).permute(0, 3, 1, 2).detach().requires_grad_(True)
    z = F.conv2d(a, w, None, stride, k // 2)
    z.backward(_t(c["dZ"]).permute(0, 3, 1, 2))
    nhwc = lambda v: v.detach().permute(0, 2, 3, 1).numpy()
    assert R.rel_err(ref["Z"], nhwc(z)) <= TOL
    assert R.rel_err(ref["dA"], nhwc(a.grad)) <= TOL
    assert R.rel_err(ref["dW"], nhwc(w.grad)) <= TOL
    for name in ("Z", "dA", "dW"):  # the bounds are bounds: non-negative, finite, and zero only where nothing is summed
        assert np.all(np.isfinite(ref[name + "_"])) and np.all(ref[name + "_"] >= 0), name
    if stride == 2 and k == 1:  # the downsample reaches a quarter of the pixels (ceil), the rest get exact zeros
        reached = np.zeros(c["X"].shape[1:3], bool)
        reached[::2, ::2] = True
        assert np.all(ref["dA"][:, ~reached] == 0) and np.all(ref["dA_"][:, ~reached] == 0)


@pytest.mark.parametrize("case", R.BN_CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("with_res", [False, True])
def test_batchnorm_against_torch_float64(case, flags, with_res):
    import torch
    import torch.nn.functional as F

    c = R.make_bn_case(R.BN_SEEDS[case], *case)
    ref = R.bn_case_ref(c, flags, with_res)
    z, g, b = _t(c["Z"], True), _t(c["gamma"], True), _t(c["beta"], True)
    res = _t(c["Res"], True) if with_res else None
    rm, rv = _t(c["rm"]), _t(c["rv"])
    y = F.batch_norm(z, rm, rv, g, b, bool(flags & 1), float(np.float32(R.MOM)), float(np.float32(R.EPS_BN)))
    y = y + res if with_res else y
    y = torch.relu(y) if flags & 2 else y
    y.backward(_t(c["dY"]))
    assert R.rel_err(ref["Y"], y.detach().numpy()) <= TOL
    assert R.rel_err(ref["dZ"], z.grad.numpy()) <= TOL
    assert R.rel_err(ref["dgamma"], g.grad.numpy()) <= TOL and R.rel_err(ref["dbeta"], b.grad.numpy()) <= TOL
    assert R.rel_err(ref["rm"], rm.numpy()) <= TOL and R.rel_err(ref["rv"], rv.numpy()) <= TOL
    if with_res:
        assert R.rel_err(ref["dRes"], res.grad.numpy()) <= TOL
    if not flags & 1:
        assert np.array_equal(ref["rm"], c["rm"]) and np.array_equal(ref["rv"], c["rv"])
    assert ref["margin"] > 1.0 or not flags & 2


@pytest.mark.parametrize("name", list(R.BLOCK_CASES))
@pytest.mark.parametrize("batch_stats", [True, False])
def test_bottleneck_of_the_five_calls_against_torch_float64(name, batch_stats):
    import torch

    case = R.make_block_case(R.BLOCK_SEEDS[name], **R.BLOCK_CASES[name])
    mine = R.bottleneck_ref(case, batch_stats, round_scalars=False)
    want = R.torch_bottleneck(case, batch_stats, torch.float64)
    assert mine["margin"] > R.BLOCK_MARGIN
    got = dict(R.flat_items(mine))
    for key, v in R.flat_items(want):
        assert R.rel_err(got[key], v) <= TOL, key
