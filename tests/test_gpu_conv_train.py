"""fr_conv_train_forward / _backward, fr_bn2d_train_stats and fr_bn_act_forward / _backward on the GPU against the float64
restatement tests/conv_train_ref.py, which also supplies every bound (u = 2^-24; derivations in its docstring).  Each
assertion is error / bound <= 1; the largest ratio of every quantity is printed.

Measured largest ratios (MI355X; per quantity over all cases and modes, DESIGN.md §4 "Backbone training: layer4"):
  Z 0.038, dA 0.27, dW 0.18, mean 0.094, rstd 0.46, scale 0.46, shift 0.52, rm 0.12, rv 0.21, Y 0.71, dZ 0.45,
  dgamma 0.14, dbeta 0.076

Convolution cases (B, H, W, Cin, Cout, k, stride):
  (1,1,1,4,4,1,1)      the minimum
  (2,4,4,8,68,3,1)     all-border 4 x 4, Cout crosses a tile edge
  (2,5,6,4,4,3,1)      H != W
  (3,7,7,12,8,3,2)     odd size, stride 2, 7 -> 4; M of the data gradient (147) crosses two tile edges
  (3,7,7,20,72,1,2)    the downsample: dA is three-quarters zeros
  (5,4,4,132,4,1,1)    K crosses two 64-chunks, M (80) crosses a tile
  (2,4,4,512,512,3,1)  layer4's own channels at a tiny batch; the split-K boundary (36 splits)
  (2,4,4,2048,512,1,1) as above (32 splits)
Each runs without the input transform, with it, and with its ReLU; with dA and dW both requested and each alone.  The
transform's shift is nonzero in every channel (both signs), so a padded tap filled with relu(shift) instead of 0 breaks
the bound of Z and dW on every border pixel -- and every pixel of a 4 x 4 map is one.  BN cases (M, C) = (2,4), (70,68),
(130,132): both statistics modes, with and without residual and ReLU, dZ separate and written over dY.  Every call is
run twice, and the forward once more with a four-fold workspace; all outputs are bitwise equal.
Every raw C call allocates its buffers 64 sentinel elements too long and checks that the sentinels survive.
"""
import numpy as np
import pytest

from tests import conv_train_calls as C
from tests import conv_train_ref as R

pytestmark = pytest.mark.gpu

worst = {}


def note(name, got, want, bound):
    r = float(np.max(R.ratio(np.asarray(got, np.float64) - want, bound)))
    worst[name] = max(worst.get(name, 0.0), r)
    print(f"  {name}: largest error / bound = {r:.3g}")
    return r


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda", 0)


@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_convolution_against_the_restatement(dev, case):
    c = R.make_conv_case(R.CONV_SEEDS[case], *case)
    X, Wt, dZ, k, stride = c["X"], c["Wt"], c["dZ"], c["k"], c["stride"]
    worst_here = 0.0
    for mode, (sc, sh, flags) in dict(plain=(None, None, 0), affine=(c["scale"], c["shift"], 0),
                                      relu=(c["scale"], c["shift"], R.IN_RELU)).items():
        print(f"case {case} {mode}")
        ref = R.conv_ref(X, Wt, k, stride, sc, sh, flags, dZ)
        Z = C.conv_forward(dev, X, Wt, k, stride, sc, sh, flags)
        both = C.conv_backward(dev, X, Wt, k, stride, dZ, sc, sh, flags)
        worst_here = max(worst_here, note("Z", Z, ref["Z"], ref["Z_"]), note("dA", both["dA"], ref["dA"], ref["dA_"]),
                         note("dW", both["dW"], ref["dW"], ref["dW_"]))
        # each gradient alone: the other is not written, the result is the same bit for bit
        only_a = C.conv_backward(dev, X, Wt, k, stride, dZ, sc, sh, flags, want_dw=False)
        only_w = C.conv_backward(dev, X, Wt, k, stride, dZ, sc, sh, flags, want_da=False)
        assert set(only_a) == {"dA"} and set(only_w) == {"dW"}
        assert same(only_a["dA"], both["dA"]) and same(only_w["dW"], both["dW"])
        # repeatable, and independent of the workspace size
        assert same(C.conv_forward(dev, X, Wt, k, stride, sc, sh, flags), Z)
        assert same(C.conv_forward(dev, X, Wt, k, stride, sc, sh, flags, ws_scale=4), Z)
        again = C.conv_backward(dev, X, Wt, k, stride, dZ, sc, sh, flags)
        assert same(again["dA"], both["dA"]) and same(again["dW"], both["dW"])
        if stride == 2 and k == 1:  # pixels no tap reaches: +0.0f, never stale memory (the buffers start as 7.5)
            reached = np.zeros(X.shape[1:3], bool)
            reached[::2, ::2] = True
            assert np.all(both["dA"][:, ~reached].view(np.uint32) == 0)
            assert np.any(both["dA"][:, reached] != 0)
    assert worst_here <= 1.0, worst_here


def test_padded_taps_are_zero_in_the_transformed_space(dev):
    """X = 0 everywhere and a transform with shift > 0: A = relu(shift) inside the image and 0 in the padding, so Z at a
    border pixel sums fewer taps than Z in the interior, exactly as the restatement says."""
    B, H, W, Cin, Cout = 1, 5, 5, 4, 4
    X = np.zeros((B, H, W, Cin), np.float32)
    Wt = np.ones((Cout, 3, 3, Cin), np.float32)
    sc, sh = np.ones(Cin, np.float32), np.full(Cin, 0.5, np.float32)
    Z = C.conv_forward(dev, X, Wt, 3, 1, sc, sh, R.IN_RELU)
    taps = np.array([[4, 6, 6, 6, 4], [6, 9, 9, 9, 6], [6, 9, 9, 9, 6], [6, 9, 9, 9, 6], [4, 6, 6, 6, 4]], np.float32)
    assert np.array_equal(Z, np.broadcast_to((taps * 0.5 * Cin)[None, :, :, None], Z.shape))
    dW = C.conv_backward(dev, X, Wt, 3, 1, np.ones_like(Z), sc, sh, R.IN_RELU, want_da=False)["dW"]
    reach = np.array([[16, 20, 16], [20, 25, 20], [16, 20, 16]], np.float32)  # output pixels whose tap (r, s) is inside
    assert np.array_equal(dW, np.broadcast_to((reach * 0.5)[None, :, :, None], dW.shape))


def run_bn(dev, c, flags, with_res, alias=False):
    res = c["Res"] if with_res else None
    st = C.bn_stats(dev, c["Z"], c["gamma"], c["beta"], c["rm"], c["rv"], flags & 1, R.EPS_BN, R.MOM)
    out = dict(st)
    out["Y"] = C.bn_act_forward(dev, c["Z"], st["scale"], st["shift"], res, flags & 2)
    out.update(C.bn_act_backward(dev, c["dY"], c["Z"], st, c["gamma"], res, flags, want_res=with_res, alias=alias))
    return out


@pytest.mark.parametrize("case", R.BN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_batchnorm_against_the_restatement(dev, case):
    c = R.make_bn_case(R.BN_SEEDS[case], *case)
    worst_here = 0.0
    for flags in (0, 1, 2, 3):
        for with_res in (False, True):
            print(f"case {case} flags {flags} residual {with_res}")
            ref = R.bn_case_ref(c, flags, with_res)
            got = run_bn(dev, c, flags, with_res)
            for name in ("mean", "rstd", "scale", "shift", "rm", "rv", "Y", "dZ", "dgamma", "dbeta"):
                worst_here = max(worst_here, note(name, got[name], ref[name], ref[name + "_"]))
            if not flags & 1:  # running statistics are left alone, bit for bit
                assert same(got["rm"], c["rm"]) and same(got["rv"], c["rv"])
                assert same(got["mean"], c["rm"])
            # the mask is the restatement's (make_bn_case asserts the margin): exact zeros where the ReLU closes
            assert np.all(got["Y"][~ref["mask"]].view(np.uint32) == 0)
            if with_res:  # dRes = dH: dY where the ReLU passes, +0.0f elsewhere
                assert same(got["dRes"], np.where(ref["mask"], c["dY"], np.float32(0)).astype(np.float32))
            # dZ written over dY, and a second run: bitwise the same
            over, again = run_bn(dev, c, flags, with_res, alias=True), run_bn(dev, c, flags, with_res)
            for name in got:
                assert same(over[name], got[name]) and same(again[name], got[name]), name
            # the gradients are optional: dgamma / dbeta NULL leaves dZ unchanged; they alone match too
            st = {k: got[k] for k in ("mean", "rstd", "scale", "shift")}
            res = c["Res"] if with_res else None
            noaff = C.bn_act_backward(dev, c["dY"], c["Z"], st, c["gamma"], res, flags, want_affine=False)
            assert set(noaff) == {"dZ"} and same(noaff["dZ"], got["dZ"])
            aff = C.bn_act_backward(dev, c["dY"], c["Z"], st, c["gamma"], res, flags, want_dz=False)
            assert set(aff) == {"dgamma", "dbeta"} and same(aff["dgamma"], got["dgamma"]) and same(aff["dbeta"], got["dbeta"])
    assert worst_here <= 1.0, worst_here


def test_print_the_largest_ratios():
    print("  largest error / bound per quantity:", ", ".join(f"{k} {v:.2g}" for k, v in worst.items()))
