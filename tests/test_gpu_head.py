"""fr_head_forward / fr_head_backward, fr_features and facerecognition_amd.head on the GPU against the float64
restatement tests/head_ref.py, which also supplies every bound (u = 2^-24; derivations in its docstring).  Each
assertion is error / bound <= 1; the largest ratio of every quantity is printed.

Measured largest ratios (MI355X; per quantity over the six shapes and five modes, DESIGN.md §4 "Head training"):
  A 0.48, Z 0.037, Y 0.027, mean1 0.28, rstd1 0.48, rm1 0.38, rv1 0.30, mean2 0.033, rstd2 0.46, rm2 0.035, rv2 0.0039,
  dX 0.091, dW 0.33, dbias 0.24, dgamma1 0.10, dbeta1 0.071, dgamma2 0.016, dbeta2 0.18
  features round trip, 1 - cos: 2.0e-5 / 1.7e-6 / 1.8e-5 (ResNet-50 / IResNet100 / IRV1), after the reload 2.1e-5 /
  1.3e-6 / 1.2e-5; training loop: loss 35.0 -> below 1e-4 in 20 steps, both runs bitwise equal

Shapes (B, Cin, S, N): the smallest that cross a 64 x 64 tile edge, the split-K boundary and the grouped BN, the
FaceNet head without input BN and bias, and IResNet100's own head.  Modes (flags, p): each of the four flag values
with p = 0.5, and both flags with p = 0 (no generator runs).  Every mode runs with dX requested and with dX NULL.
Every raw C call allocates its buffers 64 sentinel elements too long and checks that the sentinels survive.
"""
import hashlib

import numpy as np
import pytest

from tests.head_ref import make_case, ratio, ref_of

pytestmark = pytest.mark.gpu

GUARD, SENT = 64, 7.5
SHAPES = [(2, 16, 1, 4, True), (70, 332, 1, 68, True), (130, 4, 49, 132, True), (3, 2048, 1, 512, True),
          (130, 1792, 1, 512, False), (2, 512, 49, 512, True)]  # (B, Cin, S, N, input BN and bias)
MODES = [(0, 0.5), (1, 0.5), (2, 0.5), (3, 0.5), (3, 0.0)]
EPS_BN, MOM, SEED, OFFSET = 1e-5, 0.1, 0x9E3779B97F4A7C15, (1 << 32) + 5
worst = {}


def note(name, got, want, bound):
    r = float(np.max(ratio(np.asarray(got, np.float64) - want, bound)))
    worst[name] = max(worst.get(name, 0.0), r)
    print(f"  {name}: largest error / bound = {r:.3g}")
    return r


def run_c(dev, case, S, flags, p, seed=SEED, offset=OFFSET, want_dx=True, ws_scale=1, backward=True):
    """The two raw C calls with sentinel-guarded buffers; returns numpy results (bitwise the device's)."""
    import torch
    from facerecognition_amd import _native as NL

    L = NL.lib()
    B, K = case["X"].shape
    N = case["W"].shape[0]
    Cin = K // S
    has_bn1, has_bias = case["gamma1"] is not None, case["bias"] is not None
    bufs = {}

    def guarded(name, n, init=None):
        t = torch.full((n + GUARD,), SENT, dtype=torch.float32, device=dev)
        if init is not None:
            t[:n] = torch.from_numpy(np.ascontiguousarray(init, np.float32).reshape(-1)).to(dev)
        bufs[name] = (t, n)
        return t

    for name in ("X", "W", "gamma2", "beta2", "rm2", "rv2", "dY"):
        guarded(name, case[name].size, case[name])
    for name in ("bias", "gamma1", "beta1", "rm1", "rv1"):
        if case[name] is not None:
            guarded(name, case[name].size, case[name])
    nbytes = L.fr_head_workspace(B, K, N)
    assert 0 < nbytes and nbytes % 4 == 0
    guarded("ws", ws_scale * nbytes // 4)
    for name, n in (("Y", B * N), ("Z", B * N), ("mean2", N), ("rstd2", N), ("A", B * K)):
        guarded(name, n)
    if has_bn1:
        guarded("mean1", Cin)
        guarded("rstd1", Cin)
    P = lambda name: NL.ptr(bufs[name][0]) if name in bufs else 0
    st = NL.stream_ptr(dev)
    NL.check(L.fr_head_forward(P("X"), B, K, S, P("W"), N, P("bias"), P("gamma1"), P("beta1"), P("rm1"), P("rv1"),
                               P("gamma2"), P("beta2"), P("rm2"), P("rv2"), flags, p, EPS_BN, MOM, seed, offset, P("Y"),
                               P("Z"), P("mean1"), P("rstd1"), P("mean2"), P("rstd2"), P("A"), P("ws"),
                               ws_scale * nbytes, st), "fr_head_forward")
    if backward:
        outs = [("dW", N * K), ("dgamma2", N), ("dbeta2", N)]
        outs += [("dX", B * K)] if want_dx else []
        outs += [("dbias", N)] if has_bias else []
        outs += [("dgamma1", Cin), ("dbeta1", Cin)] if has_bn1 else []
        for name, n in outs:
            guarded(name, n)
        NL.check(L.fr_head_backward(P("X"), B, K, S, P("W"), N, P("gamma1"), P("beta1"), P("gamma2"), flags, p, seed,
                                    offset, P("mean1"), P("rstd1"), P("mean2"), P("rstd2"), P("Z"), P("dY"), P("dX"),
                                    P("dW"), P("dbias"), P("dgamma1"), P("dbeta1"), P("dgamma2"), P("dbeta2"), P("ws"),
                                    ws_scale * nbytes, st), "fr_head_backward")
    torch.cuda.synchronize()
    out = {}
    shapes = {"Y": (B, N), "Z": (B, N), "A": (B, K), "dX": (B, K), "dW": (N, K)}
    for name, (t, n) in bufs.items():
        h = t.cpu().numpy()
        if name != "ws":
            assert np.all(h[n:] == SENT), f"{name}: sentinel overwritten"
            out[name] = h[:n].reshape(shapes.get(name, (n,))).copy()
    for name in ("X", "W", "bias", "gamma1", "beta1", "gamma2", "beta2", "dY"):  # inputs are read only
        if name in out:
            assert np.array_equal(out[name].reshape(-1), np.asarray(case[name], np.float32).reshape(-1)), name
    return out


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda", 0)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
def test_raw_calls_against_the_restatement(dev, shape):
    B, Cin, S, N, full = shape
    K = Cin * S
    case = make_case(B + N, B, Cin, S, N, input_bn=full, bias=full)
    worst_here = 0.0
    for flags, p in MODES:
        print(f"shape {shape} flags {flags} p {p}")
        ref = ref_of(case, S, flags, p, EPS_BN, MOM, SEED, OFFSET)
        got = run_c(dev, case, S, flags, p)
        names = ["A", "Z", "Y", "mean2", "rstd2", "rm2", "rv2", "dX", "dW", "dgamma2", "dbeta2"]
        names += ["dbias"] if full else []
        names += ["mean1", "rstd1", "rm1", "rv1", "dgamma1", "dbeta1"] if full else []
        for name in names:
            worst_here = max(worst_here, note(name, got[name], ref[name], ref[name + "_"]))
        if not flags & 1:  # running statistics are left alone, bit for bit
            for name in ("rm2", "rv2") + (("rm1", "rv1") if full else ()):
                assert np.array_equal(got[name], case[name]), name
        # the mask: +0.0 exactly where the restatement drops, and nowhere else where H != 0
        keep = ref["keep"]
        assert (flags & 2 and p > 0) == (not keep.all())
        bits = got["A"].view(np.uint32)
        assert np.all(bits[~keep] == 0)
        assert np.all(got["A"][keep & (ref["H"] != 0)] != 0)
        if not (flags & 2 and p > 0) and not full:
            assert np.array_equal(got["A"], case["X"])  # no BN, no dropout: A is X
        # dX NULL: every other result is the same, bit for bit
        nodx = run_c(dev, case, S, flags, p, want_dx=False)
        assert "dX" not in nodx
        for name in nodx:
            assert np.array_equal(nodx[name].view(np.uint32), got[name].view(np.uint32)), name
    assert worst_here <= 1.0, worst_here


def test_repeatable_and_independent_of_the_workspace(dev):
    B, Cin, S, N = 70, 332, 1, 68
    case = make_case(9, B, Cin, S, N)
    a = run_c(dev, case, S, 3, 0.5)
    b = run_c(dev, case, S, 3, 0.5)
    c = run_c(dev, case, S, 3, 0.5, ws_scale=4)
    d = run_c(dev, case, S, 3, 0.5, offset=OFFSET + 1)
    for name in a:
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), name
        assert np.array_equal(a[name].view(np.uint32), c[name].view(np.uint32)), name
    assert not np.array_equal(a["A"], d["A"])  # another offset, another mask


@pytest.mark.parametrize("shape", [(70, 332, 1, 68, True), (130, 4, 49, 132, True), (70, 332, 1, 68, False)],
                         ids=["bn1d", "bn2d", "facenet"])
def test_module_path_equals_the_raw_calls_bitwise(dev, shape):
    import torch

    from facerecognition_amd.head import EmbeddingHead

    B, Cin, S, N, full = shape
    K = Cin * S
    case = make_case(21, B, Cin, S, N, input_bn=full, bias=full)
    raw = run_c(dev, case, S, 3, 0.5, seed=1234, offset=7)
    head = EmbeddingHead(K, N, in_channels=Cin, input_bn=full, bias=full, dropout=0.5, eps=EPS_BN, momentum=MOM).to(dev)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)
    with torch.no_grad():
        head.fc.weight.copy_(t(case["W"]))
        head.bn_out.weight.copy_(t(case["gamma2"])); head.bn_out.bias.copy_(t(case["beta2"]))
        head.bn_out.running_mean.copy_(t(case["rm2"])); head.bn_out.running_var.copy_(t(case["rv2"]))
        if full:
            head.fc.bias.copy_(t(case["bias"]))
            head.bn_in.weight.copy_(t(case["gamma1"])); head.bn_in.bias.copy_(t(case["beta1"]))
            head.bn_in.running_mean.copy_(t(case["rm1"])); head.bn_in.running_var.copy_(t(case["rv1"]))
    head.train().seed(1234, 7)
    x = t(case["X"]).requires_grad_(True)
    y = head(x)
    y.backward(t(case["dY"]))
    torch.cuda.synchronize()
    same = lambda name, v: np.array_equal(v.detach().cpu().numpy().view(np.uint32), raw[name].view(np.uint32))
    assert same("Y", y) and same("dX", x.grad) and same("dW", head.fc.weight.grad)
    assert same("dgamma2", head.bn_out.weight.grad) and same("dbeta2", head.bn_out.bias.grad)
    assert same("rm2", head.bn_out.running_mean) and same("rv2", head.bn_out.running_var)
    assert int(head.bn_out.num_batches_tracked) == 1 and head._offset == 8
    if full:
        assert same("dbias", head.fc.bias.grad) and same("dgamma1", head.bn_in.weight.grad)
        assert same("dbeta1", head.bn_in.bias.grad) and same("rm1", head.bn_in.running_mean)
        assert same("rv1", head.bn_in.running_var) and int(head.bn_in.num_batches_tracked) == 1
    # eval: the running statistics, no dropout, nothing tracked; a frozen input asks for no dX
    ev = run_c(dev, {**case, **{k: raw[k] for k in ("rm2", "rv2") + (("rm1", "rv1") if full else ())}}, S, 0, 0.5,
               backward=False)
    y2 = head.eval()(t(case["X"]))
    torch.cuda.synchronize()
    assert np.array_equal(y2.detach().cpu().numpy().view(np.uint32), ev["Y"].view(np.uint32))
    assert int(head.bn_out.num_batches_tracked) == 1 and head._offset == 8


@pytest.mark.parametrize("arch", ["resnet50_arcface", "iresnet100", "irv1_facenet"])
def test_features_and_the_round_trip_into_the_engine(dev, arch):
    import torch

    from facerecognition_amd import weights as Wt
    from facerecognition_amd.head import EmbeddingHead
    from facerecognition_amd.model import FRModel
    from facerecognition_amd.synthetic import synthetic_crops

    def agree(head, model, x):
        emb = model.embed(x, normalize=False)
        feat = model.features(x)
        assert feat.shape == (2, model.feature_dim) and feat.dtype == torch.float32
        with torch.no_grad():
            mine = head.eval()(feat)
        cos = torch.nn.functional.cosine_similarity(mine, emb).cpu().numpy()
        print(f"  {arch}: 1 - cos = {1 - cos}")
        assert np.all(cos >= 1 - 1e-3), cos

    sd = Wt.synth_state_dict(arch)
    model = FRModel(arch, sd)
    assert model.feature_dim == {"resnet50_arcface": 2048, "iresnet100": 25088, "irv1_facenet": 1792}[arch]
    x = torch.from_numpy(synthetic_crops(2, Wt.INPUT_SIZE[arch], seed=3))
    head = EmbeddingHead.for_arch(arch, sd).to(dev)
    agree(head, model, x)
    g = torch.Generator(device="cpu").manual_seed(8)
    with torch.no_grad():  # a "trained" head: every parameter and running statistic moved
        for prm in head.parameters():
            prm.mul_(1 + 0.2 * torch.randn(prm.shape, generator=g).to(dev))
        head.bn_out.bias.add_(0.1 * torch.randn(512, generator=g).to(dev))
        head.bn_out.running_mean.add_(0.1 * torch.randn(512, generator=g).to(dev))
        head.bn_out.running_var.mul_(1.3)
    sd.update(head.reference_state_dict())
    model.load_state_dict(sd)
    agree(head, model, x)
    model.close()


def test_training_loop_learns_and_repeats_bitwise(dev):
    import torch

    from facerecognition_amd.arcmargin import ArcMarginProduct
    from facerecognition_amd.head import EmbeddingHead

    B, K, C, STEPS = 64, 2048, 8, 20
    rng = np.random.default_rng(17)
    centres = rng.standard_normal((C, K))
    labels = np.arange(B) % C
    feats = torch.from_numpy((np.maximum(centres[labels] + 3.0 * rng.standard_normal((B, K)), 0)).astype(np.float32)).to(dev)
    y = torch.from_numpy(labels.astype(np.int64)).to(dev)

    def run():
        torch.manual_seed(3)
        head = EmbeddingHead(K, 512).to(dev).train().seed(99)
        arc = ArcMarginProduct(512, C).to(dev)
        opt = torch.optim.SGD(list(head.parameters()) + list(arc.parameters()), lr=0.002, momentum=0.9)
        losses, trail = [], []
        for _ in range(STEPS):
            opt.zero_grad()
            loss = arc.loss(head(feats), y)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            state = torch.cat([t.detach().reshape(-1) for t in list(head.parameters()) + list(arc.parameters())
                               + [b.float().reshape(-1) for b in head.buffers()]])
            trail.append(hashlib.sha256(state.cpu().numpy().tobytes()).hexdigest())  # every bit of every step
        return losses, trail

    l1, t1 = run()
    l2, t2 = run()
    print("  losses:", [round(v, 4) for v in l1])
    assert np.all(np.isfinite(l1)) and l1[-1] < l1[0], l1
    assert l1 == l2 and t1 == t2 and len(set(t1)) == STEPS
