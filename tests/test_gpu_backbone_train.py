"""facerecognition_amd.backbone_train on the GPU: Bottleneck against the same chain of raw C calls (bitwise) and against
the plain-torch float64 block, fr_features_at through ResNet50Layer4 against the engine's own pooled features, and the
layer4 + head + ArcFace training loop with the round trip back into the engine.

Tolerances.  Module against float64: nobody measured it beforehand, so the test measures the same block in torch float32
on the CPU against float64 (max |error| / max |value| per tensor) and allows the device 4 x that: both are float32
evaluations in different summation orders, and 4 covers the order spread without hiding a wrong term.  Both numbers are
printed per tensor.  fr_features_at: 1 - cos against FRModel.features within 4 x the 2.0e-5 the head's round trip
measures for this model (tests/test_gpu_head.py).  The training loop's round trip uses no threshold.
Measured (MI355X; DESIGN.md §4 "Backbone training: layer4"): module against float64 at most 5.0e-7 on the device and
5.4e-7 for torch float32 on the CPU, largest device / CPU ratio 3.7 (conv1.dgamma in eval mode, 2.0e-7 against 5.4e-8);
fr_features_at 1 - cos 3.9e-6 on all three plans; training loop: loss 34.2 -> below 1e-4 in six steps, both runs bitwise
equal; after the reload 1 - cos 2.8e-5 to the trained modules and 0.46 .. 0.61 to the untrained ones.
"""
import hashlib

import numpy as np
import pytest

from tests import conv_train_calls as C
from tests import conv_train_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda", 0)


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def hand_block(dev, case, batch, train_bn):
    """The chain of raw C calls of one Bottleneck, forward and backward (bottleneck_ref's order); bottleneck_ref's dict."""
    fl = 1 if batch else 0
    x, s, down = case["x"], case["stride"], "down" in case
    p = lambda n: case[n]
    st = lambda Z, n: C.bn_stats(dev, Z, p(n)["gamma"], p(n)["beta"], p(n)["rm"], p(n)["rv"], fl, R.EPS_BN, R.MOM)
    Z1 = C.conv_forward(dev, x, p("conv1")["W"], 1, 1)
    s1 = st(Z1, "conv1")
    Z2 = C.conv_forward(dev, Z1, p("conv2")["W"], 3, s, s1["scale"], s1["shift"], 1)
    s2 = st(Z2, "conv2")
    Z3 = C.conv_forward(dev, Z2, p("conv3")["W"], 1, 1, s2["scale"], s2["shift"], 1)
    s3 = st(Z3, "conv3")
    if down:
        Zd = C.conv_forward(dev, x, p("down")["W"], 1, s)
        sd = st(Zd, "down")
        Rs = C.bn_act_forward(dev, Zd, sd["scale"], sd["shift"])
    else:
        Rs = x
    Y = C.bn_act_forward(dev, Z3, s3["scale"], s3["shift"], Rs, 2)
    o3 = C.bn_act_backward(dev, case["dY"], Z3, s3, p("conv3")["gamma"], Rs, fl | 2, want_res=True, want_affine=train_bn)
    c3 = C.conv_backward(dev, Z2, p("conv3")["W"], 1, 1, o3["dZ"], s2["scale"], s2["shift"], 1)
    o2 = C.bn_act_backward(dev, c3["dA"], Z2, s2, p("conv2")["gamma"], None, fl | 2, want_affine=train_bn, alias=True)
    c2 = C.conv_backward(dev, Z1, p("conv2")["W"], 3, s, o2["dZ"], s1["scale"], s1["shift"], 1)
    o1 = C.bn_act_backward(dev, c2["dA"], Z1, s1, p("conv1")["gamma"], None, fl | 2, want_affine=train_bn, alias=True)
    c1 = C.conv_backward(dev, x, p("conv1")["W"], 1, 1, o1["dZ"])
    out = dict(Y=Y)
    parts = dict(conv1=(c1, o1, s1), conv2=(c2, o2, s2), conv3=(c3, o3, s3))
    if down:
        od = C.bn_act_backward(dev, o3["dRes"], Zd, sd, p("down")["gamma"], None, fl, want_affine=train_bn, alias=True)
        cd = C.conv_backward(dev, x, p("down")["W"], 1, s, od["dZ"])
        parts["down"] = (cd, od, sd)
        out["dX"] = c1["dA"] + cd["dA"]
    else:
        out["dX"] = c1["dA"] + o3["dRes"]
    for n, (c, o, stt) in parts.items():
        out[n] = dict(dW=c["dW"], rm=stt["rm"], rv=stt["rv"])
        if train_bn:
            out[n].update(dgamma=o["dgamma"], dbeta=o["dbeta"])
    return out


def module_block(dev, case, mode):
    """The Bottleneck module on the same values; bottleneck_ref's dict (float32 numpy)."""
    import torch

    from facerecognition_amd.backbone_train import Bottleneck

    k = R.BLOCK_CASES
    cfg = next(v for v in k.values() if v["down"] == ("down" in case))
    blk = Bottleneck(cfg["Cin"], cfg["P"], cfg["stride"], cfg["down"], R.EPS_BN, R.MOM).to(dev)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)
    pairs = dict(zip(R.CONVS, zip(blk._convs(), blk._bns())))
    with torch.no_grad():
        for n, (conv, bn) in pairs.items():
            conv.weight.copy_(t(case[n]["W"]).permute(0, 3, 1, 2))
            bn.weight.copy_(t(case[n]["gamma"])); bn.bias.copy_(t(case[n]["beta"]))
            bn.running_mean.copy_(t(case[n]["rm"])); bn.running_var.copy_(t(case[n]["rv"]))
            assert conv.weight.permute(0, 2, 3, 1).is_contiguous()
    blk.train()
    if mode == "eval":
        blk.eval()
    elif mode == "freeze_bn":
        blk.freeze_bn()
    x = t(case["x"]).requires_grad_(True)
    y = blk(x)
    y.backward(t(case["dY"]))
    torch.cuda.synchronize()
    g = lambda v: v.detach().cpu().numpy()
    out = dict(Y=g(y), dX=g(x.grad))
    for n, (conv, bn) in pairs.items():
        out[n] = dict(dW=np.ascontiguousarray(g(conv.weight.grad).transpose(0, 2, 3, 1)), rm=g(bn.running_mean), rv=g(bn.running_var))
        if mode != "freeze_bn":
            out[n].update(dgamma=g(bn.weight.grad), dbeta=g(bn.bias.grad))
        else:
            assert bn.weight.grad is None and bn.bias.grad is None
        assert int(bn.num_batches_tracked) == (1 if mode == "train" else 0)
    return out


@pytest.mark.parametrize("name", list(R.BLOCK_CASES))
@pytest.mark.parametrize("mode", ["train", "eval", "freeze_bn"])
def test_bottleneck_against_the_raw_calls_and_float64(dev, name, mode):
    import torch

    case = R.make_block_case(R.BLOCK_SEEDS[name], **R.BLOCK_CASES[name])
    batch = mode == "train"
    mod = dict(R.flat_items(module_block(dev, case, mode)))
    hand = dict(R.flat_items(hand_block(dev, case, batch, mode != "freeze_bn")))
    assert set(mod) == set(hand)
    for key in mod:  # bitwise
        assert same(mod[key].astype(np.float32), hand[key].astype(np.float32)), key
    if not batch:  # running statistics bitwise untouched
        for n in R.CONVS:
            if n in case:
                assert same(mod[f"{n}.rm"].astype(np.float32), case[n]["rm"]) and same(mod[f"{n}.rv"].astype(np.float32), case[n]["rv"])
    want = dict(R.flat_items(R.torch_bottleneck(case, batch, torch.float64)))
    cpu32 = dict(R.flat_items(R.torch_bottleneck(case, batch, torch.float32)))
    bad = []
    for key in mod:
        e_cpu, e_dev = R.rel_err(cpu32[key], want[key]), R.rel_err(mod[key], want[key])
        print(f"  {name} {mode} {key}: torch float32 on the CPU {e_cpu:.3g}, device {e_dev:.3g}")
        if e_dev > 4 * e_cpu:
            bad.append((key, e_cpu, e_dev))
    assert not bad, bad


@pytest.mark.parametrize("plan", ["default", "unfused", "chain"])
def test_features_at_feeds_layer4(dev, plan):
    import torch

    from facerecognition_amd import _native as NL
    from facerecognition_amd import weights as Wt
    from facerecognition_amd.backbone_train import ResNet50Layer4
    from facerecognition_amd.model import FRModel
    from facerecognition_amd.synthetic import synthetic_crops

    arch = "resnet50_arcface"
    sd = Wt.synth_state_dict(arch)
    model = FRModel(arch, sd)
    if plan == "unfused":
        model.set_option(NL.FR_OPT_FUSED_MASK, 0)
    elif plan == "chain":  # the layer3 chain kernel forced on, and nothing else fused
        model.set_option(NL.FR_OPT_STAGE, 2)
        model.set_option(NL.FR_OPT_FUSED_MASK, 16)
    x = torch.from_numpy(synthetic_crops(3, Wt.INPUT_SIZE[arch], seed=3))
    feat = model.features(x, at="layer4_in")
    assert feat.shape == (3, 7, 7, 1024) and feat.dtype == torch.float32 and feat.is_contiguous()
    assert same(model.features(x, at="layer4_in").cpu().numpy(), feat.cpu().numpy())
    want = model.features(x)
    layer = ResNet50Layer4.for_model(sd).to(dev).eval()
    with torch.no_grad():
        mine = layer(feat)
    assert mine.shape == want.shape == (3, 2048)
    cos = torch.nn.functional.cosine_similarity(mine, want).cpu().numpy()
    print(f"  {plan}: 1 - cos = {1 - cos}")
    assert np.all(1 - cos <= 4 * 2.0e-5), 1 - cos
    with pytest.raises(ValueError):
        model.features(x, at="layer3_in")
    model.close()
    if plan == "default":  # the other architectures have no such cut
        other = FRModel.synthetic("irv1_facenet")
        with pytest.raises(RuntimeError, match="fr_features_at"):
            other.features(torch.from_numpy(synthetic_crops(1, 160, seed=3)), at="layer4_in")
        other.close()


def test_training_loop_learns_repeats_and_folds_back(dev):
    import torch

    from facerecognition_amd import weights as Wt
    from facerecognition_amd.arcmargin import ArcMarginProduct
    from facerecognition_amd.backbone_train import ResNet50Layer4
    from facerecognition_amd.head import EmbeddingHead
    from facerecognition_amd.model import FRModel
    from facerecognition_amd.synthetic import synthetic_crops

    arch, B, CLS, STEPS = "resnet50_arcface", 8, 4, 6
    sd = Wt.synth_state_dict(arch)
    model = FRModel(arch, sd)
    x = torch.from_numpy(synthetic_crops(B, Wt.INPUT_SIZE[arch], seed=11))
    feat = model.features(x, at="layer4_in")
    y = torch.arange(B, device=dev) % CLS

    def run(freeze=False, steps=STEPS):
        torch.manual_seed(3)
        layer = ResNet50Layer4.for_model(sd).to(dev).train()
        head = EmbeddingHead.for_arch(arch, sd).to(dev).train().seed(99)
        if freeze:
            layer.freeze_bn()
        arc = ArcMarginProduct(512, CLS).to(dev)
        prm = [q for q in list(layer.parameters()) + list(head.parameters()) + list(arc.parameters()) if q.requires_grad]
        opt = torch.optim.SGD(prm, lr=0.002, momentum=0.9)
        losses, trail = [], []
        for _ in range(steps):
            opt.zero_grad()
            loss = arc.loss(head(layer(feat)), y)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            state = torch.cat([t.detach().float().reshape(-1) for t in list(layer.parameters()) + list(layer.buffers())
                               + list(head.parameters()) + list(arc.parameters())])
            trail.append(hashlib.sha256(state.cpu().numpy().tobytes()).hexdigest())  # every bit of every step
        return layer, head, losses, trail

    layer, head, l1, t1 = run()
    _, _, l2, t2 = run()
    print("  losses:", [round(v, 4) for v in l1])
    assert np.all(np.isfinite(l1)) and l1[-1] < l1[0], l1
    assert l1 == l2 and t1 == t2 and len(set(t1)) == STEPS
    assert all(q.grad is not None and bool(torch.any(q.grad != 0)) for q in layer.parameters())  # layer4 moved

    # back into the engine: its new embeddings are closer to the trained modules' output than to the untrained ones'
    with torch.no_grad():
        trained = head.eval()(layer.eval()(feat))
        fresh = EmbeddingHead.for_arch(arch, sd).to(dev).eval()(ResNet50Layer4.for_model(sd).to(dev).eval()(feat))
    new_sd = dict(sd)
    new_sd.update(layer.reference_state_dict())
    new_sd.update(head.reference_state_dict())
    model.load_state_dict(new_sd)
    emb = model.embed(x, normalize=False)
    cosd = lambda a, b: (1 - torch.nn.functional.cosine_similarity(a, b)).cpu().numpy()
    d_new, d_old = cosd(emb, trained), cosd(emb, fresh)
    print(f"  engine after the reload, 1 - cos to the trained modules {d_new}, to the untrained {d_old}")
    assert np.all(d_new < d_old)
    model.close()

    # freeze_bn: no running statistic moves, bit for bit
    before = {k: v.clone() for k, v in ResNet50Layer4.for_model(sd).state_dict().items() if "running" in k or "tracked" in k}
    frozen, _, lf, _ = run(freeze=True, steps=2)
    assert np.all(np.isfinite(lf))
    after = frozen.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k].cpu(), v), k
    assert all(q.grad is None for blk in frozen.blocks for bn in blk._bns() for q in bn.parameters())
