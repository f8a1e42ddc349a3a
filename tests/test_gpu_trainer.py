"""facerecognition_amd.trainer and facerecognition_amd.optim in a training loop on the GPU: synthetic weights and
``synthetic_crops``, 32 training and 16 validation images of 4 classes, batch 8.

The golden config (tests/golden/configs/arcface_config.yaml) is used as it stands except for ``num_epochs``,
``batch_size`` and ``warmup.epochs`` -- and ``model.freeze_ratio``, which the golden file sets to 0.0 (the whole backbone
trains): the trainer refuses that by design, so the tests set the reference's default fine-tune, 0.8, or 1.0.
No thresholds are tuned here: the comparisons are equalities, orderings (a loss falls, one distance is below another)
and the 5.0 of the config's ``grad_clip.max_norm``.
Measured (MI355X): hand-written loop 34.24 -> below 1e-4 in six steps, both runs bitwise equal; trainer train loss 6.27
-> 5.53 over two epochs, gradient norm 106 at step 1 (clipped to 5.0); after the reload into a fresh engine 1 - cos at
most 5.8e-5 to the trained modules and 0.14 .. 0.33 to the untrained ones; the resumed run bitwise equal.
"""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARCH = "resnet50_arcface"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "configs", "arcface_config.yaml")
REFERENCE_KEYS = {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "scaler_state_dict", "val_acc",
                  "val_loss", "best_val_acc", "best_val_loss", "config", "num_classes", "global_step", "warmup_enabled",
                  "warmup_epochs", "target_lr", "use_amp", "history"}
SEED = 7


@pytest.fixture(scope="module")
def dev():
    import torch

    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def sd():
    from facerecognition_amd import weights as Wt

    return Wt.synth_state_dict(ARCH)


@pytest.fixture(scope="module")
def data():
    from facerecognition_amd.synthetic import synthetic_crops

    x = synthetic_crops(48, 112, seed=21)
    y = np.arange(48) % 4
    return (x[:32], y[:32]), (x[32:], y[32:])


def config(epochs=2, freeze_ratio=0.8, **training):
    from facerecognition_amd.trainer import load_config

    cfg = load_config(GOLDEN)
    cfg["training"].update(num_epochs=epochs, batch_size=8)
    cfg["training"]["warmup"]["epochs"] = 1
    cfg["model"]["freeze_ratio"] = freeze_ratio
    for k, v in training.items():
        cfg["training"][k].update(v)
    return cfg


@pytest.fixture(scope="module")
def engine(sd):
    """One engine for every trainer here: its frozen trunk is what runs bitwise equal."""
    from facerecognition_amd.model import FRModel

    model = FRModel(ARCH, sd)
    yield model
    model.close()


def make_trainer(engine, sd, data, path, **kw):
    from facerecognition_amd.trainer import ArcFaceTrainer

    cfg = kw.pop("cfg", None) or config(**kw)
    return ArcFaceTrainer(cfg, engine, data[0], data[1], checkpoint_dir=str(path), seed=SEED, verbose=False,
                          state_dict=sd)


def snapshot(tr):
    """Every parameter, buffer and optimiser state tensor of a trainer, as numpy arrays by name."""
    import torch

    out = {}
    for name, m in (("layer4", tr.layer4), ("head", tr.head), ("arcface", tr.arcface)):
        if m is None:
            continue
        for k, v in m.state_dict().items():
            out[f"{name}.{k}"] = v.detach().cpu().numpy()
    osd = tr.optimizer.state_dict()
    for i, st in osd["state"].items():
        for k, v in st.items():
            out[f"opt.{i}.{k}"] = torch.as_tensor(v).detach().cpu().numpy()
    out["dropout"] = np.array([tr.head._seed, tr.head._offset], np.uint64)
    return out


def same(a, b):
    return set(a) == set(b) and all(a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.fixture(scope="module")
def straight(engine, sd, data, tmp_path_factory):
    """Two epochs straight through ArcFaceTrainer with the golden config."""
    path = tmp_path_factory.mktemp("straight")
    tr = make_trainer(engine, sd, data, path)
    untrained = snapshot(tr)
    best = tr.train()
    return tr, path, untrained, best


def test_hand_written_loop_with_the_fused_sgd_learns_and_repeats(dev, sd):
    import torch

    from facerecognition_amd import optim as O
    from facerecognition_amd.arcmargin import ArcMarginProduct
    from facerecognition_amd.backbone_train import ResNet50Layer4
    from facerecognition_amd.head import EmbeddingHead
    from facerecognition_amd.model import FRModel
    from facerecognition_amd.synthetic import synthetic_crops

    B, CLS, STEPS = 8, 4, 6
    model = FRModel(ARCH, sd)
    feat = model.features(torch.from_numpy(synthetic_crops(B, 112, seed=11)), at="layer4_in")
    y = torch.arange(B, device=dev) % CLS

    def run():
        torch.manual_seed(3)
        layer = ResNet50Layer4.for_model(sd).to(dev).train()
        head = EmbeddingHead.for_arch(ARCH, sd).to(dev).train().seed(99)
        arc = ArcMarginProduct(512, CLS).to(dev)
        prm = list(layer.parameters()) + list(head.parameters()) + list(arc.parameters())
        opt = O.SGD(prm, lr=0.002, momentum=0.9)  # no clipping
        losses, trail = [], []
        for _ in range(STEPS):
            opt.zero_grad()
            loss = arc.loss(head(layer(feat)), y)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            state = torch.cat([t.detach().float().reshape(-1) for t in prm + list(layer.buffers())])
            trail.append(hashlib.sha256(state.cpu().numpy().tobytes()).hexdigest())
        return losses, trail

    l1, t1 = run()
    l2, t2 = run()
    print("  losses:", [round(v, 4) for v in l1])
    assert np.all(np.isfinite(l1)) and l1[-1] < l1[0], l1
    assert l1 == l2 and t1 == t2 and len(set(t1)) == STEPS
    model.close()


def test_two_epochs_through_the_trainer(straight):
    import torch

    tr, path, untrained, best = straight
    h = tr.history
    print("  history:", {k: [round(float(v), 5) for v in vals] for k, vals in h.items()})
    assert h["epoch"] == [1, 2] and all(len(v) == 2 for v in h.values())
    for k in ("train_loss", "val_loss", "train_acc", "val_acc", "ver_acc"):
        assert np.all(np.isfinite(h[k])), k
    assert h["train_loss"][-1] < h["train_loss"][0]
    assert len(tr.grad_norms) == 4 and tr.global_step == 8  # 32 images, batch 8: four steps an epoch, two epochs
    first = float(tr.first_grad_norm)
    print(f"  gradient norm at step 1 before clipping: {first:.4g}")
    assert first > 5.0  # the clip of the config engages (seed chosen so; see SEED)
    # the LR trail by hand: one warm-up epoch at start + (target - start) * 1 / 1, then StepLR(20, 0.5) after epoch 2
    warm = 0.00001 + (0.01 - 0.00001) * ((0 + 1) / 1)
    assert h["learning_rate"] == [warm, warm * 0.5 ** (1 // 20)]
    assert tr.optimizer.max_norm == 5.0 and tr.use_amp is False and "float32" in tr.mixed_precision_message
    assert best == tr.best_val_acc == max(h["ver_acc"])
    # files: the history and the three kinds of checkpoint, with exactly the reference's keys plus rng_state
    hist = json.load(open(path / "training_history.json"))
    assert set(hist) == {"history", "best_val_acc", "best_val_loss", "total_epochs", "num_classes", "config"}
    assert hist["history"] == h and hist["total_epochs"] == 2 and hist["num_classes"] == 4
    assert set(hist["config"]) == {"model", "training", "arcface"}
    names = sorted(p.name for p in path.glob("*.pth"))
    assert names == ["arcface_best.pth", "arcface_epoch_1.pth", "arcface_epoch_2.pth", "arcface_last.pth"]
    for name in ("arcface_best.pth", "arcface_last.pth", "arcface_epoch_2.pth"):
        ck = torch.load(path / name, map_location="cpu", weights_only=True)
        assert set(ck) == REFERENCE_KEYS | {"rng_state"}, name
        assert set(ck["rng_state"]) == {"shuffle", "augment", "dropout"}
        assert ck["use_amp"] is False and ck["scaler_state_dict"] is None and ck["num_classes"] == 4
        assert ck["warmup_enabled"] is True and ck["warmup_epochs"] == 1 and ck["target_lr"] == 0.01
        assert ck["config"] == tr.config
    last = torch.load(path / "arcface_last.pth", map_location="cpu", weights_only=True)
    assert last["epoch"] == 1 and last["global_step"] == 8 and last["history"] == h
    assert set(last["optimizer_state_dict"]["state"][0]) == {"momentum_buffer"}
    assert not same(snapshot(tr), untrained)


def test_keep_last_n_removes_older_epoch_files(engine, sd, data, tmp_path):
    cfg = config(epochs=3, freeze_ratio=1.0)
    cfg["checkpoint"]["keep_last_n"] = 1
    tr = make_trainer(engine, sd, data, tmp_path, cfg=cfg)
    tr.train()
    assert sorted(p.name for p in tmp_path.glob("arcface_epoch_*.pth")) == ["arcface_epoch_3.pth"]


def test_checkpoint_folds_back_into_a_fresh_engine(straight, sd, data, dev):
    import torch

    from facerecognition_amd import weights as Wt
    from facerecognition_amd.backbone_train import ResNet50Layer4
    from facerecognition_amd.head import EmbeddingHead
    from facerecognition_amd.model import FRModel

    tr, path, _, _ = straight
    ck_sd, _ = Wt.load_checkpoint(str(path / "arcface_last.pth"))  # the existing checkpoint reader
    assert Wt.detect_arch(ck_sd) == ARCH and tuple(ck_sd["arcface.weight"].shape) == (4, 512)
    x = torch.from_numpy(data[1][0][:8])
    fresh_model = FRModel(ARCH, sd)
    feat = fresh_model.features(x, at="layer4_in")
    with torch.no_grad():
        trained = tr.head.eval()(tr.layer4.eval()(feat))
        fresh = EmbeddingHead.for_arch(ARCH, sd).to(dev).eval()(ResNet50Layer4.for_model(sd).to(dev).eval()(feat))
    fresh_model.load_state_dict(ck_sd)
    emb = fresh_model.embed(x, normalize=False)
    cosd = lambda a, b: (1 - torch.nn.functional.cosine_similarity(a, b)).cpu().numpy()
    d_new, d_old = cosd(emb, trained), cosd(emb, fresh)
    print(f"  engine after the reload, 1 - cos to the trained modules {d_new}, to the untrained {d_old}")
    assert np.all(d_new < d_old)
    fresh_model.close()


def test_resume_is_bitwise(straight, engine, sd, data, tmp_path):
    tr2, _, _, _ = straight
    want = snapshot(tr2)
    first = make_trainer(engine, sd, data, tmp_path / "a", epochs=1)
    first.train()
    assert first.history["epoch"] == [1]
    resumed = make_trainer(engine, sd, data, tmp_path / "b")
    resumed.resume_training(tmp_path / "a" / "arcface_last.pth")
    assert resumed.current_epoch == 1 and resumed.global_step == 4 and resumed.history["epoch"] == [1]
    resumed.train()
    got = snapshot(resumed)
    diff = [k for k in want if k not in got or want[k].tobytes() != got[k].tobytes()]
    assert not diff and same(got, want), diff[:5]
    assert resumed.history == tr2.history
    # without the optimizer state the second epoch starts from an empty momentum: a different result
    reset = make_trainer(engine, sd, data, tmp_path / "c")
    reset.resume_training(tmp_path / "a" / "arcface_last.pth", reset_optimizer=True)
    assert reset.get_lr() == 0.01 and reset.current_epoch == 1
    reset.train()
    assert not same(snapshot(reset), want)


def test_early_stopping_stops_after_the_second_epoch(engine, sd, data, tmp_path):
    tr = make_trainer(engine, sd, data, tmp_path, epochs=5, freeze_ratio=1.0,
                      early_stopping=dict(patience=1, min_delta=1e9))  # no loss can improve by 1e9
    tr.train()
    assert tr.history["epoch"] == [1, 2] and tr.early_stopping.early_stop and tr.early_stopping.best_epoch == 0


def test_freeze_ratio_one_trains_head_and_centres_only(engine, sd, data, tmp_path):
    tr = make_trainer(engine, sd, data, tmp_path, freeze_ratio=1.0)
    assert tr.layer4 is None
    before = snapshot(tr)
    tr.train()
    after = snapshot(tr)
    assert not any(k.startswith("layer4") for k in after)
    assert before["head.fc.weight"].tobytes() != after["head.fc.weight"].tobytes()
    assert before["arcface.weight"].tobytes() != after["arcface.weight"].tobytes()
    msd = tr.model_state_dict()
    moved = [k for k in msd if k.startswith("backbone.") and not np.array_equal(msd[k].numpy(), np.asarray(sd[k]))]
    assert not moved, moved[:5]
    assert np.all(np.isfinite(tr.history["train_loss"]))
    with pytest.raises(ValueError, match="layer3"):
        make_trainer(engine, sd, data, tmp_path / "half", freeze_ratio=0.5)
