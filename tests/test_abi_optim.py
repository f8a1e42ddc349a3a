"""The fr_optim_* entry points at the C-ABI boundary, without a GPU: declared, exported, bound, and every unsupported
argument refused with FR_ERR_ARG and a message naming the entry point before any HIP call (the pointers below are host
memory and are never dereferenced by a kernel).  Also the optimiser classes' constructors and state_dict layout, and
the trainer's host-side parts: EarlyStopping, the golden config and the warm-up."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from facerecognition_amd import _native as N

NEW = {"fr_optim_workspace": 1, "fr_optim_grad_norm": 15, "fr_optim_step": 20}
INF, NAN = float("inf"), float("nan")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "configs", "arcface_config.yaml")


def _other_message(L):
    L.fr_op_avgpool(None, 1, 1, 1, 8, None, 0, None)  # leaves another entry point's message behind


def _ids(kw):
    return ",".join(f"{k}={v}" for k, v in kw.items())


def test_optim_functions_are_declared_exported_and_bound():
    L = N.lib()
    for name, nargs in NEW.items():
        assert name in N.header_functions(), name
        assert hasattr(L, name) and name in N._SIGS, name
        assert len(N._SIGS[name][1]) == nargs, name
    assert N._SIGS["fr_optim_workspace"][0] is ctypes.c_size_t
    assert (N.FR_OPTIM_SGD, N.FR_OPTIM_ADAM, N.FR_OPTIM_ADAMW) == (0, 1, 2)
    assert (N.FR_OPTIM_NESTEROV, N.FR_OPTIM_MAXIMIZE, N.FR_OPTIM_AMSGRAD, N.FR_OPTIM_SKIP_NONFINITE) == (1, 2, 4, 8)
    assert N.FR_OPTIM_CHUNK == 65536
    assert L.fr_abi_version() == 1  # additive change


def test_workspace():
    L = N.lib()
    assert L.fr_optim_workspace(0) >= 8
    for c in (1, 7, 32, 7813, 2 ** 24):
        w = L.fr_optim_workspace(c)
        assert 8 * c <= w <= 8 * c + 256 and w % 8 == 0
    for bad in (-1, 2 ** 24 + 1):
        _other_message(L)
        assert L.fr_optim_workspace(bad) == 0 and b"fr_optim_workspace" in L.fr_last_error()


class _Args:
    """Three tensors of host memory; every argument of both calls, overridable by name."""

    def __init__(self, kw):
        self.keep = [(ctypes.c_float * 64)() for _ in range(12)]
        addr = [ctypes.addressof(b) for b in self.keep]
        n = kw.pop("n", 3)
        mk = lambda vals: (ctypes.c_void_p * 3)(*vals)
        self.a = dict(n=n, grads=mk(addr[0:3]), params=mk(addr[3:6]), s1=mk(addr[6:9]), s2=mk(addr[9:12]),
                      numel=(ctypes.c_int64 * 3)(5, 64, 1), born=(ctypes.c_int64 * 3)(0, 0, 0),
                      max_norm=5.0, nflags=0, found_inf=None, grad_scale=None, n_groups=1,
                      beta1=(ctypes.c_double * 1)(0.9), beta2=(ctypes.c_double * 1)(0.999), attempt=1,
                      ctrl=addr[0], ws=addr[1], ws_bytes=1 << 20,
                      kind=N.FR_OPTIM_ADAM, lr=1e-3, wd=0.0, momentum=0.0, dampening=0.0, b1=0.9, b2=0.999, eps=1e-8,
                      flags=0, group=0)
        for k, v in kw.items():
            if k.startswith("numel") and k != "numel":  # numel1=-1: one entry of the array
                self.a["numel"][int(k[5:])] = v
            elif k.startswith("null_"):  # null_params1: one NULL entry of a pointer array
                name, i = k[5:-1], int(k[-1])
                self.a[name][i] = None
            elif k == "odd_grad":
                self.a["grads"][v] = addr[0] + 2
            elif k in ("beta1", "beta2"):
                self.a[k] = None if v is None else (ctypes.c_double * 1)(v)
            else:
                self.a[k] = v

    def norm(self, L):
        a = self.a
        return L.fr_optim_grad_norm(a["grads"], a["numel"], a["n"], a["max_norm"], a["nflags"], a["found_inf"],
                                    a["grad_scale"], a["n_groups"], a["beta1"], a["beta2"], a["attempt"], a["ctrl"],
                                    a["ws"], a["ws_bytes"], None)

    def step(self, L):
        a = self.a
        return L.fr_optim_step(a["kind"], a["params"], a["grads"], a["s1"], a["s2"], a["numel"], a["born"], a["n"],
                               a["lr"], a["wd"], a["momentum"], a["dampening"], a["b1"], a["b2"], a["eps"], a["flags"],
                               a["ctrl"], a["group"], a["grad_scale"], None)


LIST_BAD = [dict(n=-1), dict(grads=None), dict(numel=None), dict(numel1=-1), dict(numel0=2 ** 40 + 1), dict(odd_grad=1)]
NORM_BAD = LIST_BAD + [dict(max_norm=NAN), dict(nflags=1), dict(nflags=16), dict(nflags=-1), dict(n_groups=-1),
                       dict(n_groups=33), dict(beta1=None), dict(beta2=None), dict(beta1=1.0), dict(beta1=-0.1),
                       dict(beta2=NAN), dict(beta2=1.5), dict(attempt=0), dict(attempt=-3), dict(ctrl=None),
                       dict(ws=None), dict(ws_bytes=0), dict(ws_bytes=255), dict(ctrl=4), dict(ws=12),
                       dict(found_inf=6), dict(grad_scale=2)]


@pytest.mark.parametrize("kw", NORM_BAD, ids=_ids)
def test_grad_norm_rejects_unsupported_arguments(kw):
    L = N.lib()
    _other_message(L)
    rc = _Args(dict(kw)).norm(L)
    assert rc == N.FR_ERR_ARG and b"fr_optim_grad_norm" in L.fr_last_error(), (kw, rc, L.fr_last_error())


STEP_BAD = LIST_BAD + [dict(kind=3), dict(kind=-1), dict(flags=N.FR_OPTIM_AMSGRAD), dict(flags=8), dict(flags=-1),
                       dict(lr=-1e-3), dict(lr=NAN), dict(lr=INF), dict(eps=-1e-8), dict(eps=NAN), dict(eps=INF),
                       dict(b1=1.0), dict(b1=-0.5), dict(b1=NAN), dict(b2=1.0), dict(b2=NAN), dict(wd=-0.1),
                       dict(wd=NAN), dict(flags=N.FR_OPTIM_NESTEROV), dict(params=None), dict(s1=None), dict(s2=None),
                       dict(null_params1=0), dict(null_s11=0), dict(null_s22=0), dict(group=-1), dict(group=32),
                       dict(ctrl=None), dict(ctrl=4), dict(grad_scale=2),
                       dict(kind=N.FR_OPTIM_SGD, momentum=-0.1), dict(kind=N.FR_OPTIM_SGD, momentum=NAN),
                       dict(kind=N.FR_OPTIM_SGD, dampening=INF),
                       dict(kind=N.FR_OPTIM_SGD, flags=N.FR_OPTIM_NESTEROV),  # no momentum
                       dict(kind=N.FR_OPTIM_SGD, flags=N.FR_OPTIM_NESTEROV, momentum=0.9, dampening=0.1),
                       dict(kind=N.FR_OPTIM_SGD, momentum=0.9, s1=None),
                       dict(kind=N.FR_OPTIM_ADAMW, flags=N.FR_OPTIM_AMSGRAD)]


@pytest.mark.parametrize("kw", STEP_BAD, ids=_ids)
def test_step_rejects_unsupported_arguments(kw):
    L = N.lib()
    _other_message(L)
    rc = _Args(dict(kw)).step(L)
    assert rc == N.FR_ERR_ARG and b"fr_optim_step" in L.fr_last_error(), (kw, rc, L.fr_last_error())


@pytest.mark.filterwarnings("ignore:Detected call of")
def test_module_constructors_and_defaults():
    import torch

    import facerecognition_amd as fra
    from facerecognition_amd import optim as O

    assert (fra.SGD, fra.Adam, fra.AdamW) == (O.SGD, O.Adam, O.AdamW)
    for mine, theirs in ((O.SGD, torch.optim.SGD), (O.Adam, torch.optim.Adam), (O.AdamW, torch.optim.AdamW)):
        assert issubclass(mine, torch.optim.Optimizer) and mine._step_supports_amp_scaling
        got, want = inspect.signature(mine.__init__).parameters, inspect.signature(theirs.__init__).parameters
        for name, prm in want.items():
            if name in ("self", "decoupled_weight_decay"):
                continue
            assert name in got and got[name].kind == prm.kind and got[name].default == prm.default, (mine, name)
        assert got["max_norm"].default is None and got["skip_nonfinite"].default is False
        p = torch.nn.Parameter(torch.zeros(3))
        a, b = mine([p]), theirs([p])
        for key, v in b.defaults.items():  # torch's defaults, key for key
            assert a.defaults[key] == v or key in ("foreach", "fused"), (mine, key)
        assert set(a.param_groups[0]) == set(b.param_groups[0])
        assert a.last_grad_norm is None and a.max_norm is None
    assert O.AdamW([torch.nn.Parameter(torch.zeros(1))]).defaults["weight_decay"] == 1e-2
    for bad in (dict(lr=-1.0), dict(weight_decay=-1.0)):
        for cls in (O.SGD, O.Adam, O.AdamW):
            with pytest.raises(ValueError):
                cls([torch.nn.Parameter(torch.zeros(1))], **bad)
    with pytest.raises(ValueError):
        O.SGD([torch.nn.Parameter(torch.zeros(1))], nesterov=True)
    with pytest.raises(ValueError):
        O.Adam([torch.nn.Parameter(torch.zeros(1))], amsgrad=True)
    with pytest.raises(ValueError):
        O.AdamW([torch.nn.Parameter(torch.zeros(1))], betas=(0.9, 1.0))
    with pytest.raises(ValueError):
        O.Adam([torch.nn.Parameter(torch.zeros(1))], capturable=True)
    with pytest.raises(TypeError):
        O.SGD([torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))])
    with pytest.raises(ValueError):
        O.SGD([dict(params=[torch.nn.Parameter(torch.zeros(1))]) for _ in range(33)])
    # no CPU fallback: a CPU parameter raises at the step, as EmbeddingHead does at its forward
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.ones(4)
    for cls in (O.SGD, O.Adam, O.AdamW):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cls([p], max_norm=5.0).step()
    assert torch.equal(p.detach(), torch.ones(4))
    # torch's schedulers and zero_grad work unchanged
    opt = O.SGD([p], lr=0.1, momentum=0.9)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    opt.zero_grad()
    assert p.grad is None
    sched.step()
    assert opt.param_groups[0]["lr"] == 0.05


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_state_dict_round_trip_with_torch_optim(kind):
    import torch

    from facerecognition_amd import optim as O

    g = torch.Generator().manual_seed(3)
    prm = [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (4, 7)]
    if kind == "sgd":
        kw = dict(lr=0.05, momentum=0.9, weight_decay=5e-4, nesterov=True)
        theirs, mine = torch.optim.SGD(prm, **kw), O.SGD(prm, **kw)
        for p in prm:
            theirs.state[p]["momentum_buffer"] = torch.randn(p.shape, generator=g)
    else:
        kw = dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.02)
        theirs, mine = torch.optim.AdamW(prm, **kw), O.AdamW(prm, **kw)
        for p in prm:
            theirs.state[p].update(step=torch.tensor(3.0), exp_avg=torch.randn(p.shape, generator=g),
                                   exp_avg_sq=torch.rand(p.shape, generator=g))
    sd = theirs.state_dict()
    mine.load_state_dict(sd)  # torch -> fused
    back = mine.state_dict()
    assert back["param_groups"] == sd["param_groups"]
    assert set(back["state"]) == set(sd["state"])
    for i, st in sd["state"].items():
        assert set(back["state"][i]) == set(st)
        for k, v in st.items():
            got = back["state"][i][k]
            assert got.dtype == v.dtype and got.device == v.device and torch.equal(got, v), (i, k)
    if kind == "adamw":  # the counters of the device block: step 3 and the running products by the recurrence
        ctrl = mine._ctrl
        assert float(ctrl[8]) == 3.0 and float(ctrl[9]) == 0.8 * 0.8 * 0.8 and float(ctrl[10]) == 0.99 * 0.99 * 0.99
        assert float(mine.state[prm[0]]["step"]) == 3.0
    fresh = (torch.optim.SGD if kind == "sgd" else torch.optim.AdamW)(prm, **kw)
    fresh.load_state_dict(back)  # fused -> torch
    again = fresh.state_dict()
    for i, st in sd["state"].items():
        for k, v in st.items():
            assert torch.equal(torch.as_tensor(again["state"][i][k]), v), (i, k)
    assert again["param_groups"] == sd["param_groups"]
    if kind == "adamw":
        theirs.state[prm[1]]["step"] = torch.tensor(4.0)
        with pytest.raises(ValueError, match="per param group"):
            mine.load_state_dict(theirs.state_dict())


def test_early_stopping_follows_a_scripted_sequence():
    import facerecognition_amd as fra
    from facerecognition_amd.trainer import EarlyStopping

    assert fra.EarlyStopping is EarlyStopping
    assert list(inspect.signature(EarlyStopping.__init__).parameters)[1:] == ["patience", "min_delta", "mode", "verbose"]
    d = EarlyStopping()
    assert (d.patience, d.min_delta, d.mode, d.verbose, d.counter, d.best_score, d.early_stop, d.best_epoch) == (
        10, 0.001, 'max', True, 0, None, False, 0)
    # mode 'max', patience 2, min_delta 0.01: (score, returned, counter, best_score, best_epoch)
    es = EarlyStopping(patience=2, min_delta=0.01, mode='max', verbose=False)
    script = [(0.50, False, 0, 0.50, 0), (0.505, False, 1, 0.50, 0), (0.52, False, 0, 0.52, 2),
              (0.52, False, 1, 0.52, 2), (0.53, False, 2, 0.52, 2)]
    script[-1] = (0.53, True, 2, 0.52, 2)  # 0.53 is not above 0.52 + 0.01: the second miss stops
    for epoch, (score, ret, counter, best, best_epoch) in enumerate(script):
        assert es(score, epoch) is ret, epoch
        assert (es.counter, es.best_score, es.best_epoch) == (counter, best, best_epoch), epoch
    assert es.early_stop
    es.reset()
    assert (es.counter, es.best_score, es.early_stop, es.best_epoch) == (0, None, False, 0)
    # mode 'min': a loss
    es = EarlyStopping(patience=3, min_delta=0.1, mode='min', verbose=False)
    got = [es(s, e) for e, s in enumerate([2.0, 1.95, 1.8, 1.75, 1.71, 1.70, 1.0])]
    assert got == [False, False, False, False, False, True, False]
    assert es.best_score == 1.0 and es.best_epoch == 6 and es.counter == 0 and es.early_stop


def test_golden_config_parses_and_warms_up_as_the_reference():
    import torch

    from facerecognition_amd import trainer as T

    cfg = T.load_config(GOLDEN)
    assert cfg["model"] == dict(backbone="resnet50", embedding_size=512, pretrained=True, freeze_ratio=0.0)
    assert cfg["arcface"] == dict(margin=0.1, scale=64.0, easy_margin=True)
    tc = cfg["training"]
    assert tc["optimizer"] == dict(type="sgd", lr=0.01, momentum=0.9, weight_decay=0.0005)
    assert tc["warmup"] == dict(enabled=True, epochs=5, start_lr=0.00001)
    assert tc["scheduler"]["type"] == "step" and tc["scheduler"]["step_size"] == 20 and tc["scheduler"]["gamma"] == 0.5
    assert tc["grad_clip"] == dict(enabled=True, max_norm=5.0)
    assert tc["early_stopping"] == dict(enabled=True, patience=15, min_delta=0.0001)
    assert cfg["checkpoint"]["keep_last_n"] == 2 and cfg["mixed_precision"] == dict(enabled=True)
    assert T.load_config(cfg) == cfg and T.load_config(cfg) is not cfg
    # the optimizer, scheduler and warm-up of the config, without a model: setup_optimizer needs only parameters
    t = T.ArcFaceTrainer.__new__(T.ArcFaceTrainer)
    t.config, t.verbose = cfg, False
    p = torch.nn.Parameter(torch.zeros(2))
    t.trainable_parameters = lambda: [p]
    t.setup_optimizer()
    from facerecognition_amd import optim as O
    assert isinstance(t.optimizer, O.SGD) and t.optimizer.max_norm == 5.0
    g = t.optimizer.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"]) == (0.00001, 0.9, 0.0005)
    assert isinstance(t.scheduler, torch.optim.lr_scheduler.StepLR) and t.scheduler_type == "epoch"
    lrs = []
    for epoch in range(7):
        warm = t.adjust_warmup_lr(epoch)
        assert warm == (epoch < 5)
        lrs.append(t.get_lr())
    want = [0.00001 + (0.01 - 0.00001) * ((e + 1) / 5) for e in range(5)]  # the reference's linear rule
    assert lrs[:5] == want and lrs[5] == lrs[6] == 0.01
    np.testing.assert_allclose(want, [0.002008, 0.004006, 0.006004, 0.008002, 0.01], rtol=1e-12)
    # the cosine scheduler's T_max rule and the other optimizers
    cfg2 = T.load_config(cfg)
    cfg2["training"]["scheduler"] = dict(type="cosine", eta_min=1e-5)
    cfg2["training"]["optimizer"] = dict(type="adamw", lr=0.001)
    t.config = cfg2
    t.setup_optimizer()
    assert isinstance(t.optimizer, O.AdamW) and t.optimizer.param_groups[0]["weight_decay"] == 0.01
    assert t.scheduler.T_max == 150 - 5 and t.scheduler.eta_min == 1e-5
    cfg2["training"]["warmup"]["enabled"] = False
    cfg2["training"]["scheduler"] = dict(type="plateau", factor=0.5)
    cfg2["training"]["optimizer"] = dict(type="adam", lr=0.001)
    cfg2["training"]["grad_clip"]["enabled"] = False
    t.setup_optimizer()
    assert isinstance(t.optimizer, O.Adam) and t.optimizer.max_norm is None and t.get_lr() == 0.001
    assert t.scheduler_type == "metric" and t.adjust_warmup_lr(0) is False
    # freeze_ratio: what the reference would leave trainable
    assert T.trainable_layers(0.8)[-1] == "layer4" and T.trainable_layers(1.0) == []
    assert T.trainable_layers(0.5) == ["layer3", "layer4"] and len(T.trainable_layers(0.0)) == 5
