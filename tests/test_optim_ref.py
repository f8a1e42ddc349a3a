"""tests/optim_ref.py (the numpy float32 specification of the fused optimiser step) against torch.optim on the CPU.

Ten steps on random tensors: ``clip_grad_norm_`` + ``torch.optim.SGD/Adam/AdamW(foreach=False)`` in float64 is the
truth, the same in float32 is the yardstick.  The bound is derived, not chosen: the restatement and torch-float32 are
both float32 evaluations of the same formulas (torch's CPU kernels fuse some multiply-adds, the restatement rounds every
product), so the restatement's error against float64 may be at most 4 times torch-float32's own error on the same
tensor, plus one ulp of the tensor's largest value -- the rule of tests/test_gpu_backbone_train.py.  The ratios are
printed; DESIGN.md §4 "Optimiser step and training loop" records them.
Observed (largest ratio per case): SGD plain 2.92, momentum 1.0, nesterov 1.0, dampening 1.25, weight decay 1.44,
maximize 1.0; Adam 1.93, with L2 1.96; AdamW 2.6, with decay 2.22.
"""
import numpy as np
import pytest
import torch

from tests import optim_ref as R

SIZES = (1, 3, 5, 1023, 4096)
STEPS = 10


def _data(seed):
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    grads = [[(rng.standard_normal(n) * 0.5).astype(np.float32) for n in SIZES] for _ in range(STEPS)]
    return params, grads


def _torch_run(kind, kw, params, grads, dtype):
    prm = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(dtype)) for p in params]
    opt = R.torch_optimizer(kind, prm, **kw)
    norms = []
    for gs in grads:
        for p, g in zip(prm, gs):
            p.grad = torch.from_numpy(g.copy()).to(dtype)  # clip_grad_norm_ scales in place
        norms.append(torch.nn.utils.clip_grad_norm_(prm, R.MAX_NORM, foreach=False).to(torch.float32).item())
        opt.step()
    names = {"sgd": ("momentum_buffer",), "adam": ("exp_avg", "exp_avg_sq"), "adamw": ("exp_avg", "exp_avg_sq")}[kind]
    out = {}
    for i, p in enumerate(prm):
        out[f"p{i}"] = p.detach().numpy().astype(np.float64)
        for n in names:
            if opt.state[p].get(n) is not None:
                out[f"{n}{i}"] = opt.state[p][n].numpy().astype(np.float64)
    return out, norms


@pytest.mark.parametrize("name,kind,kw", R.CASES, ids=[c[0] for c in R.CASES])
def test_restatement_against_torch(name, kind, kw):
    params, grads = _data(sum(map(ord, name)))
    truth, _ = _torch_run(kind, kw, params, grads, torch.float64)
    ref32, norms = _torch_run(kind, kw, params, grads, torch.float32)
    assert min(norms) > R.MAX_NORM  # every step clips
    opt = R.RefOptimizer(kind, params, max_norm=R.MAX_NORM, **kw)
    for gs, norm in zip(grads, norms):
        opt.step(gs, np.float32(norm))
    got = {}
    for i in range(len(params)):
        got[f"p{i}"] = opt.p[i]
        for n, v in opt.state(i).items():
            got[f"{n}{i}"] = v
    assert set(got) == set(truth)
    bad, worst = [], 0.0
    for key in got:
        assert got[key].dtype == np.float32
        ok, ratio = R.error_rule(got[key], ref32[key], truth[key])
        worst = max(worst, ratio if np.isfinite(ratio) and ratio < 1e100 else 0.0)
        if not ok:
            bad.append((key, ratio))
    print(f"  {name}: largest error ratio restatement / torch float32 = {worst:.3g}")
    assert not bad, bad


def test_clip_coefficient_and_skip():
    assert R.clip_coef(np.float32(10.0), None) == 1 and R.clip_coef(np.float32(10.0), 0.0) == 1
    assert R.clip_coef(np.float32(0.5), 1.0) == 1
    c = R.clip_coef(np.float32(10.0), 5.0)
    assert c.dtype == np.float32 and c == np.float32(5.0) / (np.float32(10.0) + np.float32(1e-6))
    assert np.isnan(R.clip_coef(np.float32("nan"), 1.0))
    opt = R.RefOptimizer("adam", [np.ones(3, np.float32)], lr=0.1)
    opt.step([np.ones(3, np.float32)], np.float32(1.7), skip=True)
    assert opt.t == 0 and opt.b1pow == 1.0 and opt.m[0] is None and np.array_equal(opt.p[0], np.ones(3, np.float32))
    opt.step([None], np.float32(0.0))
    assert opt.t == 1 and opt.m[0] is None
