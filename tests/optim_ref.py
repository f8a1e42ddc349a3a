"""numpy float32 restatement of the fused optimiser step (facerecognition_amd.optim / csrc/optim.hip): the specification.

It takes the global gradient norm as an input (a float32), applies torch's clip coefficient and then torch's
single-tensor SGD / Adam / AdamW formulas in torch's operation order.  Every operation is one float32 numpy operation,
so every product is rounded before it is added; numpy's float32 sqrt and divide are correctly rounded.  The running
products beta^t are Python doubles advanced by ``pow *= beta``, as the device keeps them.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32


def clip_coef(norm, max_norm):
    """torch's clip_grad_norm_ coefficient in float32; max_norm None or <= 0: 1."""
    if max_norm is None or not max_norm > 0:
        return f32(1.0)
    c = f32(max_norm) / (f32(norm) + f32(1e-6))
    return f32(1.0) if c > f32(1.0) else c  # NaN stays NaN


def grad_norm64(grads, grad_scale=None):
    """The float64 norm of a list of float32 gradients (what the device norm is compared with)."""
    total = 0.0
    for g in grads:
        g = np.asarray(g, np.float32)
        if grad_scale is not None:
            g = g / f32(grad_scale)
        total += float(np.sum(g.astype(np.float64) ** 2))
    return float(np.sqrt(total))


class RefOptimizer:
    """kind 'sgd' | 'adam' | 'adamw' over a list of float32 arrays (copied).  ``step(grads, norm)``: grads is a list with
    None for an absent gradient; norm is the global norm of the (unscaled) gradients as a float32."""

    def __init__(self, kind, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
                 maximize=False, betas=(0.9, 0.999), eps=1e-8, max_norm=None):
        self.kind = kind
        self.p = [np.array(p, dtype=np.float32, copy=True) for p in params]
        self.lr, self.momentum, self.dampening, self.weight_decay = float(lr), float(momentum), float(dampening), float(weight_decay)
        self.nesterov, self.maximize = bool(nesterov), bool(maximize)
        self.beta1, self.beta2, self.eps = float(betas[0]), float(betas[1]), float(eps)
        self.max_norm = max_norm
        self.buf = [None] * len(self.p)      # momentum_buffer
        self.m = [None] * len(self.p)        # exp_avg
        self.v = [None] * len(self.p)        # exp_avg_sq
        self.t = 0
        self.b1pow = 1.0
        self.b2pow = 1.0

    def step(self, grads, norm, grad_scale=None, skip=False):
        if skip:
            return
        clip = clip_coef(norm, self.max_norm)
        self.t += 1
        self.b1pow *= self.beta1
        self.b2pow *= self.beta2
        for i, g in enumerate(grads):
            if g is None or self.p[i].size == 0:
                continue
            g = np.asarray(g, np.float32)
            if grad_scale is not None:
                g = g / f32(grad_scale)
            g = g * clip
            if self.maximize:
                g = -g
            if self.kind == "sgd":
                self._sgd(i, g)
            else:
                self._adam(i, g)

    def _sgd(self, i, g):
        p = self.p[i]
        if self.weight_decay != 0:
            g = g + f32(self.weight_decay) * p
        if self.momentum != 0:
            if self.buf[i] is None:
                self.buf[i] = g.copy()
            else:
                self.buf[i] = self.buf[i] * f32(self.momentum) + f32(1.0 - self.dampening) * g
            g = g + f32(self.momentum) * self.buf[i] if self.nesterov else self.buf[i]
        self.p[i] = p + f32(-self.lr) * g

    def _adam(self, i, g):
        p = self.p[i]
        if self.m[i] is None:
            self.m[i] = np.zeros_like(p)
            self.v[i] = np.zeros_like(p)
        if self.weight_decay != 0:
            if self.kind == "adamw":
                p = p * f32(1.0 - self.lr * self.weight_decay)
            else:
                g = g + f32(self.weight_decay) * p
        w = f32(1.0 - self.beta1)
        diff = g - self.m[i]
        self.m[i] = self.m[i] + w * diff if w < f32(0.5) else g - diff * (f32(1.0) - w)
        self.v[i] = self.v[i] * f32(self.beta2) + (f32(1.0 - self.beta2) * g) * g
        bc1 = 1.0 - self.b1pow
        bc2 = 1.0 - self.b2pow
        neg_step = f32(-(self.lr / bc1))
        bc2_sqrt = f32(np.sqrt(np.float64(bc2)))
        denom = np.sqrt(self.v[i]) / bc2_sqrt + f32(self.eps)
        self.p[i] = p + (neg_step * self.m[i]) / denom

    def state(self, i):
        """{name: array} of parameter i in torch's state names."""
        if self.kind == "sgd":
            return {} if self.buf[i] is None else {"momentum_buffer": self.buf[i]}
        return {} if self.m[i] is None else {"exp_avg": self.m[i], "exp_avg_sq": self.v[i]}


# Hyper-parameter cases shared by the CPU and the GPU tests: (name, kind, kwargs)
CASES = [
    ("sgd_plain", "sgd", dict(lr=0.1)),
    ("sgd_momentum", "sgd", dict(lr=0.1, momentum=0.9)),
    ("sgd_nesterov", "sgd", dict(lr=0.1, momentum=0.9, nesterov=True)),
    ("sgd_dampening", "sgd", dict(lr=0.1, momentum=0.9, dampening=0.3)),
    ("sgd_wd", "sgd", dict(lr=0.1, momentum=0.9, weight_decay=5e-4)),
    ("sgd_maximize", "sgd", dict(lr=0.1, momentum=0.9, maximize=True)),
    ("adam", "adam", dict(lr=1e-2)),
    ("adam_wd", "adam", dict(lr=1e-2, weight_decay=1e-2)),
    ("adamw", "adamw", dict(lr=1e-2, weight_decay=0.0)),
    ("adamw_wd", "adamw", dict(lr=1e-2, weight_decay=1e-2)),
]
MAX_NORM = 1.0  # every case clips at this norm; the test gradients have a larger one


def torch_optimizer(kind, params, **kw):
    """torch.optim's single-tensor (foreach=False) optimiser for a case."""
    import torch
    cls = {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "adamw": torch.optim.AdamW}[kind]
    return cls(params, foreach=False, **kw)


def error_rule(got, ref32, truth64):
    """The bound of tests/test_gpu_backbone_train.py: the error of ``got`` against the float64 truth may be at most 4
    times torch-float32's own error on the same tensors, plus one ulp of the value.  Returns (ok, ratio) with ratio =
    max err_got / max(err_ref32, tiny) for the record."""
    got = np.asarray(got, np.float64)
    ref32 = np.asarray(ref32, np.float64)
    truth = np.asarray(truth64, np.float64)
    if got.size == 0:
        return True, 0.0
    err_got = np.abs(got - truth).max()
    err_ref = np.abs(ref32 - truth).max()
    ulp = float(np.spacing(np.float32(np.abs(truth).max())))
    ok = err_got <= 4.0 * err_ref + ulp
    return bool(ok), float(err_got / max(err_ref, 1e-300))
