"""SGD, Adam and AdamW with gradient clipping as one fused device step (libfrhip's fr_optim_* entry points).

``opt.step()`` is ``torch.nn.utils.clip_grad_norm_(params, max_norm)`` followed by ``torch.optim.SGD/Adam/AdamW.step()``
in two stages on the caller's stream: the global L2 norm of every gradient (all param groups together), then one update
pass per param group that applies torch's single-tensor formulas in torch's operation order, every product rounded.
The clip coefficient, the skip decision (``found_inf`` / ``skip_nonfinite``) and the step counters stay on the device:
a step never synchronises.  Everything is bitwise repeatable (no floating-point atomics, fixed summation orders).

The classes subclass ``torch.optim.Optimizer`` and keep torch's constructor arguments, ``param_groups`` and
``state_dict()`` layout (``momentum_buffer``; ``step``, ``exp_avg``, ``exp_avg_sq``), so torch's LR schedulers,
``zero_grad`` and checkpoints written by or for ``torch.optim`` work unchanged.  ``torch.amp.GradScaler`` hands its
``grad_scale`` and ``found_inf`` to the step (``_step_supports_amp_scaling``), as it does to torch's fused optimisers.
Two differences from torch, both consequences of keeping the counters on the device: the step count of Adam / AdamW
is kept per param group, not per parameter (``state[p]["step"]`` is a live device view of it; ``state_dict()`` turns
it into torch's CPU scalar, which synchronises), and ``amsgrad``, ``capturable``, ``differentiable``, sparse gradients
and non-float32 parameters are refused.  There is no CPU fallback: a CPU parameter raises.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from . import _native as N

_HEAD = 8  # the control block in doubles: 8 for the head, 8 per param group (fr_optim_ctrl_head / fr_optim_group_state)
_STEP, _B1POW, _B2POW, _LAST_OK, _PREV_OK = 0, 1, 2, 3, 4


def _chunks(numel: int) -> int:
    return (numel + N.FR_OPTIM_CHUNK - 1) // N.FR_OPTIM_CHUNK


def _dense_like(p: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """t in p's memory layout (the kernels walk storage order)."""
    if t.stride() == p.stride() or t.numel() <= 1:
        return t
    return torch.empty_like(p, memory_format=torch.preserve_format).copy_(t)


class _FusedOptimizer(torch.optim.Optimizer):
    _step_supports_amp_scaling = True
    _kind = N.FR_OPTIM_SGD

    def __init__(self, params, defaults, max_norm, skip_nonfinite):
        if max_norm is not None and not float(max_norm) == float(max_norm):
            raise ValueError("max_norm must not be NaN")
        super().__init__(params, defaults)
        self.max_norm = None if max_norm is None else float(max_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._ctrl: Optional[torch.Tensor] = None
        self._attempt = 0
        self._born = {}  # parameter -> the attempt at which its state was created (absent: loaded, 0)

    # -- parameters -----------------------------------------------------------------------------------------------
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        name = type(self).__name__
        if len(self.param_groups) > N.FR_OPTIM_MAX_GROUPS:
            raise ValueError(f"{name}: at most {N.FR_OPTIM_MAX_GROUPS} param groups")
        for p in self.param_groups[-1]["params"]:
            if p.dtype != torch.float32 or p.is_sparse:
                raise TypeError(f"{name}: dense float32 parameters expected, got {p.dtype}")
            if not torch._prims_common.is_non_overlapping_and_dense(p):
                raise ValueError(f"{name}: a parameter must be dense in memory (contiguous in some dimension order)")

    def _device(self):
        for g in self.param_groups:
            for p in g["params"]:
                return p.device
        raise RuntimeError(f"{type(self).__name__}: no parameters")

    # -- the device control block ---------------------------------------------------------------------------------
    def _fresh_ctrl(self, steps):
        host = torch.zeros(_HEAD * (1 + len(steps)), dtype=torch.float64)
        for gi, (t, b1, b2) in enumerate(steps):
            b1pow = b2pow = 1.0
            for _ in range(int(t)):  # the device's recurrence, so a restored counter continues bit for bit
                b1pow *= b1
                b2pow *= b2
            e = _HEAD * (1 + gi)
            host[e + _STEP], host[e + _B1POW], host[e + _B2POW] = float(int(t)), b1pow, b2pow
        return host

    def _betas(self, group):
        return tuple(float(b) for b in group.get("betas", (0.0, 0.0)))

    def _ensure_ctrl(self):
        G = len(self.param_groups)
        if self._ctrl is not None and self._ctrl.numel() == _HEAD * (1 + G):
            return self._ctrl
        dev = self._device()
        old = self._ctrl
        have = 0 if old is None else old.numel() // _HEAD - 1
        fresh = self._fresh_ctrl([(0,) + self._betas(g) for g in self.param_groups]).to(dev)
        if old is not None:  # groups added after the first step: the earlier counters stay
            fresh[:_HEAD * (1 + have)].copy_(old)
        self._ctrl = fresh
        self._bind_steps()
        return fresh

    def _bind_steps(self):
        """state[p]['step'] of every Adam parameter is a view of its group's device counter."""
        if self._kind == N.FR_OPTIM_SGD or self._ctrl is None:
            return
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                if "exp_avg" in self.state.get(p, {}):
                    self.state[p]["step"] = self._ctrl[_HEAD * (1 + gi) + _STEP]

    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """The global gradient norm of the last step before clipping, what ``clip_grad_norm_`` would have returned: a
        0-dim float32 device tensor (reading it synchronises), or None before the first step."""
        if self._ctrl is None or self._attempt == 0:
            return None
        return self._ctrl.view(torch.float32)[0].clone()

    @property
    def last_step_skipped(self) -> Optional[torch.Tensor]:
        """0-dim int32 device tensor: 1 when the last step was skipped (found_inf, or skip_nonfinite and a non-finite norm)."""
        if self._ctrl is None or self._attempt == 0:
            return None
        return self._ctrl.view(torch.int32)[2].clone()

    # -- state_dict in torch's layout -----------------------------------------------------------------------------
    def state_dict(self):
        sd = super().state_dict()
        if self._ctrl is None:
            return sd
        host = self._ctrl.cpu()  # synchronises
        index = {}
        for gi, (g, packed) in enumerate(zip(self.param_groups, sd["param_groups"])):
            for p, i in zip(g["params"], packed["params"]):
                index[i] = (gi, p)
        state = {}
        for i, st in sd["state"].items():
            st = dict(st)
            gi, p = index[i]
            e = _HEAD * (1 + gi)
            if "step" in st:
                st["step"] = torch.tensor(float(host[e + _STEP]), dtype=torch.float32)
            if self._kind == N.FR_OPTIM_SGD and self._born.get(p, 0) > int(host.view(torch.int64)[e + _LAST_OK]):
                st.pop("momentum_buffer", None)  # created in a skipped step: not yet a momentum
            if st:
                state[i] = st
        sd["state"] = state
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if len(self.param_groups) > N.FR_OPTIM_MAX_GROUPS:
            raise ValueError(f"{type(self).__name__}: at most {N.FR_OPTIM_MAX_GROUPS} param groups")
        steps = []
        for g in self.param_groups:
            seen = {float(self.state[p]["step"]) for p in g["params"] if "step" in self.state.get(p, {})}
            if len(seen) > 1:
                raise ValueError(f"{type(self).__name__}: the step count is kept per param group, but the loaded "
                                 f"parameters of one group disagree: {sorted(seen)}")
            steps.append((seen.pop() if seen else 0,) + self._betas(g))
        for g in self.param_groups:
            for p in g["params"]:
                st = self.state.get(p, {})
                for k in ("momentum_buffer", "exp_avg", "exp_avg_sq"):
                    if st.get(k) is not None:
                        st[k] = _dense_like(p, st[k].to(device=p.device, dtype=torch.float32))
                    elif k in st:
                        del st[k]
        self._ctrl = self._fresh_ctrl(steps).to(self._device())
        self._attempt = 0
        self._born = {}
        self._bind_steps()

    # -- the step -------------------------------------------------------------------------------------------------
    def _state_for(self, group, p):  # -> (state1, state2), creating them
        raise NotImplementedError

    def _hyper(self, group):  # -> (lr, weight_decay, momentum, dampening, beta1, beta2, eps, flags)
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        name = type(self).__name__
        for group in self.param_groups:
            for p in group["params"]:
                if not p.is_cuda:
                    raise RuntimeError(f"{name} needs ROCm GPU parameters; there is deliberately no CPU fallback")
        ctrl = self._ensure_ctrl()
        dev = ctrl.device
        self._attempt += 1
        live = []  # per group: [(p, g)]
        for group in self.param_groups:
            rows = []
            for p in group["params"]:
                g = p.grad
                if g is None or p.numel() == 0:
                    continue
                if g.is_sparse:
                    raise RuntimeError(f"{name} does not support sparse gradients")
                if g.dtype != torch.float32 or g.device != p.device or p.device != dev:
                    raise TypeError(f"{name}: float32 gradients on the parameters' device expected")
                rows.append((p, _dense_like(p, g)))
            live.append(rows)

        def scalar(t, what):
            if t is None:
                return None
            if not (isinstance(t, torch.Tensor) and t.numel() == 1):
                raise TypeError(f"{name}: {what} must be a one-element tensor")
            return t.to(device=dev, dtype=torch.float32)

        found_inf = scalar(getattr(self, "found_inf", None), "found_inf")
        grad_scale = scalar(getattr(self, "grad_scale", None), "grad_scale")

        L = N.lib()
        stream = N.stream_ptr(dev)
        grads = [g for rows in live for _, g in rows]
        n = len(grads)
        n_chunks = sum(_chunks(g.numel()) for g in grads)
        nbytes = L.fr_optim_workspace(n_chunks)
        if nbytes == 0:
            N.check(N.FR_ERR_ARG, "fr_optim_workspace")
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        G = len(self.param_groups)
        b1 = (ctypes.c_double * G)(*[self._betas(g)[0] for g in self.param_groups])
        b2 = (ctypes.c_double * G)(*[self._betas(g)[1] for g in self.param_groups])
        gp = (ctypes.c_void_p * max(n, 1))(*[g.data_ptr() for g in grads])
        gn = (ctypes.c_int64 * max(n, 1))(*[g.numel() for g in grads])
        flags = N.FR_OPTIM_SKIP_NONFINITE if self.skip_nonfinite else 0
        N.check(L.fr_optim_grad_norm(gp, gn, n, -1.0 if self.max_norm is None else self.max_norm, flags,
                                     N.ptr(found_inf), N.ptr(grad_scale), G, b1, b2, self._attempt, N.ptr(ctrl),
                                     N.ptr(ws), nbytes, stream), "fr_optim_grad_norm")
        for gi, (group, rows) in enumerate(zip(self.param_groups, live)):
            if not rows:
                continue
            lr, wd, mom, damp, beta1, beta2, eps, hflags = self._hyper(group)
            states = [self._state_for(group, p) for p, _ in rows]
            m = len(rows)
            arr = lambda vals: (ctypes.c_void_p * m)(*vals)
            N.check(L.fr_optim_step(self._kind, arr([p.data_ptr() for p, _ in rows]),
                                    arr([g.data_ptr() for _, g in rows]),
                                    arr([N.ptr(s1) for s1, _ in states]), arr([N.ptr(s2) for _, s2 in states]),
                                    (ctypes.c_int64 * m)(*[p.numel() for p, _ in rows]),
                                    (ctypes.c_int64 * m)(*[self._born.get(p, 0) for p, _ in rows]), m,
                                    lr, wd, mom, damp, beta1, beta2, eps, hflags, N.ptr(ctrl), gi, N.ptr(grad_scale),
                                    stream), "fr_optim_step")
        return loss


class SGD(_FusedOptimizer):
    """``torch.optim.SGD`` (momentum, dampening, weight_decay, nesterov, maximize) with ``max_norm`` clipping fused in."""
    _kind = N.FR_OPTIM_SGD

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None, max_norm=None, skip_nonfinite=False):
        if isinstance(lr, torch.Tensor):
            lr = float(lr)
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if differentiable:
            raise ValueError("SGD: differentiable=True is not supported")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize, foreach=None, differentiable=False, fused=None)
        super().__init__(params, defaults, max_norm, skip_nonfinite)

    def _hyper(self, group):
        flags = (N.FR_OPTIM_NESTEROV if group.get("nesterov", False) else 0) | \
                (N.FR_OPTIM_MAXIMIZE if group.get("maximize", False) else 0)
        return (float(group["lr"]), float(group["weight_decay"]), float(group["momentum"]), float(group["dampening"]),
                0.0, 0.0, 0.0, flags)

    def _state_for(self, group, p):
        if group["momentum"] == 0:
            return None, None
        st = self.state[p]
        if st.get("momentum_buffer") is None:
            st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            self._born[p] = self._attempt
        return st["momentum_buffer"], None


class Adam(_FusedOptimizer):
    """``torch.optim.Adam`` (L2 weight decay added to the gradient) with ``max_norm`` clipping fused in."""
    _kind = N.FR_OPTIM_ADAM

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *,
                 foreach=None, maximize=False, capturable=False, differentiable=False, fused=None,
                 max_norm=None, skip_nonfinite=False):
        name = type(self).__name__
        if isinstance(lr, torch.Tensor):
            lr = float(lr)
        betas = tuple(float(b) for b in betas)
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if eps < 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if amsgrad:
            raise ValueError(f"{name}: amsgrad is not supported")
        if capturable or differentiable:
            raise ValueError(f"{name}: capturable and differentiable are not supported")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=maximize,
                        foreach=None, capturable=False, differentiable=False, fused=None,
                        decoupled_weight_decay=self._kind == N.FR_OPTIM_ADAMW)
        super().__init__(params, defaults, max_norm, skip_nonfinite)

    def _hyper(self, group):
        flags = (N.FR_OPTIM_MAXIMIZE if group.get("maximize", False) else 0) | \
                (N.FR_OPTIM_AMSGRAD if group.get("amsgrad", False) else 0)
        beta1, beta2 = self._betas(group)
        return float(group["lr"]), float(group["weight_decay"]), 0.0, 0.0, beta1, beta2, float(group["eps"]), flags

    def _state_for(self, group, p):
        st = self.state[p]
        if "exp_avg" not in st:
            gi = next(i for i, g in enumerate(self.param_groups) if g is group)
            st["step"] = self._ctrl[_HEAD * (1 + gi) + _STEP]
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st["exp_avg"], st["exp_avg_sq"]


class AdamW(Adam):
    """``torch.optim.AdamW`` (decoupled decay ``p *= 1 - lr wd``) with ``max_norm`` clipping fused in."""
    _kind = N.FR_OPTIM_ADAMW

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *,
                 maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                 max_norm=None, skip_nonfinite=False):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, foreach=foreach, maximize=maximize,
                         capturable=capturable, differentiable=differentiable, fused=fused, max_norm=max_norm,
                         skip_nonfinite=skip_nonfinite)
