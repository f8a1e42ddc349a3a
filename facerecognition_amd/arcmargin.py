"""ArcFace additive-angular-margin head and its loss on the device (libfrhip's fr_arcmargin_* entry points).

Drop-in for the reference's ``ArcMarginProduct`` (models/arcface/arcface_model.py:23-62: same constructor, same
``weight`` parameter and ``state_dict`` key, ``forward(input, label)`` returns the ``[B, C]`` logits) plus a fused
``loss`` that never stores a ``B x C`` tensor: cross-entropy with label smoothing and mixup
(train_arcface.py:109-111) straight from the embeddings and the class centres.  Both are differentiable in
``input`` and ``weight`` through ``torch.autograd.Function``s whose backward is fr_arcmargin_backward.  There is
no CPU or PyTorch fallback: tensors must live on the GPU.

A label outside ``[0, C)`` is ignored: it contributes loss 0 and no gradient (an ignored first label also means no
margin for the row).
"""
from __future__ import annotations

import math

import torch
from torch import nn

from . import _native as N


def _check(input, weight):
    if not (input.is_cuda and weight.is_cuda):
        raise RuntimeError("arcmargin needs ROCm GPU tensors; there is deliberately no CPU fallback")
    if input.dim() != 2 or weight.dim() != 2 or input.shape[1] != weight.shape[1]:
        raise ValueError(f"arcmargin: input [B, D] and weight [C, D] expected, got {tuple(input.shape)} and "
                         f"{tuple(weight.shape)}")
    if input.dtype != torch.float32 or weight.dtype != torch.float32:
        raise TypeError("arcmargin: float32 input and weight expected (the scores are exact float32)")


def _labels(label, B, device):
    if label is None:
        return None
    l = torch.as_tensor(label, device=device).reshape(-1).to(torch.int32).contiguous()
    if l.numel() != B:
        raise ValueError(f"arcmargin: {B} labels expected, got {l.numel()}")
    return l


def _workspace(B, C, D, device):
    nbytes = N.lib().fr_arcmargin_workspace(B, C, D)
    if nbytes == 0:
        N.check(-1, "fr_arcmargin_workspace")
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device), nbytes


def _forward(e, w, y, yb, lam, scale, margin, easy, ls, want_logits):
    """One fr_arcmargin_forward: (loss [B], lse, inv_e, inv_w, logits or None)."""
    B, D = e.shape
    C = w.shape[0]
    dev = e.device
    ws, nbytes = _workspace(B, C, D, dev)
    loss, lse, inv_e = (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(3))
    inv_w = torch.empty(C, dtype=torch.float32, device=dev)
    logits = torch.empty((B, C), dtype=torch.float32, device=dev) if want_logits else None
    N.check(N.lib().fr_arcmargin_forward(N.ptr(e), B, D, N.ptr(w), C, N.ptr(y), N.ptr(yb), lam, scale, margin,
                                         int(easy), ls, N.ptr(loss), N.ptr(lse), N.ptr(inv_e), N.ptr(inv_w),
                                         N.ptr(logits), N.ptr(ws), nbytes, N.stream_ptr(dev)), "fr_arcmargin_forward")
    return loss, lse, inv_e, inv_w, logits


def _backward(e, w, y, yb, lam, scale, margin, easy, ls, lse, inv_e, inv_w, u, dlogits, need_e, need_w):
    B, D = e.shape
    C = w.shape[0]
    dev = e.device
    ws, nbytes = _workspace(B, C, D, dev)
    dE = torch.empty_like(e) if need_e else None
    dW = torch.empty_like(w) if need_w else None
    N.check(N.lib().fr_arcmargin_backward(N.ptr(e), B, D, N.ptr(w), C, N.ptr(y), N.ptr(yb), lam, scale, margin,
                                          int(easy), ls, N.ptr(lse), N.ptr(inv_e), N.ptr(inv_w), N.ptr(u),
                                          N.ptr(dlogits), N.ptr(dE), N.ptr(dW), N.ptr(ws), nbytes,
                                          N.stream_ptr(dev)), "fr_arcmargin_backward")
    return dE, dW


class _Logits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, weight, label, scale, margin, easy):
        e, w = input.detach().contiguous(), weight.detach().contiguous()
        _, lse, inv_e, inv_w, logits = _forward(e, w, label, None, 1.0, scale, margin, easy, 0.0, True)
        ctx.save_for_backward(e, w, label, inv_e, inv_w)
        ctx.opts = (scale, margin, easy)
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        e, w, label, inv_e, inv_w = ctx.saved_tensors
        scale, margin, easy = ctx.opts
        need_e, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_e or need_w):
            return (None,) * 6
        dE, dW = _backward(e, w, label, None, 1.0, scale, margin, easy, 0.0, None, inv_e, inv_w, None,
                           dlogits.float().contiguous(), need_e, need_w)
        return dE, dW, None, None, None, None


class _Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input, weight, label, label_b, lam, scale, margin, easy, ls):
        e, w = input.detach().contiguous(), weight.detach().contiguous()
        loss, lse, inv_e, inv_w, _ = _forward(e, w, label, label_b, lam, scale, margin, easy, ls, False)
        ctx.save_for_backward(e, w, label, label_b, lse, inv_e, inv_w)
        ctx.opts = (lam, scale, margin, easy, ls)
        return loss

    @staticmethod
    def backward(ctx, u):
        e, w, label, label_b, lse, inv_e, inv_w = ctx.saved_tensors
        lam, scale, margin, easy, ls = ctx.opts
        need_e, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_e or need_w):
            return (None,) * 9
        dE, dW = _backward(e, w, label, label_b, lam, scale, margin, easy, ls, lse, inv_e, inv_w,
                           u.float().contiguous(), None, need_e, need_w)
        return dE, dW, None, None, None, None, None, None, None


def arcface_logits(input, weight, label, scale: float = 64.0, margin: float = 0.5, easy_margin: bool = False):
    """The reference module's forward over an explicit weight: ``[B, C]`` logits, the margin on ``label``."""
    _check(input, weight)
    return _Logits.apply(input, weight, _labels(label, input.shape[0], input.device), float(scale), float(margin),
                         bool(easy_margin))


def arcface_loss(input, weight, label, label_b=None, lam: float = 1.0, scale: float = 64.0, margin: float = 0.5,
                 easy_margin: bool = False, label_smoothing: float = 0.0, reduction: str = "mean"):
    """Margin-softmax cross-entropy of embeddings ``input [B, D]`` against class centres ``weight [C, D]`` without a
    ``B x C`` tensor: ``lam CE(z, label) + (1 - lam) CE(z, label_b)`` with label smoothing, the logits ``z`` carrying
    the margin on ``label``.  reduction: 'mean' | 'sum' | 'none' (per-sample losses ``[B]``)."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"arcface_loss: reduction must be 'mean', 'sum' or 'none', not {reduction!r}")
    _check(input, weight)
    B, dev = input.shape[0], input.device
    loss = _Loss.apply(input, weight, _labels(label, B, dev), _labels(label_b, B, dev), float(lam), float(scale),
                       float(margin), bool(easy_margin), float(label_smoothing))
    return loss if reduction == "none" else (loss.sum() if reduction == "sum" else loss.mean())


def class_accuracy(input, weight, label) -> float:
    """The reference's training accuracy "from the pure cosine" (train_arcface.py:637-649): the share of samples
    whose nearest normalised class centre is their label, by the exact top-1 gallery match (no margin, no logits)."""
    from .gallery import DeviceGallery

    _check(input, weight)
    with torch.no_grad():
        gal = DeviceGallery(dim=int(weight.shape[1]), device=input.device.index or 0)
        try:
            gal.set_device_rows(nn.functional.normalize(weight.detach()))
            _, idx = gal.search_device(input.detach(), 1)
        finally:
            gal.close()
        y = _labels(label, input.shape[0], input.device)
        return float((idx[:, 0] == y).float().mean().item())


class ArcMarginProduct(nn.Module):
    """The reference's ArcFace layer: ``cos(theta + m)`` on the label's logit, everything scaled by ``scale``."""

    def __init__(self, in_features: int, out_features: int, scale: float = 64.0, margin: float = 0.5,
                 easy_margin: bool = False):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.scale = scale
        self.margin = margin
        self.easy_margin = easy_margin
        self.weight = nn.Parameter(torch.empty(out_features, in_features, dtype=torch.float32))
        nn.init.xavier_uniform_(self.weight)
        self.cos_m = math.cos(margin)
        self.sin_m = math.sin(margin)
        self.th = math.cos(math.pi - margin)
        self.mm = math.sin(math.pi - margin) * margin

    def forward(self, input, label):
        return arcface_logits(input, self.weight, label, self.scale, self.margin, self.easy_margin)

    def loss(self, input, label, label_b=None, lam: float = 1.0, label_smoothing: float = 0.0,
             reduction: str = "mean"):
        """The fused criterion (no logits are stored): see arcface_loss."""
        return arcface_loss(input, self.weight, label, label_b, lam, self.scale, self.margin, self.easy_margin,
                            label_smoothing, reduction)

    def class_accuracy(self, input, label) -> float:
        return class_accuracy(input, self.weight, label)

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, out_features={self.out_features}, scale={self.scale}, "
                f"margin={self.margin}, easy_margin={self.easy_margin}")
