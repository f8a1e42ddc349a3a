"""The embedding head between a frozen trunk and the losses, trained on the device (libfrhip's fr_head_* entry points).

``EmbeddingHead`` is the reference's ``bn1 -> dropout -> fc -> bn2`` (models/arcface/arcface_model.py:154-159,
191-196), IResNet100's ``bn2 -> flatten -> fc -> features`` and FaceNet's ``dropout -> last_linear -> last_bn`` as one
module over ``FRModel.features(x)``: its forward and backward are one ``torch.autograd.Function`` over
fr_head_forward / fr_head_backward (input BN, dropout, Linear and output BN fused; exact float32; bitwise
repeatable).  Its parameters and buffers are ordinary ``nn.Parameter``s and buffers held by ``nn.BatchNorm1d`` /
``nn.Linear`` containers, so ``torch.optim``, ``state_dict`` and ``.train()`` / ``.eval()`` work unchanged, and
``reference_state_dict()`` hands the trained head back to ``FRModel.load_state_dict`` under the reference's key names.
There is no CPU or PyTorch fallback: the forward needs GPU tensors.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import _native as N
from . import weights as Wt

# (input BN, Linear, output BN) key prefixes in the reference's checkpoints
REFERENCE_KEYS = {
    "resnet50_arcface": ("bn1", "fc", "bn2"),
    "iresnet100": ("bn2", "fc", "features"),
    "irv1_facenet": (None, "model.last_linear", "model.last_bn"),
}


def _workspace(B, K, Nout, device):
    nbytes = N.lib().fr_head_workspace(B, K, Nout)
    if nbytes == 0:
        N.check(-1, "fr_head_workspace")
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device), nbytes


def _check(x, weight):
    if not (x.is_cuda and weight.is_cuda):
        raise RuntimeError("EmbeddingHead needs ROCm GPU tensors; there is deliberately no CPU fallback")
    if x.dim() != 2 or x.shape[1] != weight.shape[1]:
        raise ValueError(f"EmbeddingHead: input [B, {weight.shape[1]}] expected, got {tuple(x.shape)}")
    if x.dtype != torch.float32 or weight.dtype != torch.float32:
        raise TypeError("EmbeddingHead: float32 input and parameters expected")


def head_forward(x, S, weight, bias, gamma1, beta1, rm1, rv1, gamma2, beta2, rm2, rv2, flags, p, eps, momentum, seed,
                 offset):
    """One fr_head_forward on contiguous float32 device tensors: (Y, Z, mean1, rstd1, mean2, rstd2).
    With FR_HEAD_BATCH_STATS the running statistics are updated in place."""
    B, K = x.shape
    Nout = weight.shape[0]
    dev = x.device
    ws, nbytes = _workspace(B, K, Nout, dev)
    Y, Z = (torch.empty((B, Nout), dtype=torch.float32, device=dev) for _ in range(2))
    mean2, rstd2 = (torch.empty(Nout, dtype=torch.float32, device=dev) for _ in range(2))
    mean1 = rstd1 = None
    if gamma1 is not None:
        mean1, rstd1 = (torch.empty(K // S, dtype=torch.float32, device=dev) for _ in range(2))
    N.check(N.lib().fr_head_forward(N.ptr(x), B, K, S, N.ptr(weight), Nout, N.ptr(bias), N.ptr(gamma1), N.ptr(beta1),
                                    N.ptr(rm1), N.ptr(rv1), N.ptr(gamma2), N.ptr(beta2), N.ptr(rm2), N.ptr(rv2),
                                    int(flags), float(p), float(eps), float(momentum), int(seed), int(offset), N.ptr(Y),
                                    N.ptr(Z), N.ptr(mean1), N.ptr(rstd1), N.ptr(mean2), N.ptr(rstd2), None,
                                    N.ptr(ws), nbytes, N.stream_ptr(dev)), "fr_head_forward")
    return Y, Z, mean1, rstd1, mean2, rstd2


def head_backward(x, S, weight, gamma1, beta1, gamma2, flags, p, seed, offset, mean1, rstd1, mean2, rstd2, Z, dY,
                  need_x=True, need_w=True, need_bias=True, need_bn1=True, need_bn2=True):
    """One fr_head_backward: (dX, dW, dbias, dgamma1, dbeta1, dgamma2, dbeta2), None where not asked for."""
    B, K = x.shape
    Nout = weight.shape[0]
    dev = x.device
    ws, nbytes = _workspace(B, K, Nout, dev)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    dX = new(B, K) if need_x else None
    dW = new(Nout, K) if need_w else None
    dbias = new(Nout) if need_bias else None
    need_bn1 = need_bn1 and gamma1 is not None
    dg1, db1 = (new(K // S), new(K // S)) if need_bn1 else (None, None)
    dg2, db2 = (new(Nout), new(Nout)) if need_bn2 else (None, None)
    N.check(N.lib().fr_head_backward(N.ptr(x), B, K, S, N.ptr(weight), Nout, N.ptr(gamma1), N.ptr(beta1), N.ptr(gamma2),
                                     int(flags), float(p), int(seed), int(offset), N.ptr(mean1), N.ptr(rstd1),
                                     N.ptr(mean2), N.ptr(rstd2), N.ptr(Z), N.ptr(dY), N.ptr(dX), N.ptr(dW), N.ptr(dbias),
                                     N.ptr(dg1), N.ptr(db1), N.ptr(dg2), N.ptr(db2), N.ptr(ws), nbytes,
                                     N.stream_ptr(dev)), "fr_head_backward")
    return dX, dW, dbias, dg1, db1, dg2, db2


class _Head(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, gamma1, beta1, gamma2, beta2, rm1, rv1, rm2, rv2, opts):
        S, flags, p, eps, momentum, seed, offset = opts
        det = lambda t: None if t is None else t.detach().contiguous()
        x_, w_, g1, b1, g2 = det(x), det(weight), det(gamma1), det(beta1), det(gamma2)
        Y, Z, mean1, rstd1, mean2, rstd2 = head_forward(x_, S, w_, det(bias), g1, b1, rm1, rv1, g2, det(beta2), rm2,
                                                        rv2, flags, p, eps, momentum, seed, offset)
        ctx.save_for_backward(x_, w_, g1, b1, g2, mean1, rstd1, mean2, rstd2, Z)
        ctx.opts = (S, flags, p, seed, offset)
        ctx.has_bias = bias is not None
        return Y

    @staticmethod
    def backward(ctx, dY):
        x, w, g1, b1, g2, mean1, rstd1, mean2, rstd2, Z = ctx.saved_tensors
        S, flags, p, seed, offset = ctx.opts
        need = ctx.needs_input_grad
        need_x, need_w, need_bias = need[0], need[1], ctx.has_bias and need[2]
        need_bn1, need_bn2 = g1 is not None and (need[3] or need[4]), need[5] or need[6]
        if not (need_x or need_w or need_bias or need_bn1 or need_bn2):
            return (None,) * 12
        dX, dW, dbias, dg1, db1, dg2, db2 = head_backward(x, S, w, g1, b1, g2, flags, p, seed, offset, mean1, rstd1, mean2,
                                                          rstd2, Z, dY.float().contiguous(), need_x, need_w, need_bias,
                                                          need_bn1, need_bn2)
        pick = lambda g, i: g if need[i] else None
        return (dX, dW, dbias, pick(dg1, 3), pick(db1, 4), pick(dg2, 5), pick(db2, 6), None, None, None, None, None)


class EmbeddingHead(nn.Module):
    """``[B, in_features]`` pre-head features -> ``[B, embedding_size]`` un-normalised embeddings.

    in_channels: channels of the input BN (feature ``f`` belongs to channel ``f // (in_features // in_channels)``);
    None means ``in_features`` (BatchNorm1d).  input_bn=False drops the input BN (FaceNet).  ``.train()`` / ``.eval()``
    follow ``nn.Module``: training uses batch statistics and dropout, ``freeze_bn()`` keeps dropout but puts both BNs
    on their running statistics (the reference helper: BN modules in eval mode, their parameters frozen)."""

    def __init__(self, in_features: int, embedding_size: int = 512, in_channels: Optional[int] = None,
                 input_bn: bool = True, bias: bool = True, dropout: float = 0.5, eps: float = 1e-5,
                 momentum: float = 0.1):
        super().__init__()
        in_channels = in_features if in_channels is None else in_channels
        if in_channels < 1 or in_features % in_channels:
            raise ValueError(f"EmbeddingHead: in_channels {in_channels} must divide in_features {in_features}")
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"EmbeddingHead: dropout must be in [0, 1), got {dropout}")
        self.in_features = in_features
        self.embedding_size = embedding_size
        self.in_channels = in_channels
        self.spatial = in_features // in_channels
        self.dropout = float(dropout)
        self.eps = float(eps)
        self.momentum = float(momentum)
        # containers of the parameters and buffers only: their own forward is never called
        self.bn_in = nn.BatchNorm1d(in_channels, eps=eps, momentum=momentum) if input_bn else None
        self.fc = nn.Linear(in_features, embedding_size, bias=bias)
        self.bn_out = nn.BatchNorm1d(embedding_size, eps=eps, momentum=momentum)
        self.keys = REFERENCE_KEYS["resnet50_arcface" if input_bn else "irv1_facenet"]
        self._seed: Optional[int] = None
        self._offset = 0

    # -- construction ---------------------------------------------------------------------------------------------
    @classmethod
    def for_arch(cls, arch: str, state_dict=None) -> "EmbeddingHead":
        """The head of one of the three models, with the values of ``state_dict`` (reference keys) when given."""
        if arch not in REFERENCE_KEYS:
            raise ValueError(f"unknown arch {arch!r}")
        eps = Wt.BN_EPS[arch]
        if arch == "resnet50_arcface":
            head = cls(2048, 512, dropout=0.5, eps=eps)
        elif arch == "iresnet100":
            head = cls(25088, 512, in_channels=512, dropout=0.0, eps=eps)
        else:
            head = cls(1792, 512, input_bn=False, bias=False, dropout=0.6, eps=eps)
        head.keys = REFERENCE_KEYS[arch]
        if state_dict is not None:
            head.load_reference_state_dict(state_dict)
        return head

    def _named(self):
        """(reference prefix, container) pairs."""
        k_in, k_fc, k_out = self.keys
        out = [(k_fc, self.fc), (k_out, self.bn_out)]
        return ([(k_in, self.bn_in)] if self.bn_in is not None else []) + out

    def reference_state_dict(self) -> dict:
        """The head under the reference's key names (CPU tensors): ``sd.update(head.reference_state_dict());
        model.load_state_dict(sd)`` puts it into the engine."""
        sd = {}
        for prefix, mod in self._named():
            for name, t in mod.state_dict().items():
                sd[f"{prefix}.{name}"] = t.detach().cpu().clone()
        return sd

    def load_reference_state_dict(self, sd) -> None:
        """Take the head's values from a state_dict with the reference's key names (other keys are ignored)."""
        for prefix, mod in self._named():
            own = mod.state_dict()
            new = {}
            for name, t in own.items():
                key = f"{prefix}.{name}"
                if key not in sd:
                    if name == "num_batches_tracked":
                        continue
                    raise KeyError(f"EmbeddingHead: {key} missing from the state_dict")
                v = torch.as_tensor(sd[key])
                if name == "weight" and mod is self.fc:
                    v = v.reshape(self.embedding_size, self.in_features)
                new[name] = v.to(t.dtype)
            mod.load_state_dict(new, strict=False)

    # -- modes ----------------------------------------------------------------------------------------------------
    def freeze_bn(self) -> "EmbeddingHead":
        """The reference's freeze_bn: both BNs use (and keep) their running statistics and their parameters stop
        training; dropout stays as ``.training`` says.  Like the reference's, it holds until the next ``.train()``."""
        for bn in (self.bn_in, self.bn_out):
            if bn is not None:
                bn.eval()
                for prm in bn.parameters():
                    prm.requires_grad = False
        return self

    def seed(self, seed: int, offset: int = 0) -> "EmbeddingHead":
        """The dropout generator's (seed, offset): each forward with active dropout uses one offset, then adds 1."""
        self._seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._offset = int(offset) & 0xFFFFFFFFFFFFFFFF
        return self

    def flags(self) -> int:
        batch = self.bn_out.training
        if self.bn_in is not None and self.bn_in.training != batch:
            raise RuntimeError("EmbeddingHead: both BNs must be in the same mode")
        return (N.FR_HEAD_BATCH_STATS if batch else 0) | (N.FR_HEAD_DROPOUT if self.training and self.dropout > 0 else 0)

    def forward(self, x):
        _check(x, self.fc.weight)
        flags = self.flags()
        if self._seed is None:
            self.seed(torch.initial_seed())
        offset = self._offset
        if flags & N.FR_HEAD_DROPOUT:
            self._offset = (self._offset + 1) & 0xFFFFFFFFFFFFFFFF
        bi, bo = self.bn_in, self.bn_out
        if flags & N.FR_HEAD_BATCH_STATS:
            for bn in (bi, bo):
                if bn is not None:
                    bn.num_batches_tracked += 1
        opts = (self.spatial, flags, self.dropout, self.eps, self.momentum, self._seed, offset)
        return _Head.apply(x, self.fc.weight, self.fc.bias, bi.weight if bi is not None else None,
                           bi.bias if bi is not None else None, bo.weight, bo.bias,
                           bi.running_mean if bi is not None else None, bi.running_var if bi is not None else None,
                           bo.running_mean, bo.running_var, opts)

    def extra_repr(self) -> str:
        return (f"in_features={self.in_features}, embedding_size={self.embedding_size}, in_channels={self.in_channels}, "
                f"dropout={self.dropout}, eps={self.eps}, momentum={self.momentum}")
