"""ResNet-50's layer4 trained on the device (libfrhip's fr_conv_train_* / fr_bn* entry points).

The reference's fine-tuning helper ``freeze_layers(model, freeze_ratio=0.8)`` (models/arcface/arcface_model.py:223)
freezes the first 127 of the backbone's 159 parameter tensors, which leaves exactly ``backbone.layer4`` (and the two
affine tensors of ``layer3.5.bn3``, left out here) trainable.  ``ResNet50Layer4`` is those three torchvision v1.5
Bottlenecks over ``FRModel.features(x, at="layer4_in")``; its output is what ``EmbeddingHead.for_arch(
"resnet50_arcface")`` reads.  Each ``Bottleneck``'s forward and backward are one ``torch.autograd.Function`` over the
five C calls (exact float32, bitwise repeatable): only the raw conv outputs, the block input and the block output are
kept, ``relu(bn(.))`` of the inner activations is recomputed where conv2 / conv3 and their weight gradients read it.
Parameters and buffers are ordinary ``nn.Conv2d`` / ``nn.BatchNorm2d`` containers (conv weights ``channels_last``, which
is the device's [Cout][kh][kw][Cin]), so ``torch.optim``, ``state_dict`` and ``.train()`` / ``.eval()`` work unchanged,
and ``reference_state_dict()`` hands the trained layer back to ``FRModel.load_state_dict`` under the reference's keys.
Activations are physical NHWC ``[B, H, W, C]`` tensors.  There is no CPU or PyTorch fallback.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _native as N
from . import weights as Wt


def _new(dev, *shape):
    return torch.empty(shape, dtype=torch.float32, device=dev)


def _out_size(n, k, stride):
    return (n + 2 * (k // 2) - k) // stride + 1


def conv_forward(x, w, k, stride, scale=None, shift=None, relu=False):
    """fr_conv_train_forward: x [B,H,W,Cin], w [Cout,k,k,Cin] (contiguous float32 device tensors) -> Z [B,OH,OW,Cout]."""
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    L = N.lib()
    nbytes = L.fr_conv_train_workspace(B, H, W, Cin, Cout, k, stride)
    if nbytes == 0:
        N.check(-1, "fr_conv_train_workspace")
    ws = _new(x.device, (nbytes + 3) // 4)
    Z = _new(x.device, B, _out_size(H, k, stride), _out_size(W, k, stride), Cout)
    N.check(L.fr_conv_train_forward(N.ptr(x), B, H, W, Cin, N.ptr(scale), N.ptr(shift), N.FR_CONV_IN_RELU if relu else 0,
                                    N.ptr(w), Cout, k, stride, N.ptr(Z), N.ptr(ws), nbytes, N.stream_ptr(x.device)),
            "fr_conv_train_forward")
    return Z


def conv_backward(x, w, k, stride, dZ, scale=None, shift=None, relu=False, need_a=True, need_w=True):
    """fr_conv_train_backward: (dA [B,H,W,Cin], dW [Cout,k,k,Cin]), None where not asked for."""
    B, H, W, Cin = x.shape
    Cout = w.shape[0]
    dA = _new(x.device, B, H, W, Cin) if need_a else None
    dW = _new(x.device, Cout, k, k, Cin) if need_w else None
    if need_a or need_w:
        N.check(N.lib().fr_conv_train_backward(N.ptr(x), B, H, W, Cin, N.ptr(scale), N.ptr(shift),
                                               N.FR_CONV_IN_RELU if relu else 0, N.ptr(w), Cout, k, stride, N.ptr(dZ),
                                               N.ptr(dA), N.ptr(dW), N.stream_ptr(x.device)), "fr_conv_train_backward")
    return dA, dW


def bn_stats(Z, gamma, beta, rm, rv, batch, eps, momentum):
    """fr_bn2d_train_stats over Z [..., C]: (mean, rstd, scale, shift); with batch statistics rm / rv are updated."""
    C = Z.shape[-1]
    mean, rstd, scale, shift = (_new(Z.device, C) for _ in range(4))
    N.check(N.lib().fr_bn2d_train_stats(N.ptr(Z), Z.numel() // C, C, N.ptr(gamma), N.ptr(beta), N.ptr(rm), N.ptr(rv),
                                        N.FR_BN_BATCH_STATS if batch else 0, float(eps), float(momentum), N.ptr(mean),
                                        N.ptr(rstd), N.ptr(scale), N.ptr(shift), N.stream_ptr(Z.device)),
            "fr_bn2d_train_stats")
    return mean, rstd, scale, shift


def bn_act_forward(Z, scale, shift, res=None, relu=False):
    """fr_bn_act_forward: relu?(Z scale + shift + res?)."""
    C = Z.shape[-1]
    Y = torch.empty_like(Z)
    N.check(N.lib().fr_bn_act_forward(N.ptr(Z), Z.numel() // C, C, N.ptr(scale), N.ptr(shift), N.ptr(res),
                                      N.FR_BN_RELU if relu else 0, N.ptr(Y), N.stream_ptr(Z.device)), "fr_bn_act_forward")
    return Y


def bn_act_backward(dY, Z, stats, gamma, res=None, batch=True, relu=False, need_res=False, need_affine=True,
                    in_place=False):
    """fr_bn_act_backward: (dZ, dRes, dgamma, dbeta); stats = bn_stats' tuple.  in_place: dZ overwrites dY."""
    C = Z.shape[-1]
    mean, rstd, scale, shift = stats
    dZ = dY if in_place else torch.empty_like(Z)
    dRes = torch.empty_like(Z) if need_res else None
    dg, db = (_new(Z.device, C), _new(Z.device, C)) if need_affine else (None, None)
    flags = (N.FR_BN_BATCH_STATS if batch else 0) | (N.FR_BN_RELU if relu else 0)
    N.check(N.lib().fr_bn_act_backward(N.ptr(dY), N.ptr(Z), Z.numel() // C, C, N.ptr(mean), N.ptr(rstd), N.ptr(gamma),
                                       N.ptr(scale), N.ptr(shift), N.ptr(res), flags, N.ptr(dZ), N.ptr(dRes), N.ptr(dg),
                                       N.ptr(db), N.stream_ptr(Z.device)), "fr_bn_act_backward")
    return dZ, dRes, dg, db


def _khwc(w):
    """An OIHW-shaped conv weight as the device's contiguous [Cout, kh, kw, Cin] (no copy when it is channels_last)."""
    return w.detach().permute(0, 2, 3, 1).contiguous()


class _BottleneckFn(torch.autograd.Function):
    """Arguments: x, then (weight, gamma, beta) of conv1, conv2, conv3 and the downsample (three Nones without one),
    then the running statistics [(rm, rv)] in that order and (stride, batch, eps, momentum)."""

    @staticmethod
    def forward(ctx, x, w1, g1, b1, w2, g2, b2, w3, g3, b3, wd, gd, bd, running, opts):
        stride, batch, eps, momentum = opts
        det = lambda t: t.detach().contiguous()
        x_ = det(x)
        W = [_khwc(w1), _khwc(w2), _khwc(w3)] + ([_khwc(wd)] if wd is not None else [])
        G = [det(g) for g in (g1, g2, g3)] + ([det(gd)] if wd is not None else [])
        Bt = [det(b) for b in (b1, b2, b3)] + ([det(bd)] if wd is not None else [])
        st = lambda Z, i: bn_stats(Z, G[i], Bt[i], running[i][0], running[i][1], batch, eps, momentum)
        Z1 = conv_forward(x_, W[0], 1, 1)
        s1 = st(Z1, 0)
        Z2 = conv_forward(Z1, W[1], 3, stride, s1[2], s1[3], True)
        s2 = st(Z2, 1)
        Z3 = conv_forward(Z2, W[2], 1, 1, s2[2], s2[3], True)
        s3 = st(Z3, 2)
        saved = [x_, Z1, Z2, Z3, *W, *G, *s1, *s2, *s3]
        if wd is not None:
            Zd = conv_forward(x_, W[3], 1, stride)
            sd = st(Zd, 3)
            R = bn_act_forward(Zd, sd[2], sd[3])
            saved += [Zd, R, *sd]
        else:
            R = x_
        Y = bn_act_forward(Z3, s3[2], s3[3], R, True)
        ctx.save_for_backward(*saved)
        ctx.opts = (stride, batch, wd is not None)
        return Y

    @staticmethod
    def backward(ctx, dY):
        stride, batch, down = ctx.opts
        t = list(ctx.saved_tensors)
        x, Z1, Z2, Z3 = t[:4]
        n = 4 if down else 3
        W, G = t[4:4 + n], t[4 + n:4 + 2 * n]
        rest = t[4 + 2 * n:]
        s1, s2, s3 = rest[0:4], rest[4:8], rest[8:12]
        need = ctx.needs_input_grad
        aff = lambda i: need[2 + 3 * i] or need[3 + 3 * i]
        out = [None] * 15
        if not any(need[:13]):
            return tuple(out)
        dY = dY.float().contiguous()
        R = rest[13] if down else x
        need_res = need[0] or (down and any(need[10:13]))
        dZ3, dRes, out[8], out[9] = bn_act_backward(dY, Z3, s3, G[2], R, batch, True, need_res, aff(2))
        dA2, dW3 = conv_backward(Z2, W[2], 1, 1, dZ3, s2[2], s2[3], True, True, need[7])
        dZ2, _, out[5], out[6] = bn_act_backward(dA2, Z2, s2, G[1], None, batch, True, False, aff(1), in_place=True)
        dA1, dW2 = conv_backward(Z1, W[1], 3, stride, dZ2, s1[2], s1[3], True, True, need[4])
        dZ1, _, out[2], out[3] = bn_act_backward(dA1, Z1, s1, G[0], None, batch, True, False, aff(0), in_place=True)
        dX, dW1 = conv_backward(x, W[0], 1, 1, dZ1, need_a=need[0], need_w=need[1])
        dWd = None
        if down:
            Zd, sd = rest[12], rest[14:18]
            if need_res:
                dZd, _, out[11], out[12] = bn_act_backward(dRes, Zd, sd, G[3], None, batch, False, False, aff(3),
                                                           in_place=True)
                dXd, dWd = conv_backward(x, W[3], 1, stride, dZd, need_a=need[0], need_w=need[10])
                if need[0]:
                    dX = dX + dXd
        elif need[0]:
            dX = dX + dRes
        oihw = lambda g: None if g is None else g.permute(0, 3, 1, 2)  # a channels_last gradient of OIHW shape
        out[0] = dX
        out[1], out[4], out[7], out[10] = oihw(dW1), oihw(dW2), oihw(dW3), oihw(dWd)
        for i in range(13):
            if not need[i]:
                out[i] = None
        return tuple(out)


def _check(x, cin):
    if not x.is_cuda:
        raise RuntimeError("backbone_train needs ROCm GPU tensors; there is deliberately no CPU fallback")
    if x.dim() != 4 or x.shape[3] != cin:
        raise ValueError(f"Bottleneck: physical NHWC input [B, H, W, {cin}] expected, got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise TypeError("Bottleneck: float32 input expected")


class Bottleneck(nn.Module):
    """torchvision's v1.5 Bottleneck (the stride on conv2, expansion 4) on physical NHWC ``[B, H, W, inplanes]`` ->
    ``[B, OH, OW, 4 planes]``.  ``.train()`` / ``.eval()`` follow ``nn.Module``: training BNs use batch statistics and
    update the running ones; eval-mode BNs, or BNs after ``freeze_bn()``, use the running ones."""

    expansion = 4

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: bool = False, eps: float = 1e-5,
                 momentum: float = 0.1):
        super().__init__()
        out = planes * self.expansion
        if not downsample and (stride != 1 or inplanes != out):
            raise ValueError("Bottleneck: a block that changes the shape needs downsample=True")
        self.inplanes, self.planes, self.stride = inplanes, planes, stride
        self.eps, self.momentum = float(eps), float(momentum)
        bn = lambda c: nn.BatchNorm2d(c, eps=eps, momentum=momentum)
        # containers of the parameters and buffers only: their own forward is never called
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = bn(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = bn(planes)
        self.conv3 = nn.Conv2d(planes, out, 1, bias=False)
        self.bn3 = bn(out)
        self.downsample = nn.Sequential(nn.Conv2d(inplanes, out, 1, stride, bias=False), bn(out)) if downsample else None
        for conv in self._convs():
            conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)

    def _convs(self):
        return [self.conv1, self.conv2, self.conv3] + ([self.downsample[0]] if self.downsample is not None else [])

    def _bns(self):
        return [self.bn1, self.bn2, self.bn3] + ([self.downsample[1]] if self.downsample is not None else [])

    def freeze_bn(self) -> "Bottleneck":
        """The reference's freeze_bn: every BN uses (and keeps) its running statistics and its parameters stop
        training.  Like the reference's, it holds until the next ``.train()``."""
        for bn in self._bns():
            bn.eval()
            for prm in bn.parameters():
                prm.requires_grad = False
        return self

    def batch_stats(self) -> bool:
        modes = {bn.training for bn in self._bns()}
        if len(modes) != 1:
            raise RuntimeError("Bottleneck: all BNs must be in the same mode")
        return modes.pop()

    def forward(self, x):
        _check(x, self.inplanes)
        batch = self.batch_stats()
        bns = self._bns()
        if batch:
            if x.shape[0] * _out_size(x.shape[1], 3, self.stride) * _out_size(x.shape[2], 3, self.stride) < 2:
                raise ValueError("Bottleneck: batch statistics need more than one value per channel")
            for bn in bns:
                bn.num_batches_tracked += 1
        args = []
        for conv, bn in zip(self._convs(), bns):
            args += [conv.weight, bn.weight, bn.bias]
        args += [None] * (12 - len(args))
        running = [(bn.running_mean, bn.running_var) for bn in bns]
        return _BottleneckFn.apply(x, *args, running, (self.stride, batch, self.eps, self.momentum))


class ResNet50Layer4(nn.Module):
    """``backbone.layer4`` of the reference's ResNet-50: ``[B, 7, 7, 1024]`` features (``FRModel.features(x,
    at="layer4_in")``) -> the pooled ``[B, 2048]`` tensor ``EmbeddingHead.for_arch("resnet50_arcface")`` takes."""

    PREFIX = "backbone.layer4"

    def __init__(self, eps: float = Wt.BN_EPS["resnet50_arcface"], momentum: float = 0.1):
        super().__init__()
        self.blocks = nn.ModuleList([Bottleneck(1024, 512, 2, True, eps, momentum), Bottleneck(2048, 512, 1, False, eps, momentum),
                                     Bottleneck(2048, 512, 1, False, eps, momentum)])

    @classmethod
    def for_model(cls, state_dict=None) -> "ResNet50Layer4":
        """layer4 with the values of ``state_dict`` (the reference's keys) when given."""
        layer = cls()
        if state_dict is not None:
            layer.load_reference_state_dict(state_dict)
        return layer

    def reference_state_dict(self) -> dict:
        """layer4 under the reference's key names (contiguous CPU tensors of torch's shapes): ``sd.update(
        layer4.reference_state_dict()); model.load_state_dict(sd)`` puts it into the engine."""
        sd = {}
        for i, blk in enumerate(self.blocks):
            for name, t in blk.state_dict().items():
                sd[f"{self.PREFIX}.{i}.{name}"] = t.detach().cpu().contiguous().clone()
        return sd

    def load_reference_state_dict(self, sd) -> None:
        """Take layer4's values from a state_dict with the reference's key names (other keys are ignored)."""
        for i, blk in enumerate(self.blocks):
            new = {}
            for name, t in blk.state_dict().items():
                key = f"{self.PREFIX}.{i}.{name}"
                if key not in sd:
                    if name.endswith("num_batches_tracked"):
                        continue
                    raise KeyError(f"ResNet50Layer4: {key} missing from the state_dict")
                new[name] = torch.as_tensor(sd[key]).to(t.dtype).reshape(t.shape)
            blk.load_state_dict(new, strict=False)  # copies in place: the conv weights stay channels_last

    def freeze_bn(self) -> "ResNet50Layer4":
        for blk in self.blocks:
            blk.freeze_bn()
        return self

    def forward(self, x):
        for blk in self.blocks:
            x = blk(x)
        return x.mean(dim=(1, 2))
