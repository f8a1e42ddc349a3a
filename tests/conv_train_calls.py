"""The five backbone-training C calls made raw, numpy in and numpy out (a helper of the GPU tests): every buffer is
allocated 64 sentinel elements too long, the sentinels are checked after the call, and inputs are checked to be unchanged.
Device results come back bit for bit, so a chain of these calls is the chain the modules run."""
import numpy as np

GUARD, SENT = 64, 7.5


class Call:
    """The buffers of one C call."""

    def __init__(self, dev):
        import torch
        from facerecognition_amd import _native as NL

        self.torch, self.NL, self.L, self.dev = torch, NL, NL.lib(), dev
        self.bufs, self.inputs = {}, {}
        self.stream = NL.stream_ptr(dev)

    def put(self, name, init=None, n=None, alias=None):
        """A guarded buffer holding `init` (an input, checked afterwards), or n elements of sentinel (an output);
        alias: the address of another buffer instead.  None: no buffer (a NULL argument)."""
        if alias is not None:
            self.bufs[name] = self.bufs[alias]
            return
        if init is None and n is None:
            return
        n = int(np.asarray(init).size if init is not None else n)
        t = self.torch.full((n + GUARD,), SENT, dtype=self.torch.float32, device=self.dev)
        if init is not None:
            a = np.ascontiguousarray(init, np.float32).reshape(-1)
            t[:n] = self.torch.from_numpy(a).to(self.dev)
            self.inputs[name] = a
        self.bufs[name] = (t, n)

    def p(self, name):
        return self.NL.ptr(self.bufs[name][0]) if name in self.bufs else 0

    def done(self, rc, what, shapes, written=()):
        """Check rc, wait, check sentinels and inputs; returns {name: array} of the buffers named in `shapes`."""
        self.NL.check(rc, what)
        self.torch.cuda.synchronize()
        out = {}
        for name, (t, n) in self.bufs.items():
            h = t.cpu().numpy()
            if name != "ws":
                assert np.all(h[n:] == SENT), f"{what}: {name}: sentinel overwritten"
            if name in self.inputs and name not in written:
                assert np.array_equal(h[:n].view(np.uint32), self.inputs[name].view(np.uint32)), f"{what}: input {name} changed"
            if name in shapes:
                out[name] = h[:n].reshape(shapes[name]).copy()
        return out


def out_size(n, k, stride):
    return (n + 2 * (k // 2) - k) // stride + 1


def conv_forward(dev, X, Wt, k, stride, scale=None, shift=None, flags=0, ws_scale=1):
    B, H, W, Cin = X.shape
    Cout = Wt.shape[0]
    c = Call(dev)
    for name, v in (("X", X), ("Wt", Wt), ("scale", scale), ("shift", shift)):
        c.put(name, v)
    nbytes = c.L.fr_conv_train_workspace(B, H, W, Cin, Cout, k, stride)
    assert nbytes >= 16 and nbytes % 4 == 0
    c.put("ws", n=ws_scale * nbytes // 4)
    shape = (B, out_size(H, k, stride), out_size(W, k, stride), Cout)
    c.put("Z", n=int(np.prod(shape)))
    rc = c.L.fr_conv_train_forward(c.p("X"), B, H, W, Cin, c.p("scale"), c.p("shift"), flags, c.p("Wt"), Cout, k, stride,
                                   c.p("Z"), c.p("ws"), ws_scale * nbytes, c.stream)
    return c.done(rc, "fr_conv_train_forward", {"Z": shape})["Z"]


def conv_backward(dev, X, Wt, k, stride, dZ, scale=None, shift=None, flags=0, want_da=True, want_dw=True):
    """{dA, dW}, each only when asked for."""
    B, H, W, Cin = X.shape
    Cout = Wt.shape[0]
    c = Call(dev)
    for name, v in (("X", X), ("Wt", Wt), ("scale", scale), ("shift", shift), ("dZ", dZ)):
        c.put(name, v)
    if want_da:
        c.put("dA", n=X.size)
    if want_dw:
        c.put("dW", n=Wt.size)
    rc = c.L.fr_conv_train_backward(c.p("X"), B, H, W, Cin, c.p("scale"), c.p("shift"), flags, c.p("Wt"), Cout, k, stride,
                                    c.p("dZ"), c.p("dA"), c.p("dW"), c.stream)
    return c.done(rc, "fr_conv_train_backward", {"dA": X.shape, "dW": Wt.shape})


def bn_stats(dev, Z, gamma, beta, rm, rv, flags, eps, momentum):
    """{mean, rstd, scale, shift, rm, rv}."""
    C = Z.shape[-1]
    c = Call(dev)
    for name, v in (("Z", Z), ("gamma", gamma), ("beta", beta), ("rm", rm), ("rv", rv)):
        c.put(name, v)
    for name in ("mean", "rstd", "scale", "shift"):
        c.put(name, n=C)
    rc = c.L.fr_bn2d_train_stats(c.p("Z"), Z.size // C, C, c.p("gamma"), c.p("beta"), c.p("rm"), c.p("rv"), flags, eps,
                                 momentum, c.p("mean"), c.p("rstd"), c.p("scale"), c.p("shift"), c.stream)
    return c.done(rc, "fr_bn2d_train_stats", {n: (C,) for n in ("mean", "rstd", "scale", "shift", "rm", "rv")},
                  written=("rm", "rv") if flags & 1 else ())


def bn_act_forward(dev, Z, scale, shift, Res=None, flags=0):
    C = Z.shape[-1]
    c = Call(dev)
    for name, v in (("Z", Z), ("scale", scale), ("shift", shift), ("Res", Res)):
        c.put(name, v)
    c.put("Y", n=Z.size)
    rc = c.L.fr_bn_act_forward(c.p("Z"), Z.size // C, C, c.p("scale"), c.p("shift"), c.p("Res"), flags, c.p("Y"), c.stream)
    return c.done(rc, "fr_bn_act_forward", {"Y": Z.shape})["Y"]


def bn_act_backward(dev, dY, Z, st, gamma, Res=None, flags=0, want_dz=True, want_res=False, want_affine=True, alias=False):
    """{dZ, dRes, dgamma, dbeta}, each only when asked for; st: bn_stats' dict; alias: dZ is written over dY."""
    C = Z.shape[-1]
    c = Call(dev)
    for name, v in (("dY", dY), ("Z", Z), ("mean", st["mean"]), ("rstd", st["rstd"]), ("gamma", gamma),
                    ("scale", st["scale"]), ("shift", st["shift"]), ("Res", Res)):
        c.put(name, v)
    if want_dz:
        c.put("dZ", n=Z.size, alias="dY" if alias else None)
    if want_res:
        c.put("dRes", n=Z.size)
    if want_affine:
        c.put("dgamma", n=C)
        c.put("dbeta", n=C)
    rc = c.L.fr_bn_act_backward(c.p("dY"), c.p("Z"), Z.size // C, C, c.p("mean"), c.p("rstd"), c.p("gamma"), c.p("scale"),
                                c.p("shift"), c.p("Res"), flags, c.p("dZ"), c.p("dRes"), c.p("dgamma"), c.p("dbeta"), c.stream)
    return c.done(rc, "fr_bn_act_backward", {"dZ": Z.shape, "dRes": Z.shape, "dgamma": (C,), "dbeta": (C,)},
                  written=("dY",) if alias else ())
