"""Backbone training restated in numpy float64 (a test helper, like head_ref.py): the five calls of include/frhip.h
"Backbone training" -- convolution forward and backward with the input transform, BatchNorm2d statistics, and the
BN + residual + ReLU forward and backward -- plus the float32 error bounds the GPU tests assert, a Bottleneck composed
of those five restatements, and a plain-torch Bottleneck (F.conv2d, F.batch_norm, autograd) to hold both against.

Layouts are the device's: activations [B, H, W, C], weights [Cout, k, k, Cin].  Scalars enter as the device sees them
(eps and momentum rounded to float32).  Every bound is computed here from float64 values alone, never from a device
output.  With u = 2^-24, first order, a sum of n terms in any order costing at most (n + c) u times the sum of the
absolute terms, and a bar for "bound of":

  transform   pre = X scale + shift (one fma), pre_ = |scale| X_ + |X| scale_ + shift_ + u |pre|;  A = relu?(pre),
              A_ = pre_ where the ReLU passes, else 0 (the mask is exact: `margin` below)
  forward     Z_ = A_ |W|^T + (K + 68) u |A| |W|^T        (K = k k Cin terms, at most 64 split partials)
  dW          dZ_^T |A| + |dZ|^T A_ + (M + 4) u |dZ|^T |A|                     (M = B OH OW terms)
  dA          scatter(dZ_ |W|) + (k k Cout + 4) u scatter(|dZ| |W|)             (the device sums every tap, zeros too)
  BN          mean, var, rstd, x^ and the running update: head_ref._bn's rules over the M rows
  scale       gamma rstd:  scale_ = |gamma| rstd_ + u |scale|
  shift       beta - mean scale:  shift_ = mean_ |scale| + |mean| scale_ + u |mean scale| + u |shift|
  Y           y = fma(Z, scale, shift) + Res:  y_ = |scale| Z_ + |Z| scale_ + shift_ + u |Z scale + shift| + u |y|
  backward    dH = dY [y > 0];  dgamma, dbeta, dZ: head_ref._bn_input_grad's rules (running statistics: dZ = dH scale,
              within the same bound);  dRes = dH exactly
`margin` is the smallest |pre-activation| / its bound over every ReLU input: make_case asserts it is above 1, so that no
float32 evaluation within the bounds can flip a mask bit, and the masks of device and restatement agree exactly.
"""
import numpy as np

from tests.head_ref import EPS, _bn, _bn_input_grad, ratio  # noqa: F401  (ratio is re-exported)

IN_RELU = 1
BATCH_STATS, RELU = 1, 2

# (B, H, W, Cin, Cout, k, stride): see tests/test_gpu_conv_train.py for what each is for
CONV_CASES = [(1, 1, 1, 4, 4, 1, 1), (2, 4, 4, 8, 68, 3, 1), (2, 5, 6, 4, 4, 3, 1), (3, 7, 7, 12, 8, 3, 2),
              (3, 7, 7, 20, 72, 1, 2), (5, 4, 4, 132, 4, 1, 1), (2, 4, 4, 512, 512, 3, 1), (2, 4, 4, 2048, 512, 1, 1)]
BN_CASES = [(2, 4), (70, 68), (130, 132)]  # (M, C)
EPS_BN, MOM = 1e-5, 0.1


def out_size(n, k, stride):
    return (n + 2 * (k // 2) - k) // stride + 1


def _margin(pre, pre_):
    """min |pre| / pre_ over the elements with pre != 0 (an exact zero stays an exact zero on the device)."""
    nz = pre != 0
    if not nz.any():
        return np.inf
    with np.errstate(divide="ignore"):
        return float(np.min(np.abs(pre[nz]) / np.maximum(pre_[nz], 1e-300)))


def transform(X, scale, shift, flags, X_=0.0, scale_=0.0, shift_=0.0):
    """A, A_, margin."""
    X = np.asarray(X, np.float64)
    if scale is None:
        return X, np.zeros_like(X) + X_, np.inf
    pre = X * scale + shift
    pre_ = np.abs(scale) * X_ + np.abs(X) * scale_ + shift_ + EPS * np.abs(pre)
    if flags & IN_RELU:
        return np.where(pre > 0, pre, 0.0), np.where(pre > 0, pre_, 0.0), _margin(pre, pre_)
    return pre, pre_, np.inf


def im2col(A, k, stride):
    """[B, H, W, C] -> [B OH OW, k k C] in (r, s, c) order, zeros under padded taps."""
    B, H, W, C = A.shape
    pad = k // 2
    OH, OW = out_size(H, k, stride), out_size(W, k, stride)
    Ap = np.zeros((B, H + 2 * pad, W + 2 * pad, C))
    Ap[:, pad:pad + H, pad:pad + W] = A
    cols = np.zeros((B, OH, OW, k, k, C))
    for r in range(k):
        for s in range(k):
            cols[:, :, :, r, s] = Ap[:, r:r + (OH - 1) * stride + 1:stride, s:s + (OW - 1) * stride + 1:stride]
    return cols.reshape(B * OH * OW, k * k * C)


def col2im(dcols, shape, k, stride):
    """The transpose of im2col: [B OH OW, k k C] -> [B, H, W, C]."""
    B, H, W, C = shape
    pad = k // 2
    OH, OW = out_size(H, k, stride), out_size(W, k, stride)
    d = dcols.reshape(B, OH, OW, k, k, C)
    out = np.zeros((B, H + 2 * pad, W + 2 * pad, C))
    for r in range(k):
        for s in range(k):
            out[:, r:r + (OH - 1) * stride + 1:stride, s:s + (OW - 1) * stride + 1:stride] += d[:, :, :, r, s]
    return out[:, pad:pad + H, pad:pad + W]


def conv_ref(X, Wt, k, stride, scale=None, shift=None, flags=0, dZ=None, X_=0.0, scale_=0.0, shift_=0.0, dZ_=0.0):
    """dict: A, Z (+ dA, dW with dZ), each with a `_` bound, and margin."""
    u = EPS
    X, Wt = np.asarray(X, np.float64), np.asarray(Wt, np.float64)
    f = lambda a: None if a is None else np.asarray(a, np.float64)
    A, A_, margin = transform(X, f(scale), f(shift), flags, X_, scale_, shift_)
    B, H, W, Cin = X.shape
    N = Wt.shape[0]
    K = k * k * Cin
    Wm = Wt.reshape(N, K)
    cols, cols_ = im2col(A, k, stride), im2col(A_, k, stride)
    OH, OW = out_size(H, k, stride), out_size(W, k, stride)
    Z = cols @ Wm.T
    Z_ = cols_ @ np.abs(Wm).T + (K + 68) * u * (np.abs(cols) @ np.abs(Wm).T)
    out = dict(A=A, A_=A_, margin=margin, Z=Z.reshape(B, OH, OW, N), Z_=Z_.reshape(B, OH, OW, N))
    if dZ is None:
        return out
    M = B * OH * OW
    dZm = np.asarray(dZ, np.float64).reshape(M, N)
    dZm_ = np.zeros_like(dZm) + np.asarray(dZ_, np.float64).reshape(-1, N) if np.ndim(dZ_) else np.zeros_like(dZm) + dZ_
    out["dW"] = (dZm.T @ cols).reshape(Wt.shape)
    out["dW_"] = (dZm_.T @ np.abs(cols) + np.abs(dZm).T @ cols_ + (M + 4) * u * (np.abs(dZm).T @ np.abs(cols))).reshape(Wt.shape)
    out["dA"] = col2im(dZm @ Wm, X.shape, k, stride)
    out["dA_"] = col2im(dZm_ @ np.abs(Wm), X.shape, k, stride) + (k * k * N + 4) * u * col2im(np.abs(dZm) @ np.abs(Wm), X.shape, k, stride)
    return out


def bn_stats_ref(Z, gamma, beta, rm, rv, flags, eps=EPS_BN, momentum=MOM, Z_=None, round_scalars=True):
    """dict: mean, rstd, scale, shift, rm, rv with `_` bounds, and `bn` (head_ref._bn's dict, for the backward)."""
    u = EPS
    Z = np.asarray(Z, np.float64)
    C = Z.shape[-1]
    Zm = Z.reshape(-1, C)
    M = Zm.shape[0]
    gamma, beta, rm, rv = (np.asarray(a, np.float64) for a in (gamma, beta, rm, rv))
    eps, mom = (float(np.float32(eps)), float(np.float32(momentum))) if round_scalars else (float(eps), float(momentum))
    Zm_ = np.zeros_like(Zm) if Z_ is None else np.asarray(Z_, np.float64).reshape(-1, C)
    bn = _bn(Zm, Zm_, (0,), M, bool(flags & BATCH_STATS), rm, rv, eps, mom, (1, C))
    mean, rstd = bn["mean"].reshape(-1), bn["rstd"].reshape(-1)
    mean_, rstd_ = bn["mean_"].reshape(-1), bn["rstd_"].reshape(-1)
    scale = gamma * rstd
    scale_ = np.abs(gamma) * rstd_ + u * np.abs(scale)
    shift = beta - mean * scale
    shift_ = mean_ * np.abs(scale) + np.abs(mean) * scale_ + u * np.abs(mean * scale) + u * np.abs(shift)
    return dict(bn=bn, mean=mean, mean_=mean_, rstd=rstd, rstd_=rstd_, scale=scale, scale_=scale_, shift=shift,
                shift_=shift_, rm=bn["rm"], rm_=bn["rm_"], rv=bn["rv"], rv_=bn["rv_"])


def bn_act_ref(Z, st, gamma, flags, Res=None, dY=None, Z_=None, Res_=None, dY_=None):
    """Y (+ dZ, dRes, dgamma, dbeta with dY) with `_` bounds, and margin; st is bn_stats_ref's result for this Z."""
    u = EPS
    Z = np.asarray(Z, np.float64)
    C = Z.shape[-1]
    Zm = Z.reshape(-1, C)
    M = Zm.shape[0]
    zero = np.zeros_like(Zm)
    Zm_ = zero if Z_ is None else np.asarray(Z_, np.float64).reshape(-1, C)
    y0 = Zm * st["scale"] + st["shift"]
    y = y0 + (0.0 if Res is None else np.asarray(Res, np.float64).reshape(-1, C))
    y_ = np.abs(st["scale"]) * Zm_ + np.abs(Zm) * st["scale_"] + st["shift_"] + u * np.abs(y0)
    if Res is not None:
        y_ = y_ + u * np.abs(y) + (0.0 if Res_ is None else np.asarray(Res_, np.float64).reshape(-1, C))
    relu = bool(flags & RELU)
    mask = y > 0 if relu else np.ones_like(y, bool)
    out = dict(Y=np.where(mask, y, 0.0).reshape(Z.shape), Y_=np.where(mask, y_, 0.0).reshape(Z.shape), mask=mask.reshape(Z.shape),
               margin=_margin(y, y_) if relu else np.inf)
    if dY is None:
        return out
    dYm = np.asarray(dY, np.float64).reshape(-1, C)
    dYm_ = zero if dY_ is None else np.asarray(dY_, np.float64).reshape(-1, C)
    dH, dH_ = np.where(mask, dYm, 0.0), np.where(mask, dYm_, 0.0)
    g = np.asarray(gamma, np.float64).reshape(1, C)
    dg, dg_, db, db_, dZ, dZ_ = _bn_input_grad(dH, dH_, st["bn"], g, M, (0,), bool(flags & BATCH_STATS))
    out.update(dZ=dZ.reshape(Z.shape), dZ_=dZ_.reshape(Z.shape), dRes=dH.reshape(Z.shape), dRes_=dH_.reshape(Z.shape),
               dgamma=dg, dgamma_=dg_, dbeta=db, dbeta_=db_)
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------
f32 = lambda v: np.ascontiguousarray(v, np.float32)


def make_conv_case(seed, B, H, W, Cin, Cout, k, stride):
    """float32 inputs of one convolution case: X, Wt, a transform with a nonzero shift of both signs (so that a padded
    tap wrongly filled with relu(shift) would show), dZ.  Asserts the ReLU margin."""
    rng = np.random.default_rng(seed)
    OH, OW = out_size(H, k, stride), out_size(W, k, stride)
    a = np.sqrt(6.0 / (k * k * Cin + Cout))
    shift = rng.uniform(0.25, 1.0, Cin) * np.where(np.arange(Cin) % 3 == 1, -1.0, 1.0)
    case = dict(X=f32(rng.standard_normal((B, H, W, Cin))), Wt=f32(rng.uniform(-a, a, (Cout, k, k, Cin))),
                scale=f32(rng.uniform(0.5, 1.5, Cin) * rng.choice([-1.0, 1.0], Cin)), shift=f32(shift),
                dZ=f32(rng.standard_normal((B, OH, OW, Cout))), k=k, stride=stride)
    m = conv_ref(case["X"], case["Wt"], k, stride, case["scale"], case["shift"], IN_RELU)["margin"]
    assert m > 1.0, (seed, m)
    return case


def make_bn_case(seed, M, C):
    """float32 inputs of one BN case: Z with per-column means and deviations, one constant column, one gamma exactly 0,
    Res, dY.  Asserts the ReLU margin in every mode."""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((M, C)) * rng.uniform(0.3, 3.0, (1, C)) + rng.uniform(-2.0, 2.0, (1, C))
    Z[:, C // 3] = 1.375
    g = rng.uniform(0.5, 1.5, C)
    g[C // 2] = 0.0
    beta = rng.uniform(0.25, 0.75, C) * rng.choice([-1.0, 1.0], C)
    case = dict(Z=f32(Z), gamma=f32(g), beta=f32(beta), rm=f32(rng.uniform(-1.0, 1.0, C)), rv=f32(rng.uniform(0.5, 4.0, C)),
                Res=f32(rng.standard_normal((M, C))), dY=f32(rng.standard_normal((M, C))))
    for flags in (RELU, RELU | BATCH_STATS):
        for res in (None, case["Res"]):
            r = bn_case_ref(case, flags, res is not None)
            assert r["margin"] > 1.0, (seed, flags, r["margin"])
    return case


def bn_case_ref(case, flags, with_res, grad=True):
    st = bn_stats_ref(case["Z"], case["gamma"], case["beta"], case["rm"], case["rv"], flags)
    out = bn_act_ref(case["Z"], st, case["gamma"], flags, case["Res"] if with_res else None, case["dY"] if grad else None)
    out.update({k: v for k, v in st.items() if k != "bn"})
    return out


CONV_SEEDS = {c: 100 + i for i, c in enumerate(CONV_CASES)}
BN_SEEDS = {c: 200 + i for i, c in enumerate(BN_CASES)}


# ---- one Bottleneck out of the five restatements ---------------------------------------------------------------------
BLOCK_CASES = {"down": dict(B=3, H=7, Cin=24, P=8, Cout=32, stride=2, down=True),
               "plain": dict(B=2, H=4, Cin=32, P=8, Cout=32, stride=1, down=False)}
CONVS = ("conv1", "conv2", "conv3", "down")
# The ReLU margin a block case must have.  Carried through three convolutions and BNs, the worst-case bounds (every
# rounding of every sum aligned, layer after layer) are so wide that some of a few thousand pre-activations always lie
# within them (margins of 0.002 .. 0.18 over the first eleven seeds), so the single calls' "above 1" cannot be asked of
# a whole block.  The block tests hold the device to a measured tolerance, not to these bounds, and a flipped mask bit
# moves a gradient by a whole dY element -- it can only fail such a test, never let it pass -- so the margin here only
# keeps the cases away from needless flips: the seeds below are the best of the first eleven.
BLOCK_MARGIN = 1.0 / 16
BLOCK_SEEDS = {"down": 6, "plain": 10}


def make_block_case(seed, B, H, Cin, P, Cout, stride, down):
    """float32 parameters (reference layout [Cout, k, k, Cin]), statistics, input x [B, H, H, Cin] and dY."""
    rng = np.random.default_rng(seed)
    Ho = out_size(H, 3, stride)
    case = dict(x=f32(np.maximum(rng.standard_normal((B, H, H, Cin)) + 0.3, 0)), dY=f32(rng.standard_normal((B, Ho, Ho, Cout))),
                stride=stride)
    shapes = dict(conv1=(P, 1, Cin), conv2=(P, 3, P), conv3=(Cout, 1, P))
    if down:
        shapes["down"] = (Cout, 1, Cin)
    for name, (n, k, c) in shapes.items():
        a = np.sqrt(6.0 / (k * k * c + n))
        case[name] = dict(W=f32(rng.uniform(-a, a, (n, k, k, c))), gamma=f32(rng.uniform(0.5, 1.5, n)),
                          beta=f32(rng.uniform(-0.5, 0.5, n)), rm=f32(rng.uniform(-0.3, 0.3, n)),
                          rv=f32(rng.uniform(0.5, 2.0, n)))
    for batch in (True, False):
        m = bottleneck_ref(case, batch)["margin"]
        assert m > BLOCK_MARGIN, (seed, batch, m)
    return case


def bottleneck_ref(case, batch_stats, eps=EPS_BN, momentum=MOM, round_scalars=True):
    """Forward and backward of torchvision's v1.5 Bottleneck as the chain of calls the device runs.  Returns Y, dX, and
    per conv dW, dgamma, dbeta, rm, rv (no bounds: the device test's tolerance is measured, see its docstring), and the
    smallest ReLU margin of the forward, its bounds carried through the chain."""
    fl = BATCH_STATS if batch_stats else 0
    x, s = np.asarray(case["x"], np.float64), case["stride"]
    down = "down" in case
    p = lambda n: case[n]
    stats = lambda c, n: bn_stats_ref(c["Z"], p(n)["gamma"], p(n)["beta"], p(n)["rm"], p(n)["rv"], fl, eps, momentum,
                                      c["Z_"], round_scalars)
    tr = lambda st: dict(scale=st["scale"], shift=st["shift"], flags=IN_RELU, scale_=st["scale_"], shift_=st["shift_"])
    f1 = conv_ref(x, p("conv1")["W"], 1, 1)
    s1 = stats(f1, "conv1")
    f2 = conv_ref(f1["Z"], p("conv2")["W"], 3, s, X_=f1["Z_"], **tr(s1))
    s2 = stats(f2, "conv2")
    f3 = conv_ref(f2["Z"], p("conv3")["W"], 1, 1, X_=f2["Z_"], **tr(s2))
    s3 = stats(f3, "conv3")
    Z1, Z2, Z3 = f1["Z"], f2["Z"], f3["Z"]
    R_ = None
    if down:
        fd = conv_ref(x, p("down")["W"], 1, s)
        Zd = fd["Z"]
        sd = stats(fd, "down")
        rd = bn_act_ref(Zd, sd, p("down")["gamma"], fl, Z_=fd["Z_"])
        R, R_ = rd["Y"], rd["Y_"]
    else:
        R = x
    margin = min(f2["margin"], f3["margin"], bn_act_ref(Z3, s3, p("conv3")["gamma"], fl | RELU, R, Z_=f3["Z_"], Res_=R_)["margin"])
    o3 = bn_act_ref(Z3, s3, p("conv3")["gamma"], fl | RELU, R, case["dY"])
    c3 = conv_ref(Z2, p("conv3")["W"], 1, 1, s2["scale"], s2["shift"], IN_RELU, o3["dZ"])
    o2 = bn_act_ref(Z2, s2, p("conv2")["gamma"], fl | RELU, None, c3["dA"])
    c2 = conv_ref(Z1, p("conv2")["W"], 3, s, s1["scale"], s1["shift"], IN_RELU, o2["dZ"])
    o1 = bn_act_ref(Z1, s1, p("conv1")["gamma"], fl | RELU, None, c2["dA"])
    c1 = conv_ref(x, p("conv1")["W"], 1, 1, dZ=o1["dZ"])
    out = dict(Y=o3["Y"], margin=margin)
    grads = dict(conv1=(c1, o1, s1), conv2=(c2, o2, s2), conv3=(c3, o3, s3))
    if down:
        od = bn_act_ref(Zd, sd, p("down")["gamma"], fl, None, o3["dRes"])
        cd = conv_ref(x, p("down")["W"], 1, s, dZ=od["dZ"])
        grads["down"] = (cd, od, sd)
        out["dX"] = c1["dA"] + cd["dA"]
    else:
        out["dX"] = c1["dA"] + o3["dRes"]
    for n, (c, o, st) in grads.items():
        out[n] = dict(dW=c["dW"], dgamma=o["dgamma"], dbeta=o["dbeta"], rm=st["rm"], rv=st["rv"])
    return out


def torch_bottleneck(case, batch_stats, dtype, eps=EPS_BN, momentum=MOM):
    """The same block in plain torch on the CPU (F.conv2d, F.batch_norm, autograd) in `dtype`; bottleneck_ref's dict, as
    numpy float64, in the device's layouts."""
    import torch
    import torch.nn.functional as F

    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    x = t(case["x"]).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    s = case["stride"]
    prm, buf = {}, {}
    for n in CONVS:
        if n in case:
            prm[n] = dict(W=t(case[n]["W"]).permute(0, 3, 1, 2).contiguous().requires_grad_(True),
                          gamma=t(case[n]["gamma"]).requires_grad_(True), beta=t(case[n]["beta"]).requires_grad_(True))
            buf[n] = dict(rm=t(case[n]["rm"]).clone(), rv=t(case[n]["rv"]).clone())

    def cbn(v, n, stride, pad):
        z = F.conv2d(v, prm[n]["W"], None, stride, pad)
        return F.batch_norm(z, buf[n]["rm"], buf[n]["rv"], prm[n]["gamma"], prm[n]["beta"], batch_stats, momentum, eps)

    h = F.relu(cbn(x, "conv1", 1, 0))
    h = F.relu(cbn(h, "conv2", s, 1))
    h = cbn(h, "conv3", 1, 0)
    idn = cbn(x, "down", s, 0) if "down" in case else x
    y = F.relu(h + idn)
    y.backward(t(case["dY"]).permute(0, 3, 1, 2))
    nhwc = lambda v: v.detach().permute(0, 2, 3, 1).double().numpy()
    out = dict(Y=nhwc(y), dX=nhwc(x.grad))
    for n in prm:
        out[n] = dict(dW=nhwc(prm[n]["W"].grad), dgamma=prm[n]["gamma"].grad.double().numpy(),
                      dbeta=prm[n]["beta"].grad.double().numpy(), rm=buf[n]["rm"].double().numpy(),
                      rv=buf[n]["rv"].double().numpy())
    return out


def flat_items(res):
    """(name, array) pairs of a bottleneck result dict."""
    for k, v in res.items():
        if k == "margin":
            continue
        if isinstance(v, dict):
            for k2, v2 in v.items():
                yield f"{k}.{k2}", np.asarray(v2, np.float64)
        else:
            yield k, np.asarray(v, np.float64)


def rel_err(a, b):
    """max |a - b| / max |b|."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))
