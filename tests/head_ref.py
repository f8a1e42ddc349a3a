"""Head training restated in numpy float64 (a test helper, like arcmargin_ref.py): the formulas of include/frhip.h
"Head training", forward and backward, Philox4x32-10 included, plus the float32 error bounds the GPU tests assert.

Scalars enter as the device sees them: p, eps and momentum rounded to float32, 1 / (1 - p) computed in float32.
Every bound is computed here from float64 values alone, never from a device output.  With u = 2^-24 (float32's unit
roundoff), first order, a sum of n terms in any order costing at most (n + 4) u times the sum of the absolute terms
(the + 4 covers the division or scaling that follows), and a bar for "bound of":

  mean        m_ = (n + 4) u sum|x| / n + mean(z_)           (z_: the bound of the summed values; 0 for X)
  var         d = x - mean, d_ = z_ + m_ + u |d|;   v_ = (sum 2 |d| d_ + (n + 6) u sum d^2) / n
  rstd        r_ = rstd^3 (v_ + u (var + eps)) / 2 + 3 u rstd        (add, square root, division)
  x^          xh_ = rstd (z_ + m_) + |d| r_ + 2 u |x^|
  affine      H_ = |gamma| xh_ + 2 u (|gamma x^| + |beta|)
  running     rm_ = mom m_ + 4 u (|(1 - mom) rm| + |mom mean|);  rv_ = mom f v_ + 6 u (|(1 - mom) rv| + |mom f var|),
              f = n / (n - 1)
  dropout     A_ = scale m H_ + u |A|;  the mask itself is exact (integers)
  Linear      Z_ = A_ |W|^T + (K + 68) u (|A| |W|^T + |bias|)        (K terms, at most 64 split partials, the bias)
  Y           the output BN's mean / var / rstd / x^ / affine rules over the B rows with z_ = Z_
  dbeta2      (B + 4) u sum|dY|;   dgamma2: sum |dY| zh_ + (B + 4) u sum|dY z^|
  dZ          t = dY - dbeta2 / B - z^ dgamma2 / B,  t_ = dbeta2_ / B + (zh_ |dgamma2| + |z^| dgamma2_) / B
              + 6 u (|dY| + |dbeta2| / B + |z^ dgamma2| / B);  dZ_ = |gamma2| (r2_ |t| + rstd2 t_) + 3 u |dZ|
              (running statistics: dZ_ = |dY gamma2| r2_ + 3 u |dZ|)
  dbias       sum dZ_ + (B + 4) u sum|dZ|
  dW          dZ_^T |A| + |dZ|^T A_ + (B + 4) u |dZ|^T |A|
  dA          dZ_ |W| + (N + 4) u |dZ| |W|;   dH_ = scale m dA_ + u |dH|
  dbeta1      sum dH_ + (n1 + 4) u sum|dH|;  dgamma1: sum (dH_ |x^| + |dH| xh_) + (n1 + 4) u sum|dH x^|
  dX          as dZ with (dH, x^, gamma1, rstd1, n1) in place of (dY, z^, gamma2, rstd2, B) and dH_ added to t_
              (running statistics: |gamma1| (dH_ rstd1 + |dH| r1_) + 3 u |dX|; no input BN: dH_).
A bound can be exactly 0 (a dropped element, an all-zero column, gamma2 = 0): `ratio` then demands an exact result.
"""
import numpy as np

EPS = 2.0 ** -24
BATCH_STATS, DROPOUT = 1, 2
M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (or [2]) uint32-valued -> [..., 4] uint32 (Random123's Philox4x32-10)."""
    c = [np.asarray(counter[..., i], np.uint64) for i in range(4)]
    key = np.asarray(key, np.uint64)
    k0, k1 = key[..., 0], key[..., 1]
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    mask, sh = np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [((p1 >> sh) ^ c[1] ^ k0) & mask, p1 & mask, ((p0 >> sh) ^ c[3] ^ k1) & mask, p0 & mask]
        k0 = (k0 + np.uint64(0x9E3779B9)) & mask
        k1 = (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack(c, -1).astype(np.uint32)


def dropout_threshold(p):
    return int(np.floor(float(np.float32(p)) * 4294967296.0))


def dropout_mask(B, K, p, seed, offset):
    """keep [B, K] bool: element i = b K + f keeps iff word i & 3 of block i >> 2 is >= floor(p 2^32)."""
    n = B * K
    blocks = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.stack([blocks & np.uint64(M32), blocks >> np.uint64(32),
                    np.full_like(blocks, offset & M32), np.full_like(blocks, (offset >> 32) & M32)], -1)
    words = philox4x32_10(ctr, np.array([seed & M32, (seed >> 32) & M32], np.uint64)).reshape(-1)[:n]
    return (words >= np.uint32(dropout_threshold(p))).reshape(B, K) if dropout_threshold(p) > 0 else np.ones((B, K), bool)


def ratio(err, bound):
    """|err| / bound elementwise, with 0 / 0 = 0 and x / 0 = inf."""
    err, bound = np.abs(np.asarray(err, np.float64)), np.asarray(bound, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))


def _bn(V, V_, axes, n, batch, rm, rv, eps, mom, shape):
    """BN statistics of V (bound V_) over `axes`; running statistics broadcast with `shape`.  Returns a dict."""
    u = EPS
    if batch:
        mean = V.mean(axes, keepdims=True)
        m_ = (n + 4) * u * np.abs(V).sum(axes, keepdims=True) / n + V_.mean(axes, keepdims=True)
        d = V - mean
        d_ = V_ + m_ + u * np.abs(d)
        var = (d * d).mean(axes, keepdims=True)
        v_ = ((2 * np.abs(d) * d_).sum(axes, keepdims=True) + (n + 6) * u * (d * d).sum(axes, keepdims=True)) / n
    else:
        mean, var = rm.reshape(shape), rv.reshape(shape)
        m_, v_ = np.zeros(shape), np.zeros(shape)
        d = V - mean
    rstd = 1.0 / np.sqrt(var + eps)
    r_ = 0.5 * rstd ** 3 * (v_ + u * (var + eps)) + 3 * u * rstd
    xh = d * rstd
    xh_ = rstd * (V_ + m_) + np.abs(d) * r_ + 2 * u * np.abs(xh)
    out = dict(mean=mean, var=var, rstd=rstd, xh=xh, mean_=m_ + u * np.abs(mean), rstd_=r_, xh_=xh_)
    if batch:
        f = n / (n - 1.0)
        out["rm"] = ((1 - mom) * rm.reshape(shape) + mom * mean).reshape(-1)
        out["rv"] = ((1 - mom) * rv.reshape(shape) + mom * var * f).reshape(-1)
        out["rm_"] = (mom * m_ + 4 * u * (np.abs((1 - mom) * rm.reshape(shape)) + np.abs(mom * mean))).reshape(-1)
        out["rv_"] = (mom * f * v_ + 6 * u * (np.abs((1 - mom) * rv.reshape(shape)) + np.abs(mom * f * var))).reshape(-1)
    else:
        out["rm"], out["rv"] = rm.copy(), rv.copy()
        out["rm_"], out["rv_"] = np.zeros_like(rm), np.zeros_like(rv)
    return out


def _bn_input_grad(dV, dV_, bn, gamma, n, axes, batch):
    """dgamma, dbeta and the gradient by the BN's input, with bounds."""
    u = EPS
    xh, xh_, rstd, r_ = bn["xh"], bn["xh_"], bn["rstd"], bn["rstd_"]
    db = dV.sum(axes, keepdims=True)
    db_ = dV_.sum(axes, keepdims=True) + (n + 4) * u * np.abs(dV).sum(axes, keepdims=True)
    dg = (dV * xh).sum(axes, keepdims=True)
    dg_ = (dV_ * np.abs(xh) + np.abs(dV) * xh_).sum(axes, keepdims=True) + (n + 4) * u * np.abs(dV * xh).sum(axes, keepdims=True)
    if batch:
        t = dV - db / n - xh * dg / n
        t_ = dV_ + db_ / n + (xh_ * np.abs(dg) + np.abs(xh) * dg_) / n + 6 * u * (np.abs(dV) + np.abs(db) / n + np.abs(xh * dg) / n)
        dx = gamma * rstd * t
        dx_ = np.abs(gamma) * (r_ * np.abs(t) + rstd * t_) + 3 * u * np.abs(dx)
    else:
        dx = dV * gamma * rstd
        dx_ = np.abs(gamma) * (dV_ * rstd + np.abs(dV) * r_) + 3 * u * np.abs(dx)
    return dg.reshape(-1), dg_.reshape(-1), db.reshape(-1), db_.reshape(-1), dx, dx_


def head_ref(X, S, W, bias, gamma1, beta1, rm1, rv1, gamma2, beta2, rm2, rv2, flags=0, p=0.0, eps=1e-5, momentum=0.1,
             seed=0, offset=0, dY=None, round_scalars=True):
    """Returns a dict of float64 results and `<name>_` bounds: A, Z, Y, mean1, rstd1, mean2, rstd2, rm1, rv1, rm2, rv2,
    keep (the mask) and, with dY, dX, dW, dbias, dgamma1, dbeta1, dgamma2, dbeta2 (the input BN's only when it exists).
    round_scalars=False keeps eps and momentum as given (float64 comparisons with modules that hold them as doubles)."""
    u = EPS
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)
    X, W, bias, gamma1, beta1, rm1, rv1, gamma2, beta2, rm2, rv2 = map(
        f64, (X, W, bias, gamma1, beta1, rm1, rv1, gamma2, beta2, rm2, rv2))
    B, K = X.shape
    N = W.shape[0]
    batch = bool(flags & BATCH_STATS)
    eps, mom = (float(np.float32(eps)), float(np.float32(momentum))) if round_scalars else (float(eps), float(momentum))
    drop = bool(flags & DROPOUT) and float(np.float32(p)) > 0
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if drop else 1.0
    keep = dropout_mask(B, K, p, seed, offset) if drop else np.ones((B, K), bool)
    out = dict(keep=keep, scale=scale)

    if gamma1 is not None:
        Cin, n1 = K // S, B * S
        bn1 = _bn(X.reshape(B, Cin, S), np.zeros((B, Cin, S)), (0, 2), n1, batch, rm1, rv1, eps, mom, (1, Cin, 1))
        g1 = gamma1.reshape(1, Cin, 1)
        H = (g1 * bn1["xh"] + beta1.reshape(1, Cin, 1)).reshape(B, K)
        H_ = (np.abs(g1) * bn1["xh_"] + 2 * u * (np.abs(g1 * bn1["xh"]) + np.abs(beta1.reshape(1, Cin, 1)))).reshape(B, K)
        for k in ("mean", "rstd"):
            out[k + "1"], out[k + "1_"] = bn1[k].reshape(-1), bn1[k + "_"].reshape(-1)
        for k in ("rm", "rv"):
            out[k + "1"], out[k + "1_"] = bn1[k], bn1[k + "_"]
    else:
        H, H_ = X, np.zeros((B, K))
    A = np.where(keep, H * scale, 0.0)
    A_ = np.where(keep, scale * H_ + (u * np.abs(A) if drop else 0.0), 0.0)
    absAW = np.abs(A) @ np.abs(W).T + (0.0 if bias is None else np.abs(bias)[None, :])
    Z = A @ W.T + (0.0 if bias is None else bias[None, :])
    Z_ = A_ @ np.abs(W).T + (K + 68) * u * absAW
    bn2 = _bn(Z, Z_, (0,), B, batch, rm2, rv2, eps, mom, (1, N))
    g2 = gamma2.reshape(1, N)
    Y = g2 * bn2["xh"] + beta2.reshape(1, N)
    Y_ = np.abs(g2) * bn2["xh_"] + 2 * u * (np.abs(g2 * bn2["xh"]) + np.abs(beta2.reshape(1, N)))
    out.update(H=H, A=A, A_=A_, Z=Z, Z_=Z_, Y=Y, Y_=Y_, zh=bn2["xh"])
    for k in ("mean", "rstd"):
        out[k + "2"], out[k + "2_"] = bn2[k].reshape(-1), bn2[k + "_"].reshape(-1)
    for k in ("rm", "rv"):
        out[k + "2"], out[k + "2_"] = bn2[k], bn2[k + "_"]
    if dY is None:
        return out

    dY = f64(dY)
    dg2, dg2_, db2, db2_, dZ, dZ_ = _bn_input_grad(dY, np.zeros((B, N)), bn2, g2, B, (0,), batch)
    out.update(dgamma2=dg2, dgamma2_=dg2_, dbeta2=db2, dbeta2_=db2_, dZ=dZ, dZ_=dZ_)
    out["dbias"] = dZ.sum(0)
    out["dbias_"] = dZ_.sum(0) + (B + 4) * u * np.abs(dZ).sum(0)
    out["dW"] = dZ.T @ A
    out["dW_"] = dZ_.T @ np.abs(A) + np.abs(dZ).T @ A_ + (B + 4) * u * (np.abs(dZ).T @ np.abs(A))
    dA = dZ @ W
    dA_ = dZ_ @ np.abs(W) + (N + 4) * u * (np.abs(dZ) @ np.abs(W))
    dH = np.where(keep, dA * scale, 0.0)
    dH_ = np.where(keep, scale * dA_ + (u * np.abs(dH) if drop else 0.0), 0.0)
    if gamma1 is not None:
        dg1, dg1_, db1, db1_, dX, dX_ = _bn_input_grad(dH.reshape(B, Cin, S), dH_.reshape(B, Cin, S), bn1, g1, n1, (0, 2),
                                                       batch)
        out.update(dgamma1=dg1, dgamma1_=dg1_, dbeta1=db1, dbeta1_=db1_, dX=dX.reshape(B, K), dX_=dX_.reshape(B, K))
    else:
        out.update(dX=dH, dX_=dH_)
    return out


def make_case(seed, B, Cin, S, N, input_bn=True, bias=True):
    """float32 inputs of one case: per-column means in [-2, 2] and standard deviations in [0.3, 3], one all-zero
    column (a dead post-ReLU feature) and one constant non-zero column, one gamma2 entry exactly 0, random dY."""
    rng = np.random.default_rng(seed)
    K = Cin * S
    X = rng.standard_normal((B, K)) * rng.uniform(0.3, 3.0, (1, K)) + rng.uniform(-2.0, 2.0, (1, K))
    X[:, K // 3] = 0.0
    X[:, (2 * K) // 3] = 1.375
    a = np.sqrt(6.0 / (K + N))
    f32 = lambda v: np.ascontiguousarray(v, np.float32)
    case = dict(X=f32(X), W=f32(rng.uniform(-a, a, (N, K))), bias=f32(rng.uniform(-0.5, 0.5, N)) if bias else None,
                gamma1=None, beta1=None, rm1=None, rv1=None)
    if input_bn:
        case.update(gamma1=f32(rng.uniform(0.5, 1.5, Cin)), beta1=f32(rng.uniform(-0.5, 0.5, Cin)),
                    rm1=f32(rng.uniform(-1.0, 1.0, Cin)), rv1=f32(rng.uniform(0.5, 4.0, Cin)))
    g2 = rng.uniform(0.5, 1.5, N)
    g2[N // 2] = 0.0
    case.update(gamma2=f32(g2), beta2=f32(rng.uniform(-0.5, 0.5, N)), rm2=f32(rng.uniform(-1.0, 1.0, N)),
                rv2=f32(rng.uniform(0.5, 4.0, N)), dY=f32(rng.standard_normal((B, N))))
    return case


def ref_of(case, S, flags, p=0.0, eps=1e-5, momentum=0.1, seed=0, offset=0, grad=True):
    """head_ref on a make_case dict."""
    c = case
    return head_ref(c["X"], S, c["W"], c["bias"], c["gamma1"], c["beta1"], c["rm1"], c["rv1"], c["gamma2"], c["beta2"],
                    c["rm2"], c["rv2"], flags, p, eps, momentum, seed, offset, c["dY"] if grad else None)
