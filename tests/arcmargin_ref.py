"""ArcFace margin-softmax loss restated in numpy float64 (a test helper, like lbph_ref.py): the formulas of
include/frhip.h "ArcFace margin loss", forward and backward, plus the float32 error bounds the GPU tests assert.

Every bound is computed here from float64 values alone, never from a device output.  With eps = 2^-24 (float32's
unit roundoff), A_bj = sum_i |e^_bi w^_ji| and p = softmax(z):

  logits  |dz_bj|  <= (D + 16) eps s A_bj max(1, |dzy/dc|)                                        =: zb_bj
          (D terms of the dot product in any order, 16 for the two norms' roundings, the scaling and the margin
          arithmetic; through phi the cosine's error is multiplied by |dzy/dc|)
  lse     |dlse_b| <= sum_j p_bj zb_bj + (C + 16) eps + 4 eps (|lse_b| + max_j |z_bj|)
          (first-order propagation; C exponentials summed in any order, relative, so absolute on the logarithm; the
          roundings of max + log)
  mean    |d mean_j z_bj| <= (sum_j zb_bj + (C + 16) eps sum_j |z_bj|) / C
  loss    the terms above in the loss formula's linear combination + 8 eps (|lse| + |z_y| + |z_y'| + |mean|)
  g       |dg_bj| <= |u_b| wt p_bj (zb_bj + dlse_b) s |dz_j| + |g_bj| (8 eps + |d2zy/dc2 / dzy/dc| (D + 16) eps A_bj
          at the label)        (softmax - target is linear in p, dp_j = p_j (dz_j - dlse); the last term: dzy/dc moves
          with the cosine's error)
  dE^     |d dE^_bd| <= sum_j dg_bj |w^_jd| + (C + D + 16) eps sum_j |g_bj w^_jd|
          (C terms in any order; D for the rounding of w^'s norm over D squares)
  dE      the normalise Jacobian applied to the bound: inv_e (d dE^_bd + |e^_bd| sum_k d dE^_bk |e^_bk|
          + (D + 16) eps |e^_bd| sum_k |dE^_bk e^_bk| + 8 eps (|dE^_bd| + |dE^_b . e^_b| |e^_bd|))
  dW      the same with the roles of b and j exchanged (B + D + 16 terms).
"""
import math

import numpy as np

EPS = 2.0 ** -24


def _normalize(X):
    n = np.maximum(np.sqrt((X * X).sum(1, keepdims=True)), 1e-12)
    return X / n, 1.0 / n[:, 0]


def _jacobian(dhat, xhat, inv, clamped):
    dot = (dhat * xhat).sum(1, keepdims=True)
    dot = np.where(clamped[:, None], 0.0, dot)
    return (dhat - dot * xhat) * inv[:, None]


def _jacobian_bound(dhat, dhat_b, xhat, inv, D):
    ax = np.abs(xhat)
    prop = (dhat_b * ax).sum(1, keepdims=True)
    adot = (np.abs(dhat) * ax).sum(1, keepdims=True)
    dot = np.abs((dhat * xhat).sum(1, keepdims=True))
    return inv[:, None] * (dhat_b + ax * prop + (D + 16) * EPS * ax * adot + 8 * EPS * (np.abs(dhat) + dot * ax))


def arcmargin_ref(E, W, label, label_b=None, lam=1.0, scale=64.0, margin=0.5, easy_margin=False,
                  label_smoothing=0.0, u=None, dlogits=None):
    """Returns a dict: z [B, C], c_label [B] (nan: label ignored), lse, loss [B], dE, dW, their bounds *_bound and
    the absolute sums they are built from (A, abs_z, abs_gW, abs_gE).  The gradient is that of sum_b u_b loss_b
    (u defaults to ones) or, with dlogits [B, C], of a function whose gradient by z is dlogits."""
    E = np.asarray(E, np.float64)
    W = np.asarray(W, np.float64)
    B, D = E.shape
    C = W.shape[0]
    y = np.asarray(label, np.int64)
    yb = np.full(B, -1, np.int64) if label_b is None else np.asarray(label_b, np.int64)
    if label_b is None:
        lam = 1.0
    s, m, ls = float(scale), float(margin), float(label_smoothing)
    cos_m, sin_m = math.cos(m), math.sin(m)
    th, mm = math.cos(math.pi - m), math.sin(math.pi - m) * m

    Eh, inv_e = _normalize(E)
    Wh, inv_w = _normalize(W)
    cos = Eh @ Wh.T
    A = np.abs(Eh) @ np.abs(Wh).T
    va = (y >= 0) & (y < C)
    vb = (yb >= 0) & (yb < C)
    rows = np.arange(B)
    ya, ybb = np.where(va, y, 0), np.where(vb, yb, 0)

    c = cos[rows, ya]
    q = 1.0 - c * c
    sine = np.sqrt(np.maximum(q, 1e-7))
    phi = c * cos_m - sine * sin_m
    on = (c > 0) if easy_margin else (c > th)
    zy = np.where(on, phi, c if easy_margin else c - mm)
    slope = np.where(q >= 1e-7, sin_m * c / sine, 0.0)
    dz = np.where(on, cos_m + slope, 1.0)
    d2z = np.where(on & (q >= 1e-7), sin_m / np.maximum(q, 1e-7) ** 1.5, 0.0)

    z = s * cos
    z[rows[va], y[va]] = s * zy[va]
    dzm = np.ones((B, C))
    dzm[rows[va], y[va]] = dz[va]
    rel2 = np.zeros((B, C))  # |d2zy/dc2 / dzy/dc| at the label
    rel2[rows[va], y[va]] = (d2z / np.maximum(np.abs(dz), 1e-300))[va]

    zmax = z.max(1)
    ex = np.exp(z - zmax[:, None])
    lse = zmax + np.log(ex.sum(1))
    p = ex / ex.sum(1, keepdims=True)
    mean = z.mean(1)
    la = np.where(va, lam, 0.0)
    lb = np.where(vb, 1.0 - lam, 0.0)
    z_a, z_b = np.where(va, z[rows, ya], 0.0), np.where(vb, z[rows, ybb], 0.0)
    loss = la * ((1 - ls) * (lse - z_a) + ls * (lse - mean)) + lb * ((1 - ls) * (lse - z_b) + ls * (lse - mean))

    z_bound = (D + 16) * EPS * s * A * np.maximum(1.0, np.abs(dzm))
    abs_z = np.abs(z).sum(1)
    lse_bound = (p * z_bound).sum(1) + (C + 16) * EPS + 4 * EPS * (np.abs(lse) + np.abs(z).max(1))
    mean_bound = (z_bound.sum(1) + (C + 16) * EPS * abs_z) / C
    loss_bound = ((la + lb) * (lse_bound + ls * mean_bound) + (1 - ls) * (la * z_bound[rows, ya] + lb * z_bound[rows, ybb])
                  + 8 * EPS * (np.abs(lse) + np.abs(z_a) + np.abs(z_b) + np.abs(mean)))

    if dlogits is None:
        uu = np.ones(B) if u is None else np.asarray(u, np.float64)
        tgt = (la + lb)[:, None] * (ls / C) * np.ones((B, C))
        tgt[rows[va], y[va]] += (la * (1 - ls))[va]
        tgt[rows[vb], yb[vb]] += (lb * (1 - ls))[vb]
        wt = (la + lb)[:, None]
        g = uu[:, None] * (wt * p - tgt) * s * dzm
        g_bound = np.abs(uu)[:, None] * wt * p * (z_bound + lse_bound[:, None]) * s * np.abs(dzm)
    else:
        g = np.asarray(dlogits, np.float64) * s * dzm
        g_bound = np.zeros((B, C))
    g_bound = g_bound + np.abs(g) * (8 * EPS + rel2 * (D + 16) * EPS * A)

    dEh, dWh = g @ Wh, g.T @ Eh
    abs_gW, abs_gE = np.abs(g) @ np.abs(Wh), np.abs(g).T @ np.abs(Eh)
    dEh_bound = g_bound @ np.abs(Wh) + (C + D + 16) * EPS * abs_gW
    dWh_bound = g_bound.T @ np.abs(Eh) + (B + D + 16) * EPS * abs_gE
    ce = np.sqrt((E * E).sum(1)) < 1e-12
    cw = np.sqrt((W * W).sum(1)) < 1e-12
    return dict(z=z, c_label=np.where(va, c, np.nan), q_label=np.where(va, q, np.nan), lse=lse, loss=loss,
                dE=_jacobian(dEh, Eh, inv_e, ce), dW=_jacobian(dWh, Wh, inv_w, cw),
                z_bound=z_bound, lse_bound=lse_bound, loss_bound=loss_bound,
                dE_bound=_jacobian_bound(dEh, dEh_bound, Eh, inv_e, D),
                dW_bound=_jacobian_bound(dWh, dWh_bound, Wh, inv_w, D),
                A=A, abs_z=abs_z, abs_gW=abs_gW, abs_gE=abs_gE, th=(0.0 if easy_margin else th), inv_e=inv_e, inv_w=inv_w)
