"""Online triplet mining and the triplet margin loss on the device (libfrhip's fr_triplet_* entry points).

Drop-in for what the reference's ``models/facenet`` package exports next to ``FaceNetModel``: ``TripletLoss``
(facenet_model.py:53-64), ``mine_triplets`` (:71-115), ``mine_semi_hard_triplets`` and ``mine_batch_hard_triplets``
(facenet_dataloader.py:169-284), plus train_facenet.py's ``compute_triplet_metrics``.  The reference mines with
``torch.cdist`` and a Python loop that synchronises with the host for every (anchor, positive) pair; here a mining
call is a handful of launches and one read-back of the triplet count.  The definitions (distance form, tie rule,
output order, the gradient at the hinge) are in include/frhip.h "Triplet mining and loss".

There is no CPU or PyTorch fallback: tensors must live on the GPU, float32.  At most 32768 rows per call.
"""
from __future__ import annotations

import torch
from torch import nn

from . import _native as N

SEMI_HARD, BATCH_HARD, FIRST = 0, 1, 2
_MODES = {"semi_hard": SEMI_HARD, "batch_hard": BATCH_HARD, "hard": BATCH_HARD}  # 'hard': train_facenet.py's name


def _check(embeddings):
    if not (isinstance(embeddings, torch.Tensor) and embeddings.is_cuda):
        raise RuntimeError("triplet mining and loss need ROCm GPU tensors; there is deliberately no CPU fallback")
    if embeddings.dim() != 2:
        raise ValueError(f"triplet: embeddings [N, D] expected, got {tuple(embeddings.shape)}")
    if embeddings.dtype != torch.float32:
        raise TypeError("triplet: float32 embeddings expected (the mining scores are exact float32)")


def _i32(x, n, device, what):
    t = torch.as_tensor(x, device=device).reshape(-1).to(torch.int32).contiguous()
    if t.numel() != n:
        raise ValueError(f"triplet: {n} {what} expected, got {t.numel()}")
    return t


def _mine(embeddings, labels, mode, margin, ws_bytes=None):
    """fr_triplet_count + fr_triplet_mine: (a, p, n) int32 [T], semi uint8 [T], lims int64 [N + 1].  ws_bytes: the
    workspace to use instead of the recommended one (the results do not depend on it)."""
    _check(embeddings)
    e = embeddings.detach().contiguous()
    n_rows, dim = e.shape
    dev = e.device
    y = _i32(labels, n_rows, dev, "labels")
    if n_rows < 2:  # nothing to mine (the ABI starts at two rows)
        z = torch.empty(0, dtype=torch.int32, device=dev)
        return z, z.clone(), z.clone(), torch.empty(0, dtype=torch.uint8, device=dev), \
            torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
    L = N.lib()
    lims = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
    N.check(L.fr_triplet_count(N.ptr(y), n_rows, mode, N.ptr(lims), N.stream_ptr(dev)), "fr_triplet_count")
    if ws_bytes is None:
        ws_bytes = L.fr_triplet_workspace(n_rows, dim)
        if ws_bytes == 0:
            N.check(-1, "fr_triplet_workspace")
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)
    T = int(lims[-1].item())  # the one host synchronisation of a mining call
    a, p, n = (torch.empty(T, dtype=torch.int32, device=dev) for _ in range(3))
    semi = torch.empty(T, dtype=torch.uint8, device=dev)
    if T:
        N.check(L.fr_triplet_mine(N.ptr(e), n_rows, dim, N.ptr(y), mode, float(margin), N.ptr(lims), N.ptr(a), N.ptr(p),
                                  N.ptr(n), T, N.ptr(semi), N.ptr(ws), ws_bytes, N.stream_ptr(dev)), "fr_triplet_mine")
    return a, p, n, semi, lims


def _forward(e, a, p, n, margin):
    """fr_triplet_loss_forward: stats [4] = (loss, accuracy, pos_dist, neg_dist) and the per-triplet terms [T, 4]."""
    n_rows, dim = e.shape
    T = a.numel()
    terms = torch.empty((T, 4), dtype=torch.float32, device=e.device)
    stats = torch.empty(4, dtype=torch.float32, device=e.device)
    N.check(N.lib().fr_triplet_loss_forward(N.ptr(e), n_rows, dim, N.ptr(a), N.ptr(p), N.ptr(n), T, float(margin),
                                            N.ptr(terms), N.ptr(stats), N.stream_ptr(e.device)),
            "fr_triplet_loss_forward")
    return stats, terms


def _backward(e, a, p, n, margin, u=1.0):
    n_rows, dim = e.shape
    T = a.numel()
    ws = torch.empty(2 * T, dtype=torch.float32, device=e.device)
    dE = torch.empty_like(e)
    N.check(N.lib().fr_triplet_loss_backward(N.ptr(e), n_rows, dim, N.ptr(a), N.ptr(p), N.ptr(n), T, float(margin),
                                             float(u), N.ptr(dE), N.ptr(ws), 8 * T, N.stream_ptr(e.device)),
            "fr_triplet_loss_backward")
    return dE


class _Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, embeddings, a, p, n, margin):
        e = embeddings.detach().contiguous()
        stats, _ = _forward(e, a, p, n, margin)
        ctx.save_for_backward(e, a, p, n)
        ctx.margin = margin
        ctx.mark_non_differentiable(stats)
        return stats[0].clone(), stats

    @staticmethod
    def backward(ctx, u, _):
        e, a, p, n = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 5
        # the upstream factor stays on the device: no host synchronisation in the backward pass
        return _backward(e, a, p, n, ctx.margin).mul_(u.float()), None, None, None, None


def _loss(embeddings, a, p, n, margin):
    _check(embeddings)
    T = len(a)
    if T == 0:
        raise ValueError("triplet_loss: no triplets (nn.TripletMarginLoss would return nan)")
    dev = embeddings.device
    return _Loss.apply(embeddings, _i32(a, T, dev, "anchor indices"), _i32(p, T, dev, "positive indices"),
                       _i32(n, T, dev, "negative indices"), float(margin))


def mine_semi_hard_triplets(embeddings, labels, margin=0.2):
    """The reference's online semi-hard mining: per (anchor, positive) the nearest negative with
    d(a, p) < d(a, n) < d(a, p) + margin, else the nearest negative.  Three int64 index tensors on the embeddings'
    device (``len``, ``embeddings[a_idx]`` and ``.tolist()`` behave as the reference's lists do)."""
    a, p, n, _, _ = _mine(embeddings, labels, SEMI_HARD, margin)
    return a.long(), p.long(), n.long()


def mine_batch_hard_triplets(embeddings, labels):
    """The reference's batch-hard mining: per anchor the farthest positive and the nearest negative."""
    a, p, n, _, _ = _mine(embeddings, labels, BATCH_HARD, 1.0)
    return a.long(), p.long(), n.long()


def mine_triplets(embeddings, labels, margin=0.5):
    """facenet_model.py's mine_triplets: per (anchor, positive) the first semi-hard negative, else the FARTHEST
    negative (as the reference does); a list of (anchor, positive, negative) int tuples.  An anchor without negatives
    is skipped (the reference raises there)."""
    a, p, n, _, _ = _mine(embeddings, labels, FIRST, margin)
    return list(zip(a.tolist(), p.tolist(), n.tolist()))


def triplet_loss(embeddings, a_idx, p_idx, n_idx, margin=0.5):
    """``nn.TripletMarginLoss(margin, p=2)`` of ``embeddings[a_idx], embeddings[p_idx], embeddings[n_idx]`` without the
    three gathered copies; the backward pass writes ``dE [N, D]`` directly, every row summed in a fixed order (bitwise
    repeatable, unlike the gather's scatter-add)."""
    return _loss(embeddings, a_idx, p_idx, n_idx, margin)[0]


class TripletLoss(nn.Module):
    """The reference's TripletLoss: ``nn.TripletMarginLoss(margin, p=2)`` of three ``[T, D]`` tensors, differentiable
    in all three."""

    def __init__(self, margin=0.5):
        super().__init__()
        self.margin = margin

    def forward(self, anchor, positive, negative):
        for t in (anchor, positive, negative):
            _check(t)
        if not (anchor.shape == positive.shape == negative.shape):
            raise ValueError("TripletLoss: anchor, positive and negative must have the same [T, D] shape")
        T = anchor.shape[0]
        ident = torch.arange(3 * T, dtype=torch.int32, device=anchor.device)
        return _loss(torch.cat([anchor, positive, negative]), ident[:T], ident[T:2 * T], ident[2 * T:], self.margin)[0]

    def extra_repr(self) -> str:
        return f"margin={self.margin}"


def compute_triplet_metrics(anchor_emb, positive_emb, negative_emb):
    """train_facenet.py's compute_triplet_metrics: the share of triplets with |a - p| < |a - n| and the two mean
    distances, as Python floats."""
    for t in (anchor_emb, positive_emb, negative_emb):
        _check(t)
    T = anchor_emb.shape[0]
    with torch.no_grad():
        ident = torch.arange(3 * T, dtype=torch.int32, device=anchor_emb.device)
        e = torch.cat([anchor_emb, positive_emb, negative_emb]).contiguous()
        stats, _ = _forward(e, ident[:T], ident[T:2 * T], ident[2 * T:], 1.0)
    _, acc, pos, neg = stats.tolist()
    return {"accuracy": acc, "pos_dist": pos, "neg_dist": neg}


def online_triplet_loss(embeddings, labels, margin=0.2, mining="semi_hard", loss_margin=None):
    """One reference training step's mining, loss and metrics: ``(loss, info)`` with ``info = {'triplets', 'accuracy',
    'pos_dist', 'neg_dist', 'semi_hard_fraction'}``.  The mining runs under ``no_grad`` on the detached embeddings;
    ``loss`` is differentiable in ``embeddings`` and is ``None`` when the batch has no triplets (the reference skips
    such a batch).  mining: 'semi_hard' | 'batch_hard' ('hard'); loss_margin: the criterion's margin where it differs
    from the mining's (the reference's step mines with one margin and builds its TripletLoss with another)."""
    if mining not in _MODES:
        raise ValueError(f"online_triplet_loss: mining must be one of {sorted(_MODES)}, not {mining!r}")
    with torch.no_grad():
        a, p, n, semi, _ = _mine(embeddings, labels, _MODES[mining], margin)
    T = a.numel()
    if T == 0:
        return None, {"triplets": 0, "accuracy": 0.0, "pos_dist": 0.0, "neg_dist": 0.0, "semi_hard_fraction": 0.0}
    loss, stats = _Loss.apply(embeddings, a, p, n, float(margin if loss_margin is None else loss_margin))
    _, acc, pos, neg = stats.tolist()
    return loss, {"triplets": T, "accuracy": acc, "pos_dist": pos, "neg_dist": neg,
                  "semi_hard_fraction": float(semi.float().mean().item())}
