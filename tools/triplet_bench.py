#!/usr/bin/env python3
"""Time the device triplet mining and loss (DESIGN.md §4 "Triplet mining and loss") at the reference's training-step
shape (N, D) = (128, 512) (32 identities x 4 images, margin 0.5) and at a pool shape (8192, 512), 4 rows per identity.

Per shape one JSON line, every time hipEvent-timed on the launching stream, the median of --runs (>= 50) after 10
warm-ups with [min, max]:
  mine_ms        fr_triplet_count + fr_triplet_mine (semi-hard) on preallocated buffers
  mine_api_ms    facerecognition_amd.mine_semi_hard_triplets: the same plus allocations and the read-back of T
  hard_ms        fr_triplet_count + fr_triplet_mine (batch-hard)
  loss_fwd_ms / loss_bwd_ms   fr_triplet_loss_forward / fr_triplet_loss_backward on the mined triplets
  loop_ms        THE COMPARATOR OF THE MINING: our own restatement, in torch ops on the same GPU, of the reference's
                 mine_semi_hard_triplets (torch.cdist, then a Python loop over every (anchor, positive) pair with a host
                 synchronisation per pair).  It is a restatement, not the reference's file.  At the pool shape it takes
                 seconds per call, so it is run --loop-runs times after one warm-up there.
  torch_fwd_ms / torch_bwd_ms  the comparator of the loss: embeddings[idx] three times, F.triplet_margin_loss, autograd
plus same_triplets (the comparator's lists equal the device's: a sanity check, not a test; the two may differ where
float32 ties or near-ties are ordered differently by cdist) and loss_rel_diff.
Reads nothing outside the repository.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def event_ms(fn, runs, warm=10):
    import torch
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(float(np.median(ms)), 4), [round(min(ms), 4), round(max(ms), 4)]


def loop_semi_hard(embeddings, labels, margin):
    """The reference's mine_semi_hard_triplets restated (same torch ops, same loop, same .item() calls)."""
    import torch
    B = embeddings.size(0)
    dist = torch.cdist(embeddings, embeddings, p=2)
    ar = torch.arange(B, device=embeddings.device)
    out_a, out_p, out_n = [], [], []
    for i in range(B):
        pos = torch.where((labels == labels[i]) & (ar != i))[0]
        if len(pos) == 0:
            continue
        neg = torch.where(labels != labels[i])[0]
        if len(neg) == 0:
            continue
        for p in pos:
            ap = dist[i, p]
            nd = dist[i, neg]
            mask = (nd > ap) & (nd < ap + margin)
            n = neg[mask][nd[mask].argmin()] if mask.any() else neg[nd.argmin()]
            out_a.append(i)
            out_p.append(p.item())
            out_n.append(n.item())
    return out_a, out_p, out_n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, nargs="+", default=["128,512", "8192,512"])
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--loop-runs", type=int, default=3)
    ap.add_argument("--margin", type=float, default=0.5)
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F

    import facerecognition_amd as fra
    from facerecognition_amd import _native as NL
    from facerecognition_amd import triplet as T

    if not torch.cuda.is_available():
        raise SystemExit("triplet_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    L, st = NL.lib(), NL.stream_ptr(dev)
    for shape in a.shapes:
        N, D = (int(v) for v in shape.split(","))
        g = torch.Generator(device=dev).manual_seed(N)
        centres = torch.randn((N // 4, D), device=dev, generator=g)
        e = F.normalize(centres.repeat_interleave(4, 0) + 0.8 * torch.randn((N, D), device=dev, generator=g))
        y = torch.arange(N, device=dev) // 4
        y32 = y.to(torch.int32)
        torch.cuda.synchronize()

        ia, ip, in_, semi, lims = T._mine(e, y, T.SEMI_HARD, a.margin)
        n_trip = ia.numel()
        nbytes = int(L.fr_triplet_workspace(N, D))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)

        def mine(mode):
            NL.check(L.fr_triplet_count(NL.ptr(y32), N, mode, NL.ptr(lims), st), "fr_triplet_count")
            NL.check(L.fr_triplet_mine(NL.ptr(e), N, D, NL.ptr(y32), mode, a.margin, NL.ptr(lims), NL.ptr(ia), NL.ptr(ip),
                                       NL.ptr(in_), n_trip, NL.ptr(semi), NL.ptr(ws), nbytes, st), "fr_triplet_mine")

        hard, hard_s = event_ms(lambda: mine(T.BATCH_HARD), a.runs)
        mine_ms, mine_s = event_ms(lambda: mine(T.SEMI_HARD), a.runs)  # last: ia, ip, in_ hold the semi-hard triplets
        api, api_s = event_ms(lambda: fra.mine_semi_hard_triplets(e, y, a.margin), a.runs)
        semi_share = float(semi.float().mean())

        terms = torch.empty((n_trip, 4), device=dev)
        stats = torch.empty(4, device=dev)
        coef = torch.empty(2 * n_trip, device=dev)
        dE = torch.empty_like(e)

        def fwd():
            NL.check(L.fr_triplet_loss_forward(NL.ptr(e), N, D, NL.ptr(ia), NL.ptr(ip), NL.ptr(in_), n_trip, a.margin,
                                               NL.ptr(terms), NL.ptr(stats), st), "fr_triplet_loss_forward")

        def bwd():
            NL.check(L.fr_triplet_loss_backward(NL.ptr(e), N, D, NL.ptr(ia), NL.ptr(ip), NL.ptr(in_), n_trip, a.margin, 1.0,
                                                NL.ptr(dE), NL.ptr(coef), 8 * n_trip, st), "fr_triplet_loss_backward")

        lf, lf_s = event_ms(fwd, a.runs)
        lb, lb_s = event_ms(bwd, a.runs)
        loss_f = float(stats[0])

        small = N <= 512
        loop, loop_s = event_ms(lambda: loop_semi_hard(e, y, a.margin), a.runs if small else a.loop_runs,
                                warm=10 if small else 1)
        ra, rp, rn = loop_semi_hard(e, y, a.margin)
        same = ra == ia.tolist() and rp == ip.tolist() and rn == in_.tolist()

        la, lp, ln = ia.long(), ip.long(), in_.long()
        eg = e.clone().requires_grad_(True)
        held = {}

        def tfwd():
            held["loss"] = F.triplet_margin_loss(eg[la], eg[lp], eg[ln], margin=a.margin, p=2)

        def tbwd():
            eg.grad = None
            held["loss"].backward(retain_graph=True)

        tf, tf_s = event_ms(tfwd, a.runs)
        tb, tb_s = event_ms(tbwd, a.runs)
        loss_t = float(held["loss"].detach())
        grad_diff = float((eg.grad - dE).abs().max() / eg.grad.abs().max())
        held.clear()
        out = {"N": N, "D": D, "margin": a.margin, "triplets": n_trip, "semi_hard_share": round(semi_share, 3),
               "runs": a.runs, "workspace_bytes": nbytes,
               "mine_ms": mine_ms, "mine_ms_min_max": mine_s, "mine_api_ms": api, "mine_api_ms_min_max": api_s,
               "hard_ms": hard, "hard_ms_min_max": hard_s,
               "loss_fwd_ms": lf, "loss_fwd_ms_min_max": lf_s, "loss_bwd_ms": lb, "loss_bwd_ms_min_max": lb_s,
               "loop_ms": loop, "loop_ms_min_max": loop_s, "loop_runs": a.runs if small else a.loop_runs,
               "torch_fwd_ms": tf, "torch_fwd_ms_min_max": tf_s, "torch_bwd_ms": tb, "torch_bwd_ms_min_max": tb_s,
               "same_triplets": bool(same), "loss_rel_diff": abs(loss_f - loss_t) / max(abs(loss_t), 1e-30),
               "grad_rel_diff": grad_diff, "device": torch.cuda.get_device_name(dev)}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
