"""fr_match_eval on the GPU: true-row score, true-row rank and impostor histogram.

Exact-grid inputs: every gallery row and probe has 256 entries of +-1/16 among 512 (norm exactly 1, every
dot product a multiple of 1/256 and exact in f32 in any summation order), so an independent numpy float64
oracle must be matched exactly, ties and index tie-breaks included.  Float inputs: the outputs must equal
what fr_match_topk(k = N) -- every exact score, sorted -- implies, bit for bit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 512
LO, HI, NBINS = -1.0, 1.0, 512  # (s + 1) * 256 is an integer for grid scores: none sits near a bin edge
K = 5


def grid_rows(rng, n):
    """n rows with 256 entries of +-1/16 at random places among 512."""
    rows = np.zeros((n, D), np.float32)
    for r in range(n):
        pos = rng.choice(D, 256, replace=False)
        rows[r, pos] = rng.choice(np.array([-0.0625, 0.0625], np.float32), 256)
    return rows


def grid_case(seed, B, N):
    """Gallery, probes and true rows: half the probes are their true row with 20..120 sign flips (ranks
    0, 1-4, 5-16 and beyond), half have a random true row; a few true rows are copied to one lower and one
    higher gallery index (equal scores: the index tie-break decides)."""
    rng = np.random.default_rng(seed)
    G = grid_rows(rng, N)
    true = rng.integers(N // 4, 3 * N // 4, B)
    for b in range(0, B, 9):
        lo_i, hi_i = int(rng.integers(0, N // 4)), int(rng.integers(3 * N // 4, N))
        G[lo_i] = G[true[b]]
        G[hi_i] = G[true[b]]
    P = grid_rows(rng, B)
    for b in range(0, B, 2):
        P[b] = G[true[b]]
        nz = np.flatnonzero(P[b])
        flip = rng.choice(nz, int(rng.integers(20, 121)), replace=False)
        P[b, flip] = -P[b, flip]
    return G, P, true.astype(np.int64)


def oracle(P, G, true_local, lo=LO, hi=HI, nbins=NBINS):
    """float64: scores, true score, rank in (score desc, index asc) order, impostor histogram.
    true_local < 0 or >= N: the probe's true row is not in the gallery."""
    S = P.astype(np.float64) @ G.astype(np.float64).T
    B, N = S.shape
    ts = np.full(B, -np.inf)
    rank = np.full(B, -1, np.int64)
    hist = np.zeros(nbins, np.int64)
    j = np.arange(N)
    for b in range(B):
        t = int(true_local[b])
        imp = np.ones(N, bool)
        if 0 <= t < N:
            ts[b] = S[b, t]
            imp[t] = False
            rank[b] = np.sum(imp & ((S[b] > ts[b]) | ((S[b] == ts[b]) & (j < t))))
        bins = np.clip(np.floor((S[b, imp] - lo) * (nbins / (hi - lo))).astype(np.int64), 0, nbins - 1)
        hist += np.bincount(bins, minlength=nbins)
    return S, ts, rank, hist


def run(gal, P, true_global, k=K, hist_bins=NBINS, hist_range=(LO, HI), hist=None):
    import torch

    r = gal.evaluate_device(torch.from_numpy(P).to(gal.device), torch.from_numpy(true_global.astype(np.int32)), k,
                            hist_bins, hist_range, hist)
    torch.cuda.synchronize()
    return {key: (None if v is None else v.cpu().numpy()) for key, v in r.items()}


def check_invariants(r, true_global, B, N, k, n_in_shard):
    """true_rank < k <=> true_idx in idx[:, :k], at position true_rank with true_score's bits; the
    histogram holds every pair but the true ones."""
    for b in range(B):
        t, rk = int(true_global[b]), int(r["true_rank"][b])
        inside = t in r["idx"][b, :k].tolist()
        assert inside == (0 <= rk < k), (b, t, rk, r["idx"][b])
        if inside:
            assert r["idx"][b, rk] == t
            assert r["scores"][b, rk].view(np.uint32) == r["true_score"][b].view(np.uint32), b
    if r["hist"] is not None:
        assert int(r["hist"].sum()) == B * N - n_in_shard


@pytest.fixture(scope="module")
def cases(gpu):
    """The grid cases, their oracle and their device results, computed once."""
    from facerecognition_amd.gallery import DeviceGallery

    out = {}
    for name, (seed, B, N) in {"one_split": (1, 70, 333), "splits": (2, 70, 4167), "tiles": (3, 70, 8269)}.items():
        G, P, true = grid_case(seed, B, N)
        gal = DeviceGallery(G)
        out[name] = dict(G=G, P=P, true=true, gal=gal, oracle=oracle(P, G, true), got=run(gal, P, true), B=B, N=N)
    return out


@pytest.mark.parametrize("name", ["one_split", "splits", "tiles"])
def test_grid_matches_float64_oracle(cases, name):
    from facerecognition_amd import _native as NL

    c = cases[name]
    S, ts, rank, hist = c["oracle"]
    r = c["got"]
    assert np.array_equal(S.astype(np.float32).astype(np.float64), S)  # the grid is exact in f32
    n_split = NL.lib().fr_debug_match_eval_splits(c["gal"]._h, c["B"])
    tiles = (c["N"] + 63) // 64
    if name == "one_split":
        assert tiles == 6 and c["N"] % 64 == 13  # 64 + 6 probes, 5 x 64 + 13 rows
    if name == "splits":
        assert n_split >= 2 and c["N"] % 64 != 0  # several splits, a ragged last one
    if name == "tiles":
        assert 2 <= n_split < tiles  # several tiles per split: the chunk ring wraps from tile to tile
    assert np.array_equal(r["true_score"].astype(np.float64), ts)
    assert np.array_equal(r["true_rank"].astype(np.int64), rank)
    assert np.array_equal(r["hist"], hist)
    check_invariants(r, c["true"], c["B"], c["N"], K, c["B"])
    # the planted cases really occur: ties on the true score, and every rank range
    ties = sum(int(np.sum(S[b] == ts[b])) > 1 for b in range(c["B"]))
    assert ties >= c["B"] // 9
    assert np.any(rank == 0) and np.any((rank >= 1) & (rank <= 16)) and np.any(rank > 16)


@pytest.mark.parametrize("nb", [1, 3])
def test_small_batch_equals_batch_rows(cases, nb):
    """B <= 4 (the rows-kernel top-k): a probe evaluated alone gives what it gives inside a batch."""
    c = cases["splits"]
    r = run(c["gal"], c["P"][:nb], c["true"][:nb])
    g = c["got"]
    assert np.array_equal(r["true_score"].view(np.uint32), g["true_score"][:nb].view(np.uint32))
    assert np.array_equal(r["true_rank"], g["true_rank"][:nb])
    assert np.array_equal(r["scores"].view(np.uint32), g["scores"][:nb].view(np.uint32))
    assert np.array_equal(r["idx"], g["idx"][:nb])
    assert np.array_equal(r["hist"], oracle(c["P"][:nb], c["G"], c["true"][:nb])[3])
    check_invariants(r, c["true"][:nb], nb, c["N"], K, nb)


def float_case(seed, B, N, d):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((N, d)).astype(np.float32)
    G /= np.linalg.norm(G, axis=1, keepdims=True)
    true = rng.integers(0, N, B)
    P = rng.standard_normal((B, d)).astype(np.float32)
    P[::2] = G[true[::2]] + rng.uniform(0.02, 0.12, (len(true[::2]), 1)).astype(np.float32) * P[::2]  # noisy matches
    P /= np.linalg.norm(P, axis=1, keepdims=True)
    return G.astype(np.float32), P.astype(np.float32), true.astype(np.int64)


@pytest.mark.parametrize("B,N,d", [(130, 1000, 512), (70, 333, 128)])
def test_float_inputs_equal_the_exact_scores(gpu, B, N, d):
    """fr_match_topk(k = N) returns every exact score, sorted: the position of the true row is the rank,
    its score the true score, and the bin rule in numpy float32 over the rest the histogram."""
    import torch
    from facerecognition_amd.gallery import DeviceGallery

    lo, hi, nbins = -0.05, 0.1, 300  # impostor scores fall outside on both sides: both clamps; edges not on a grid
    G, P, true = float_case(7, B, N, d)
    gal = DeviceGallery(G, dim=d)
    s_all, i_all = gal.search_device(torch.from_numpy(P).to(gal.device), N)
    s_all, i_all = s_all.cpu().numpy(), i_all.cpu().numpy()
    r = run(gal, P, true, hist_bins=nbins, hist_range=(lo, hi))
    pos = np.array([int(np.flatnonzero(i_all[b] == true[b])[0]) for b in range(B)])
    assert np.array_equal(r["true_rank"], pos)
    assert np.array_equal(r["true_score"].view(np.uint32), s_all[np.arange(B), pos].view(np.uint32))
    inv_w = np.float32(nbins) / (np.float32(hi) - np.float32(lo))
    imp = np.ones((B, N), bool)
    imp[np.arange(B), pos] = False
    x = (s_all[imp] - np.float32(lo)).astype(np.float32) * inv_w
    assert x.dtype == np.float32
    bins = np.clip(np.floor(x).astype(np.int64), 0, nbins - 1)
    want = np.bincount(bins, minlength=nbins)
    assert want[0] > 0 and want[-1] > 0
    assert np.array_equal(r["hist"], want)
    check_invariants(r, true, B, N, K, B)


def test_bf16x3_topk_path_keeps_the_invariants(cases):
    from facerecognition_amd.gallery import DeviceGallery

    c = cases["splits"]
    gal = DeviceGallery(c["G"], x3_min_rows=1024)
    r = run(gal, c["P"], c["true"])
    print(f"bf16x3 top-k under fr_match_eval: fallbacks() = {gal.fallbacks()}")
    S, ts, rank, hist = c["oracle"]
    assert np.array_equal(r["true_score"].astype(np.float64), ts)
    assert np.array_equal(r["true_rank"].astype(np.int64), rank)
    assert np.array_equal(r["hist"], hist)
    assert np.array_equal(r["idx"], c["got"]["idx"])
    check_invariants(r, c["true"], c["B"], c["N"], K, c["B"])


def test_sharded_gallery_and_rows_outside_it(cases):
    from facerecognition_amd.gallery import DeviceGallery

    c = cases["one_split"]
    B, N, base = c["B"], c["N"], 1000
    gal = DeviceGallery(c["G"], index_base=base)
    tg = c["true"] + base
    tg[0] = 500  # another shard's row
    tg[1] = -1
    r = run(gal, c["P"], tg)
    S, ts, rank, hist = oracle(c["P"], c["G"], tg - base)
    assert np.isneginf(r["true_score"][:2]).all() and (r["true_rank"][:2] == -1).all()
    assert np.array_equal(r["true_score"].astype(np.float64), ts)
    assert np.array_equal(r["true_rank"].astype(np.int64), rank)
    assert np.array_equal(r["hist"], hist)
    assert int(r["hist"].sum()) == B * N - (B - 2)
    assert r["idx"].min() >= base
    check_invariants(r, tg, B, N, K, B - 2)


def test_histogram_accumulates_and_topk_is_optional(cases):
    import torch

    c = cases["splits"]
    g = c["got"]
    a = c["gal"].evaluate_device(torch.from_numpy(c["P"][:40]).to(c["gal"].device),
                                 torch.from_numpy(c["true"][:40].astype(np.int32)), K, NBINS, (LO, HI))
    b = run(c["gal"], c["P"][40:], c["true"][40:], hist=a["hist"])
    assert np.array_equal(b["hist"], g["hist"])
    assert np.array_equal(b["true_rank"], g["true_rank"][40:])
    # no histogram, no top-k: score and rank still filled
    r = run(c["gal"], c["P"], c["true"], k=0, hist_bins=0)
    assert r["scores"] is None and r["idx"] is None and r["hist"] is None
    assert np.array_equal(r["true_score"].view(np.uint32), g["true_score"].view(np.uint32))
    assert np.array_equal(r["true_rank"], g["true_rank"])
    # the C entry point with k = 0 and hist = NULL: the caller's scores / idx buffers stay as they were
    from facerecognition_amd import _native as NL

    dev, B = c["gal"].device, c["B"]
    p = torch.from_numpy(c["P"]).to(dev)
    t = torch.from_numpy(c["true"].astype(np.int32)).to(dev)
    s = torch.full((B, K), 7.5, dtype=torch.float32, device=dev)
    i = torch.full((B, K), -7, dtype=torch.int32, device=dev)
    ts = torch.zeros(B, dtype=torch.float32, device=dev)
    tr = torch.full((B,), 99, dtype=torch.int32, device=dev)
    NL.check(NL.lib().fr_match_eval(c["gal"]._h, NL.ptr(p), B, NL.ptr(t), 0, NL.ptr(s), NL.ptr(i), NL.ptr(ts), NL.ptr(tr),
                                    None, 0, 0.0, 0.0, NL.stream_ptr(dev)), "fr_match_eval")
    torch.cuda.synchronize()
    assert bool((s == 7.5).all()) and bool((i == -7).all())
    assert np.array_equal(ts.cpu().numpy().view(np.uint32), g["true_score"].view(np.uint32))
    assert np.array_equal(tr.cpu().numpy(), g["true_rank"])


def test_evaluate_closed_set_reports_the_oracle(cases):
    from facerecognition_amd import evaluate_closed_set

    c = cases["splits"]
    S, ts, rank, hist = c["oracle"]
    rep = evaluate_closed_set(c["gal"], c["P"], c["true"], hist_bins=NBINS, hist_range=(LO, HI), max_rank=20)
    assert rep["top1_acc"] == float(np.mean(rank == 0)) and rep["top5_acc"] == float(np.mean(rank < 5))
    assert np.array_equal(rep["cmc"], np.array([np.mean(rank <= q) for q in range(20)]))
    assert rep["impostor_pairs"] == c["B"] * (c["N"] - 1)
    assert np.array_equal(rep["device"]["hist"], hist)
    assert rep["far"][0] == 1.0 and rep["far"][-1] == 0.0
