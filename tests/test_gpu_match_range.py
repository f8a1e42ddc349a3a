"""Threshold (range) search and the gallery self-join on the GPU (fr_match_range_count / _fill,
fr_gallery_read; DeviceGallery.range_search / self_pairs / reconstruct_n).

Exact-grid inputs (test_gpu_match_eval's): every row has 256 entries of +-1/16 among 512, so every score is
a multiple of 1/256, exact in f32 in any summation order, and a numpy float64 oracle must be matched
exactly.  Float inputs: the result must be, bit for bit, the subset of fr_match_topk(k = N)'s scores at or
above the threshold.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_match_eval import float_case, grid_case

pytestmark = pytest.mark.gpu

T = 0.0625  # 16/256
STEP = 1.0 / 256
SENT_S, SENT_I, GUARD = 7.5, -7, 64


def oracle_range(S, t, after=None):
    """(lims, idx, scores) of S >= t per probe, index ascending; after[b]: only columns > after[b]."""
    lims, idx, sc = [0], [], []
    for b in range(S.shape[0]):
        keep = S[b] >= t
        if after is not None:
            keep &= np.arange(S.shape[1]) > after[b]
        j = np.nonzero(keep)[0]
        idx.append(j)
        sc.append(S[b, j])
        lims.append(lims[-1] + len(j))
    return np.array(lims, np.int64), np.concatenate(idx).astype(np.int64), np.concatenate(sc)


def run(gal, P, t, after=None):
    import torch

    a = None if after is None else torch.from_numpy(np.asarray(after).astype(np.int32))
    l, s, i = gal.range_search_device(torch.from_numpy(P).to(gal.device), t, a)
    torch.cuda.synchronize()
    return l.cpu().numpy(), s.cpu().numpy(), i.cpu().numpy().astype(np.int64)


def raw(gal, P, t, after=None, capacity=None):
    """The two C calls with sentinel-filled outputs GUARD elements longer than the total:
    (lims after count, lims after fill, scores, idx, total)."""
    import torch
    from facerecognition_amd import _native as NL

    L, dev, B = NL.lib(), gal.device, len(P)
    p = torch.from_numpy(P).to(dev)
    a = None if after is None else torch.from_numpy(np.asarray(after).astype(np.int32)).to(dev)
    nbytes = L.fr_match_range_workspace(gal._h, B)
    assert nbytes == 4 * B * L.fr_debug_match_range_splits(gal._h, B)
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    lims = torch.full((B + 1,), -1, dtype=torch.int64, device=dev)
    NL.check(L.fr_match_range_count(gal._h, NL.ptr(p), B, t, NL.ptr(a), NL.ptr(ws), NL.ptr(lims), NL.stream_ptr(dev)),
             "fr_match_range_count")
    l0 = lims.cpu().numpy().copy()
    total = int(l0[-1])
    s = torch.full((total + GUARD,), SENT_S, dtype=torch.float32, device=dev)
    i = torch.full((total + GUARD,), SENT_I, dtype=torch.int32, device=dev)
    NL.check(L.fr_match_range_fill(gal._h, NL.ptr(p), B, t, NL.ptr(a), NL.ptr(ws), NL.ptr(lims), NL.ptr(s), NL.ptr(i),
                                   total if capacity is None else capacity, NL.stream_ptr(dev)), "fr_match_range_fill")
    torch.cuda.synchronize()
    return l0, lims.cpu().numpy(), s.cpu().numpy(), i.cpu().numpy(), total


@pytest.fixture(scope="module")
def cases(gpu):
    """The grid cases, their float64 scores and their device results at T, computed once."""
    from facerecognition_amd.gallery import DeviceGallery

    out = {}
    for name, (seed, B, N) in {"one_split": (1, 70, 333), "splits": (2, 70, 4167), "tiles": (3, 70, 8269)}.items():
        G, P, _ = grid_case(seed, B, N)
        gal = DeviceGallery(G)
        S = P.astype(np.float64) @ G.astype(np.float64).T
        out[name] = dict(G=G, P=P, gal=gal, S=S, got=run(gal, P, T), B=B, N=N)
    return out


def assert_equal_result(got, want):
    l, s, i = got
    wl, wi, ws = want
    assert np.array_equal(l, wl)
    assert np.array_equal(i, wi)
    assert s.dtype == np.float32 and np.array_equal(s.astype(np.float64), ws)


# 1
@pytest.mark.parametrize("name,t", [("one_split", T), ("splits", T), ("tiles", T), ("one_split", 0.125)])
def test_grid_matches_float64_oracle(cases, name, t):
    from facerecognition_amd import _native as NL

    c = cases[name]
    S = c["S"]
    assert np.array_equal(S.astype(np.float32).astype(np.float64), S)  # the grid is exact in f32
    n_split = NL.lib().fr_debug_match_range_splits(c["gal"]._h, c["B"])
    assert n_split == NL.lib().fr_debug_match_eval_splits(c["gal"]._h, c["B"])  # the same split plan
    tiles = (c["N"] + 63) // 64
    if name == "one_split":
        assert tiles == 6 and c["N"] % 64 == 13  # 64 + 6 probes, 5 x 64 + 13 rows
    if name == "splits":
        assert n_split >= 2 and c["N"] % 64 != 0  # several splits, a ragged last one
    if name == "tiles":
        assert 2 <= n_split < tiles  # several tiles per split: the chunk ring wraps from tile to tile
    got = c["got"] if t == T else run(c["gal"], c["P"], t)
    want = oracle_range(S, t)
    print(f"{name} t={t}: hits {want[0][-1]}, equal to t {int(np.sum(S == t))}, one step below {int(np.sum(S == t - STEP))}")
    assert_equal_result(got, want)
    # the planted conditions really occur
    assert np.any(S == t) and np.any(S == t - STEP)
    if t == T:
        assert want[0][-1] == {"one_split": 2124, "splits": 25255, "tiles": 49245}[name]
    else:
        assert np.any(np.diff(want[0]) == 0) and np.any(np.diff(got[0]) == 0)  # probes with no hit at all


# 2
@pytest.mark.parametrize("t", [0.0, float("-inf")])
def test_zero_probes_and_zero_rows_do_not_leak(cases, t):
    """B = 70 leaves 58 dead probe slots in the second block and N = 333 leaves 51 dead columns in the last
    tile; all of them score 0.0 >= t."""
    import torch

    c = cases["one_split"]
    B, N = c["B"], c["N"]
    l0, l1, s, i, total = raw(c["gal"], c["P"], t)
    wl, wi, ws = oracle_range(c["S"], t)
    assert np.array_equal(l0, wl) and np.array_equal(l1, wl) and total == wl[-1]
    assert np.array_equal(i[:total], wi) and np.array_equal(s[:total].astype(np.float64), ws)
    assert np.all(s[total:] == SENT_S) and np.all(i[total:] == SENT_I)
    if t == float("-inf"):
        assert np.array_equal(l0, np.arange(B + 1) * N)
        ts, ti = c["gal"].search_device(torch.from_numpy(c["P"]).to(c["gal"].device), N)
        ts, ti = ts.cpu().numpy(), ti.cpu().numpy()
        o = np.argsort(ti, axis=1, kind="stable")
        assert np.array_equal(np.take_along_axis(ti, o, 1).reshape(-1), i[:total])
        assert np.array_equal(np.take_along_axis(ts, o, 1).reshape(-1).view(np.uint32), s[:total].view(np.uint32))
    else:
        assert 0 < total < B * N


# 3
@pytest.mark.parametrize("B,N,d", [(130, 1000, 512), (70, 333, 128)])
def test_float_inputs_equal_the_exact_scores(gpu, B, N, d):
    """Bit for bit the subset of search_device(P, N) with score >= thresh, sorted by index; thresh is the
    median of each case's top-20 scores.  d = 128 runs the any-D kernel."""
    import torch
    from facerecognition_amd.gallery import DeviceGallery

    G, P, _ = float_case(7, B, N, d)
    gal = DeviceGallery(G, dim=d)
    s_all, i_all = gal.search_device(torch.from_numpy(P).to(gal.device), N)
    s_all, i_all = s_all.cpu().numpy(), i_all.cpu().numpy().astype(np.int64)
    t = float(np.median(s_all[:, :20]))
    l, s, i = run(gal, P, t)
    assert 0 < l[-1] < B * N
    for b in range(B):
        keep = s_all[b] >= np.float32(t)
        o = np.argsort(i_all[b][keep], kind="stable")
        assert np.array_equal(i[l[b]:l[b + 1]], i_all[b][keep][o]), b
        assert np.array_equal(s[l[b]:l[b + 1]].view(np.uint32), s_all[b][keep][o].view(np.uint32)), b


# 3b
def test_float_multi_tile_splits_equal_one_tile_shards(gpu):
    """D = 512 float inputs with two tiles per split (the chunk ring wraps from tile to tile and into a ragged
    last tile) against the same rows installed as shards of 1000 rows, one tile per split each: with
    thresh = -inf every score comes back, so the whole-gallery CSR must be, bit for bit in scores and exactly
    in indices, the per-probe concatenation of the shards' CSRs."""
    from facerecognition_amd import _native as NL
    from facerecognition_amd.gallery import DeviceGallery

    B, N, SHARD = 70, 8269, 1000
    G, P, _ = float_case(11, B, N, 512)
    t = float("-inf")
    whole = DeviceGallery(G)
    tiles = (N + 63) // 64
    assert 2 * NL.lib().fr_debug_match_range_splits(whole._h, B) == tiles  # two tiles per split
    l, s, i = run(whole, P, t)
    assert np.array_equal(l, np.arange(B + 1) * N)
    s, i = s.reshape(B, N), i.reshape(B, N)
    for base in range(0, N, SHARD):
        n = min(SHARD, N - base)
        shard = DeviceGallery(G[base:base + n], index_base=base)
        assert NL.lib().fr_debug_match_range_splits(shard._h, B) == (n + 63) // 64  # one tile per split
        sl, ss, si = run(shard, P, t)
        assert np.array_equal(sl, np.arange(B + 1) * n)
        assert np.array_equal(si.reshape(B, n), i[:, base:base + n]), base
        assert np.array_equal(ss.reshape(B, n).view(np.uint32), s[:, base:base + n].view(np.uint32)), base
        shard.close()
    assert np.array_equal(i, np.broadcast_to(np.arange(N), (B, N)))


# 4
def test_capacity_truncates_at_the_end(cases):
    c = cases["splits"]
    fl, fs, fi = c["got"]
    cap = int(fl[-1]) // 2
    l0, l1, s, i, total = raw(c["gal"], c["P"], T, capacity=cap)
    assert total == fl[-1] and 0 < cap < total
    assert np.array_equal(l0, fl) and np.array_equal(l1, fl)  # lims unchanged by fill
    assert np.array_equal(s[:cap].view(np.uint32), fs[:cap].view(np.uint32)) and np.array_equal(i[:cap], fi[:cap])
    assert np.all(s[cap:] == SENT_S) and np.all(i[cap:] == SENT_I)


# 5
def test_after_and_the_self_join(cases):
    c = cases["splits"]
    G, N = c["G"], c["N"]
    S = np.triu(G.astype(np.float64) @ G.astype(np.float64).T, 1)
    for t, n_pairs in ((1.0, 24), (0.125, 23022)):
        wi, wj = np.nonzero(S >= t)  # row-major: (i, j) ascending
        assert len(wi) == n_pairs
        i, j, s = c["gal"].self_pairs(t, chunk=1000)  # 5 probe chunks, the last one of 167 rows
        assert np.all(i < j)
        assert np.array_equal(i, wi) and np.array_equal(j, wj)
        assert np.array_equal(s.astype(np.float64), S[wi, wj])
    assert np.all(S[np.nonzero(S >= 1.0)] == 1.0)  # the planted copies


# 6
@pytest.mark.parametrize("nb", [1, 3])
def test_small_batch_equals_batch_rows(cases, nb):
    c = cases["splits"]
    fl, fs, fi = c["got"]
    l, s, i = run(c["gal"], c["P"][:nb], T)
    assert np.array_equal(l, fl[:nb + 1])
    assert np.array_equal(i, fi[:fl[nb]]) and np.array_equal(s.view(np.uint32), fs[:fl[nb]].view(np.uint32))


# 7
def test_sharded_gallery_after_is_global_and_piecewise_add(cases):
    from facerecognition_amd.gallery import DeviceGallery

    c = cases["one_split"]
    B, N, base = c["B"], c["N"], 1000
    gal = DeviceGallery(c["G"], index_base=base)
    l, s, i = run(gal, c["P"], T)
    fl, fs, fi = c["got"]
    assert np.array_equal(l, fl) and np.array_equal(i, fi + base) and i.min() >= base
    assert np.array_equal(s.view(np.uint32), fs.view(np.uint32))
    # after in the global index space: local bound 100 + b, some below the shard (keep all), some past it (none)
    after = base + 100 + np.arange(B)
    after[0], after[1], after[2] = 500, -1, base + N
    got = run(gal, c["P"], T, after)
    wl, wi, ws = oracle_range(c["S"], T, after - base)
    assert wl[1] - wl[0] == fl[1] - fl[0] and wl[3] == wl[2] and wl[-1] < fl[-1]
    assert_equal_result(got, (wl, wi + base, ws))
    # rows added in two pieces (the second append re-grows the allocation)
    two = DeviceGallery(c["G"][:200])
    two.add(c["G"][200:])
    l2, s2, i2 = run(two, c["P"], T)
    assert np.array_equal(l2, fl) and np.array_equal(i2, fi) and np.array_equal(s2.view(np.uint32), fs.view(np.uint32))


# 8
def test_reconstruct_n(cases):
    import torch
    from facerecognition_amd import _native as NL
    from facerecognition_amd.gallery import DeviceGallery

    c = cases["one_split"]
    gal, G, N = c["gal"], c["G"], c["N"]
    assert np.array_equal(gal.reconstruct_n(0, N).view(np.uint32), G.view(np.uint32))  # norm exactly 1: as installed
    part = gal.reconstruct_n(100, 37, device=True)
    assert part.is_cuda and np.array_equal(part.cpu().numpy().view(np.uint32), G[100:137].view(np.uint32))
    assert gal.reconstruct_n(N, 0).shape == (0, 512)
    rows = G[:3].copy()
    rows[1] *= 2.0  # norm 2: stored divided by its norm
    g2 = DeviceGallery(rows)
    assert np.array_equal(g2.reconstruct_n(), G[:3])
    # a range outside the gallery, at the C boundary
    out = torch.zeros(2 * 512)
    for row0, n in ((N, 1), (N - 1, 2), (N + 1, 0), (0, N + 1)):
        assert NL.lib().fr_gallery_read(gal._h, row0, n, NL.ptr(out), 0) == -1
        assert b"fr_gallery_read" in NL.lib().fr_last_error()
    with pytest.raises(IndexError):
        gal.reconstruct_n(N - 1, 2)


# 9
def test_order_score_is_the_prefix_of_search(cases):
    c = cases["one_split"]
    B, N = c["B"], c["N"]
    lims, D, I = c["gal"].range_search(c["P"], T, order="score", chunk=32)  # 3 probe chunks
    assert I.dtype == np.int64 and D.dtype == np.float32 and lims.dtype == np.int64
    assert np.array_equal(lims, c["got"][0])
    s_all, i_all = c["gal"].search(c["P"], N)
    ties = 0
    for b in range(B):
        n = lims[b + 1] - lims[b]
        assert np.array_equal(I[lims[b]:lims[b + 1]], i_all[b, :n]), b
        assert np.array_equal(D[lims[b]:lims[b + 1]].view(np.uint32), s_all[b, :n].view(np.uint32)), b
        ties += int(np.sum(np.diff(s_all[b, :n]) == 0))
    assert ties > 0  # the index tie-break is exercised
    # order="index" through the numpy interface, max_hits, and the empty cases
    l2, D2, I2 = c["gal"].range_search(c["P"], T, chunk=32)
    assert np.array_equal(l2, lims) and np.array_equal(I2, c["got"][2]) and np.array_equal(D2, c["got"][1])
    with pytest.raises(RuntimeError):
        c["gal"].range_search(c["P"], T, max_hits=int(lims[-1]) - 1)
    c["gal"].range_search(c["P"], T, max_hits=int(lims[-1]))
    l0, D0, I0 = c["gal"].range_search(np.zeros((0, 512), np.float32), T)
    assert np.array_equal(l0, [0]) and len(D0) == 0 and len(I0) == 0
    from facerecognition_amd.gallery import DeviceGallery
    l0, D0, I0 = DeviceGallery().range_search(c["P"][:4], T)
    assert np.array_equal(l0, np.zeros(5)) and len(D0) == 0 and len(I0) == 0


# 10
def test_engine_recognize_all_and_duplicates(cases):
    from facerecognition_amd.recognition_engine import RecognitionEngine, UnifiedRecognitionEngine

    c = cases["one_split"]
    G, P, S = c["G"], c["P"], c["S"]
    names = [f"id{n:03d}" for n in range(40)]
    db = {nm: G[n].copy() for n, nm in enumerate(names)}
    db["id005_again"] = G[5].copy()  # a second folder of the same person
    eng = RecognitionEngine(model_path=None, use_face_detection=False, threshold=0.125)
    assert eng.recognize_all_with_db(P[0]) == []  # no database
    eng.db = db
    assert UnifiedRecognitionEngine.recognize_all_with_db is RecognitionEngine.recognize_all_with_db
    best = S[:, :40].max(axis=1)
    seen = set()
    for b in list(np.nonzero(best >= 0.125)[0][:3]) + list(np.nonzero(best < 0.125)[0][:3]):
        name, score, top = eng.recognize_with_db(P[b])
        hits = eng.recognize_all_with_db(P[b])
        seen.add(name == "Unknown")
        assert (hits == []) == (name == "Unknown")
        if hits:
            assert hits[0] == (name, score)
            assert hits[:5] == top[:len(hits[:5])]
            assert all(s >= 0.125 for _, s in hits)
            want = [n for n in range(40) if S[b, n] >= 0.125]
            assert sorted(h[0] for h in hits if h[0] != "id005_again") == [names[n] for n in want]
        # an explicit threshold below every score lists the whole db, in recognize_with_db's order
        everyone = eng.recognize_all_with_db(P[b], threshold=-1.0)
        assert len(everyone) == 41 and everyone[:5] == top
    assert seen == {True, False}
    dup = eng.find_duplicate_identities(0.999)
    assert dup == [("id005", "id005_again", 1.0)]
    many = eng.find_duplicate_identities(0.125)
    assert many[0] == dup[0] and [m[2] for m in many] == sorted((m[2] for m in many), reverse=True)
    Sg = np.triu(np.vstack([G[:40], G[5:6]]).astype(np.float64) @ np.vstack([G[:40], G[5:6]]).astype(np.float64).T, 1)
    assert len(many) == int(np.sum(Sg >= 0.125))
