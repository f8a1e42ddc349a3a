"""The batched detector with its box logic on the device (nms_device.hip, mtcnn_boxes.hip,
DeviceMTCNN.detect_batch, FaceDetector.detect_batch, RecognitionEngine.recognize_frames).  The yardsticks are the
existing host functions -- fr_nms_host behind FD.nms, the numpy lines of detect_face, DeviceMTCNN.detect_face frame
by frame -- and every comparison is exact: the device arithmetic is the host's float32 operations in the same order."""
import numpy as np
import pytest
import torch

from facerecognition_amd import _native as N
from facerecognition_amd import face_detector as FD
from tests.test_face_detector import synthetic_scene

pytestmark = pytest.mark.gpu
f32 = np.float32


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype)).cuda()


# ------------------------------------------------------------------------------------------------ fr_nms
def dev_nms(boxes, order, seg_start, thresh, mode):
    """fr_nms on host arrays -> (keep [total kept], seg_kept [n_seg + 1]) as numpy."""
    L = N.lib()
    n, n_seg = len(boxes), len(seg_start) - 1
    b, o, ss = _t(boxes, f32), _t(order, np.int64), _t(seg_start, np.int64)
    keep = torch.full((max(n, 1),), -7, dtype=torch.int64, device="cuda")
    sk = torch.full((n_seg + 1,), -7, dtype=torch.int64, device="cuda")
    nws = L.fr_nms_workspace(n, n_seg)
    ws = torch.empty((nws,), dtype=torch.uint8, device="cuda")
    N.check(L.fr_nms(N.ptr(b), n, N.ptr(o), N.ptr(ss), n_seg, float(thresh), int(mode == "min"), N.ptr(keep),
                     N.ptr(sk), N.ptr(ws), nws, N.stream_ptr()), "fr_nms")
    torch.cuda.synchronize()
    sk = sk.cpu().numpy()
    return keep.cpu().numpy()[: sk[-1]], sk


def host_order(scores, mode):
    return np.argsort(-scores, kind="stable") if mode == "iou" else np.argsort(scores)[::-1]


def random_boxes(n=300, seed=0):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 100, (n, 2)).astype(f32)
    wh = rng.uniform(5, 40, (n, 2)).astype(f32)
    scores = rng.uniform(0, 1, n).astype(f32)
    scores[10] = scores[20]  # a tie
    return np.concatenate([xy, xy + wh], 1), scores


def grid_windows():
    rng = np.random.default_rng(4)
    parts = []
    for s in (1.0, 0.7, 0.49):
        yy, xx = np.mgrid[0:30, 0:40].astype(f32)
        q1 = np.floor((2 * np.stack([xx.ravel(), yy.ravel()], 1) + 1) / s)
        q2 = np.floor((2 * np.stack([xx.ravel(), yy.ravel()], 1) + 12) / s)
        parts.append(np.concatenate([q1, q2], 1))
    boxes = np.concatenate(parts + [np.array([[5, 5, 5, 9], [50, 50, 50, 50], [80, 10, 70, 20], [7, 7, 7, 7]], f32)])
    scores = np.round(rng.uniform(0.6, 1.0, len(boxes)), 2).astype(f32)  # many exact ties
    return boxes.astype(f32), scores


@pytest.mark.parametrize("make", [random_boxes, grid_windows], ids=["random300", "grid_windows"])
@pytest.mark.parametrize("mode", ["iou", "min"])
def test_nms_equals_host_nms(gpu, make, mode):
    boxes, scores = make()
    order = host_order(scores, mode)
    for t in (0.3, 0.5, 0.7):
        ref = FD.nms(boxes, scores, t, mode)
        got, sk = dev_nms(boxes, order, [0, len(boxes)], t, mode)
        assert 0 < len(ref) < len(boxes)
        assert np.array_equal(sk, [0, len(ref)]) and np.array_equal(got, ref), (t, mode)
        again, sk2 = dev_nms(boxes, order, [0, len(boxes)], t, mode)
        assert np.array_equal(again, got) and np.array_equal(sk2, sk)  # two calls are bitwise equal


def check_segments(boxes, scores, sizes, t, mode):
    """Segments of the given sizes over consecutive boxes, against FD.nms on each segment alone."""
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert starts[-1] <= len(boxes)
    order = np.arange(len(boxes), dtype=np.int64)
    refs = []
    for s in range(len(sizes)):
        a, e = starts[s], starts[s + 1]
        order[a:e] = a + host_order(scores[a:e], mode)
        refs.append(a + FD.nms(boxes[a:e], scores[a:e], t, mode))
    got, sk = dev_nms(boxes, order, starts, t, mode)
    assert np.array_equal(sk, np.concatenate([[0], np.cumsum([len(r) for r in refs])]))
    for s, r in enumerate(refs):
        assert np.array_equal(got[sk[s]:sk[s + 1]], r), (s, sizes[s])
    return refs


@pytest.mark.parametrize("mode", ["iou", "min"])
def test_nms_segments(gpu, mode):
    boxes, scores = grid_windows()
    # unequal segments with an empty one; boxes past the last segment belong to none
    check_segments(boxes, scores, [700, 0, 1200, 37, 1500], 0.5, mode)
    # the chunk edges of the 64-candidate walk
    check_segments(boxes[1000:], scores[1000:], [1, 63, 64, 65, 129], 0.5, mode)
    rb, rs = random_boxes(300, seed=3)
    check_segments(rb, rs, [1, 63, 64, 65, 107], 0.3, mode)


def test_nms_first_box_suppresses_all_and_disjoint_boxes(gpu):
    rng = np.random.default_rng(8)
    # 150 boxes nested around one centre: the best-scoring (outermost, first) box suppresses every other in 'Min' mode
    r = np.arange(150, dtype=f32)
    nested = np.stack([100 - (60 - 0.1 * r), 100 - (60 - 0.1 * r), 100 + (60 - 0.1 * r), 100 + (60 - 0.1 * r)], 1).astype(f32)
    ns = np.linspace(1.0, 0.5, 150).astype(f32)
    for mode in ("iou", "min"):
        refs = check_segments(nested, ns, [150], 0.3, mode)
        assert np.array_equal(refs[0], [0])
    # 200 pairwise disjoint boxes, all kept: the kept list crosses the 64-lane chunks; the second segment's 1300 also
    # cross the 1024-box LDS tile
    gy, gx = np.divmod(np.arange(1500), 40)
    dis = np.stack([gx * 20, gy * 20, gx * 20 + 10, gy * 20 + 10], 1).astype(f32)
    ds = rng.uniform(0, 1, 1500).astype(f32)
    for mode in ("iou", "min"):
        refs = check_segments(dis, ds, [200, 1300], 0.5, mode)
        assert len(refs[0]) == 200 and len(refs[1]) == 1300


def test_nms_empty_input(gpu):
    got, sk = dev_nms(np.zeros((0, 4), f32), np.zeros((0,), np.int64), [0, 0, 0], 0.5, "iou")
    assert len(got) == 0 and np.array_equal(sk, [0, 0, 0])
    boxes, scores = random_boxes(64)
    got, sk = dev_nms(boxes, np.arange(64), [0, 0, 0], 0.5, "iou")  # only empty segments
    assert len(got) == 0 and np.array_equal(sk, [0, 0, 0])
    assert N.lib().fr_nms(0, 0, 0, N.ptr(_t([0], np.int64)), 0, 0.5, 0, 0, N.ptr(_t([0], np.int64)), 0, 0, None) == 0


# ------------------------------------------------------------------------------------------------ box stages
def _compact_ws(total):
    nb = N.lib().fr_mtcnn_compact_workspace(total)
    assert nb > 0
    return torch.empty((nb,), dtype=torch.uint8, device="cuda"), nb


def cand_ref(out, scale, th, level):
    """detect_face's numpy lines for one level."""
    B = out.shape[0]
    prob = out[..., 1]
    bi, yy, xx = np.nonzero(prob >= f32(th))
    sc = f32(scale)
    cell = np.stack([xx, yy], 1).astype(f32)
    q1 = np.floor((f32(2) * cell + f32(1)) / sc)
    q2 = np.floor((f32(2) * cell + f32(12)) / sc)
    return (np.concatenate([q1, q2], 1).astype(f32), prob[bi, yy, xx], out[bi, yy, xx, 2:6],
            (level * B + bi).astype(np.int32))


@pytest.mark.parametrize("shape", [(2, 9, 13), (3, 70, 90)], ids=["2x9x13", "3x70x90"])
def test_candidates_equal_numpy(gpu, shape):
    L = N.lib()
    B, hh, ww = shape
    rng = np.random.default_rng(11)
    maps = [rng.uniform(0, 0.9, (B, hh, ww, 6)).astype(f32), rng.uniform(0, 0.9, (B, hh - 2, ww - 3, 6)).astype(f32)]
    scales, th = (0.6, 0.6 * 0.709), 0.6  # about a third of the cells pass
    refs = [cand_ref(m, s, th, lvl) for lvl, (m, s) in enumerate(zip(maps, scales))]
    ref = [np.concatenate([r[k] for r in refs]) for k in range(4)]
    n_ref = len(ref[0])
    assert 0.25 < n_ref / sum(m[..., 0].size for m in maps) < 0.42
    for cap in (n_ref + 9, len(refs[0][0]) + 5):  # the second: below the pass count, inside level 1
        box = torch.full((cap + 1, 4), -5.0, device="cuda")
        score = torch.full((cap + 1,), -5.0, device="cuda")
        reg = torch.full((cap + 1, 4), -5.0, device="cuda")
        seg = torch.full((cap + 1,), -5, dtype=torch.int32, device="cuda")
        counter = torch.zeros((1,), dtype=torch.int32, device="cuda")
        seen = []
        for lvl, (m, s) in enumerate(zip(maps, scales)):
            md = _t(m)
            ws, nb = _compact_ws(m[..., 0].size)
            N.check(L.fr_mtcnn_candidates(N.ptr(md), B, m.shape[1], m.shape[2], s, th, lvl, cap, N.ptr(box),
                                          N.ptr(score), N.ptr(reg), N.ptr(seg), N.ptr(counter), N.ptr(ws), nb,
                                          N.stream_ptr()), "fr_mtcnn_candidates")
            seen.append(int(counter.cpu()[0]))
        assert seen == [len(refs[0][0]), n_ref]  # the running total, also past the capacity
        k = min(cap, n_ref)
        for got, want in zip((box, score, reg, seg), ref):
            got = got.cpu().numpy()
            assert np.array_equal(got[:k], want[:k])
            assert np.all(got[k:] == -5)  # nothing is written at or past the capacity


def boxes257(W=100, H=80):
    rng = np.random.default_rng(21)
    n = 257
    c = rng.uniform(-30, 130, (n, 2)).astype(f32)  # negative coordinates and coordinates beyond the frame
    wh = rng.uniform(4, 60, (n, 2)).astype(f32)
    b = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(f32)
    b[:12] += f32(400)   # wholly right of / below the frame: ok drops them
    b[12:20] -= f32(300)  # wholly left of / above it
    score = rng.uniform(0, 1, n).astype(f32)
    mv = rng.uniform(-0.3, 0.3, (n, 4)).astype(f32)
    inds = rng.integers(0, 3, n).astype(np.int32)
    return b, score, mv, inds


def crop_ref(b5, mv, inds, W, H, plus1):
    if plus1:
        b = FD._bbreg(b5, mv)
    else:  # the P stage's lines of detect_face
        regw, regh = b5[:, 2] - b5[:, 0], b5[:, 3] - b5[:, 1]
        b = np.stack([b5[:, 0] + mv[:, 0] * regw, b5[:, 1] + mv[:, 1] * regh, b5[:, 2] + mv[:, 2] * regw,
                      b5[:, 3] + mv[:, 3] * regh, b5[:, 4]], 1).astype(f32)
    b = FD._rerec(b)
    y, ey, x, ex = FD._pad(b, W, H)
    ok = (ey > y - 1) & (ex > x - 1)
    reg = np.stack([inds, y - 1, x - 1, ey - y + 1, ex - x + 1], 1)[ok]
    return b[ok], inds[ok], reg.astype(np.int32)


@pytest.mark.parametrize("plus1", [0, 1])
@pytest.mark.parametrize("kept", [False, True], ids=["all_rows", "keep_list"])
def test_crop_boxes_equal_numpy(gpu, plus1, kept):
    L = N.lib()
    W, H, B = 100, 80, 3
    b, score, mv, inds = boxes257(W, H)
    n = len(b)
    if kept:  # a keep list as fr_nms leaves it: box rows in some order, its length on the device
        keep = np.random.default_rng(5).permutation(n)[:190].astype(np.int64)
        keep_d, nk_d = _t(np.concatenate([keep, np.full(n - 190, 10 ** 9)]), np.int64), _t([190], np.int64)
    else:
        keep = np.arange(n)
    rb, ri, rreg = crop_ref(np.concatenate([b, score[:, None]], 1)[keep], mv[keep], inds[keep], W, H, plus1)
    assert 0 < len(rb) <= len(keep) - 8  # ok drops the boxes outside the frame
    obox = torch.full((n, 4), -5.0, device="cuda")
    oscore = torch.full((n,), -5.0, device="cuda")
    oimg = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    regions = torch.full((n, 5), -5, dtype=torch.int32, device="cuda")
    counter = torch.full((1,), -5, dtype=torch.int32, device="cuda")
    ws, nb = _compact_ws(n)
    # segment ids level * B + image on the way in: the image is id % B
    bd, sd, md, idd = _t(b), _t(score), _t(mv), _t(inds + 2 * B)
    N.check(L.fr_mtcnn_crop_boxes(N.ptr(bd), N.ptr(sd), N.ptr(md), N.ptr(idd), n, B,
                                  N.ptr(keep_d) if kept else 0, N.ptr(nk_d) if kept else 0, plus1, W, H, N.ptr(obox),
                                  N.ptr(oscore), N.ptr(oimg), N.ptr(regions), N.ptr(counter), N.ptr(ws), nb,
                                  N.stream_ptr()), "fr_mtcnn_crop_boxes")
    k = int(counter.cpu()[0])
    assert k == len(rb)
    assert np.array_equal(obox.cpu().numpy()[:k], rb[:, :4]) and np.array_equal(oscore.cpu().numpy()[:k], rb[:, 4])
    assert np.array_equal(oimg.cpu().numpy()[:k], ri) and np.array_equal(regions.cpu().numpy()[:k], rreg)
    assert np.all(obox.cpu().numpy()[k:] == -5) and np.all(regions.cpu().numpy()[k:] == -5)


@pytest.mark.parametrize("C", [6, 16])
def test_select_and_final_boxes_equal_numpy(gpu, C):
    L = N.lib()
    b, _, _, inds = boxes257()
    n = len(b)
    rng = np.random.default_rng(31)
    out = rng.uniform(-0.5, 0.5, (n, C)).astype(f32)
    out[:, 1] = rng.uniform(0.4, 1.0, n).astype(f32)
    out[7, 1] = f32(0.7)  # equal to the threshold: strict > drops it
    th = 0.7
    ip = out[:, 1] > f32(th)
    assert 50 < ip.sum() < n - 50 and not ip[7]
    obox = torch.full((n, 4), -5.0, device="cuda")
    oscore = torch.full((n,), -5.0, device="cuda")
    oreg = torch.full((n, 4), -5.0, device="cuda")
    oimg = torch.full((n,), -5, dtype=torch.int32, device="cuda")
    opts = torch.full((n, 10), -5.0, device="cuda") if C == 16 else None
    counter = torch.full((2,), -5, dtype=torch.int32, device="cuda")
    ws, nb = _compact_ws(n)
    outd, bd, idd = _t(out), _t(b), _t(inds)
    N.check(L.fr_mtcnn_select(N.ptr(outd), n, C, th, N.ptr(bd), N.ptr(idd), N.ptr(obox), N.ptr(oscore),
                              N.ptr(oreg), N.ptr(oimg), N.ptr(opts), N.ptr(counter), N.ptr(ws), nb, N.stream_ptr()),
            "fr_mtcnn_select")
    k = int(counter.cpu()[0])
    assert k == ip.sum()
    assert np.array_equal(obox.cpu().numpy()[:k], b[ip]) and np.array_equal(oscore.cpu().numpy()[:k], out[ip, 1])
    assert np.array_equal(oreg.cpu().numpy()[:k], out[ip, 2:6]) and np.array_equal(oimg.cpu().numpy()[:k], inds[ip])
    assert np.all(obox.cpu().numpy()[k:] == -5)
    if C == 6:
        return
    assert np.array_equal(opts.cpu().numpy()[:k], out[ip, 6:16])
    # the O stage's last lines of detect_face
    boxes = np.concatenate([b[ip], out[ip, 1][:, None]], 1)
    mv, pts = out[ip, 2:6], out[ip, 6:16]
    w_i = boxes[:, 2] - boxes[:, 0] + f32(1)
    h_i = boxes[:, 3] - boxes[:, 1] + f32(1)
    px = w_i[:, None] * pts[:, :5] + boxes[:, 0:1] - f32(1)
    py = h_i[:, None] * pts[:, 5:10] + boxes[:, 1:2] - f32(1)
    points = np.stack([px, py], 2).astype(f32)
    boxes = FD._bbreg(boxes, mv)
    fbox = torch.full((n, 4), -5.0, device="cuda")
    fpts = torch.full((n, 10), -5.0, device="cuda")
    N.check(L.fr_mtcnn_final_boxes(N.ptr(obox), N.ptr(oreg), N.ptr(opts), n, N.ptr(counter), N.ptr(fbox), N.ptr(fpts),
                                   N.stream_ptr()), "fr_mtcnn_final_boxes")
    assert np.array_equal(fbox.cpu().numpy()[:k], boxes[:, :4])
    assert np.array_equal(fpts.cpu().numpy()[:k].reshape(-1, 5, 2), points)
    assert np.all(fbox.cpu().numpy()[k:] == -5) and np.all(fpts.cpu().numpy()[k:] == -5)  # rows past the device count


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def dev(gpu):
    return FD.DeviceMTCNN(FD.synth_mtcnn_state(7), device=0)


SCENES = [(0, 4), (1, 3), (2, 6), (3, 2)]


@pytest.fixture(scope="module")
def scenes():
    return np.stack([synthetic_scene(seed, coarse=coarse) for seed, coarse in SCENES])


@pytest.fixture(scope="module")
def small_scenes():
    return np.stack([synthetic_scene(4, H=64, W=80), synthetic_scene(5, H=64, W=80),
                     synthetic_scene(6, H=64, W=80, coarse=3)])


@pytest.fixture(scope="module")
def yard(dev, scenes, small_scenes):
    """The host-logic path frame by frame, computed once."""
    return {id(fr): [tuple(r[0] for r in dev.detect_face(f[None])) for f in fr] for fr in (scenes, small_scenes)}


@pytest.mark.parametrize("which", ["small", "scenes"])
def test_detect_batch_equals_detect_face_per_frame(dev, scenes, small_scenes, yard, which):
    frames = small_scenes if which == "small" else scenes
    ref = yard[id(frames)]
    FD.STATS = {}
    try:
        gb, gp = dev.detect_batch(frames)
        stats = dict(FD.STATS)
    finally:
        FD.STATS = None
    torch.cuda.synchronize()
    print(which, "faces per frame:", [len(r[0]) for r in ref], stats)
    assert stats.get("device_fallback_n", 0) == 0 and stats["readback_n"] == 4
    assert len(gb) == len(gp) == len(frames)
    for b, (rb, rp) in enumerate(ref):
        assert len(rb) > 10, "the comparison must not be vacuous"
        assert gb[b].dtype == rb.dtype and gp[b].dtype == rp.dtype and gp[b].shape == rp.shape
        assert np.array_equal(gb[b], rb) and np.array_equal(gp[b], rp), b
        ob, op = dev.detect_batch(frames[b:b + 1])  # the same at B = 1
        assert np.array_equal(ob[0], rb) and np.array_equal(op[0], rp), b
    tb, tp = dev.detect_batch(torch.as_tensor(frames).cuda())  # device input
    assert all(np.array_equal(a, b) for a, b in zip(tb, gb)) and all(np.array_equal(a, b) for a, b in zip(tp, gp))


@pytest.mark.parametrize("th", [(1.1, .7, .7), (.6, 1.1, .7), (.6, .7, 1.1)], ids=["P", "R", "O"])
def test_detect_batch_empty_stages(gpu, small_scenes, th):
    d = FD.DeviceMTCNN(FD.synth_mtcnn_state(7), device=0, thresholds=th)
    boxes, points = d.detect_batch(small_scenes)
    torch.cuda.synchronize()
    assert len(boxes) == len(points) == len(small_scenes)
    for bb, pp in zip(boxes, points):
        assert bb.shape == (0, 5) and pp.shape == (0, 5, 2) and bb.dtype == pp.dtype == f32
    hb, hp = d.detect_face(small_scenes[:1])  # the host path agrees that nothing is left
    assert hb[0].shape == (0, 5) and hp[0].shape == (0, 5, 2)


def test_detect_batch_capacity_fallback(gpu, dev, small_scenes, yard):
    d = FD.DeviceMTCNN(FD.synth_mtcnn_state(7), device=0, capacity=8)
    FD.STATS = {}
    try:
        gb, gp = d.detect_batch(small_scenes)
        stats = dict(FD.STATS)
    finally:
        FD.STATS = None
    assert stats["device_fallback_n"] == 1
    for b, (rb, rp) in enumerate(yard[id(small_scenes)]):
        assert np.array_equal(gb[b], rb) and np.array_equal(gp[b], rp), b


@pytest.fixture(scope="module")
def fdet(gpu):
    return FD.FaceDetector(mtcnn_state=FD.synth_mtcnn_state(7))


def test_face_detector_detect_batch(fdet, scenes):
    bgr = np.ascontiguousarray(scenes[..., ::-1])
    got = fdet.detect_batch(bgr)
    ref = [fdet.detect(f) for f in bgr]
    assert any(r is not None for r in ref)
    assert got == ref
    assert fdet.detect_batch(list(bgr)) == ref


def test_recognize_frames_equals_recognize(fdet, scenes):
    from facerecognition_amd.model import FRModel
    from facerecognition_amd.recognition_engine import RecognitionEngine
    model = FRModel.synthetic("resnet50_arcface")
    eng = RecognitionEngine(model_path=None, model=model, use_face_detection=True, face_detector=fdet,
                            batch_invariant=True)
    frames = np.ascontiguousarray(scenes[..., ::-1])
    rng = np.random.default_rng(2)
    db = {f"id{n:02d}": v / np.linalg.norm(v) for n, v in enumerate(rng.standard_normal((24, 512)).astype(f32))}
    db["scene0"] = eng.extract_embedding(frames[0])
    eng.db = db
    ref = [eng.recognize(f) for f in frames]
    got = eng.recognize_frames(frames)
    assert ref[0]["status"] == "success" and ref[0]["identity"] == "scene0"
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert g["status"] == r["status"] and g["identity"] == r["identity"]
        assert abs(g["confidence"] - r["confidence"]) <= 1e-6
        assert [n for n, _ in g["top_k"]] == [n for n, _ in r["top_k"]]
        assert np.allclose([s for _, s in g["top_k"]], [s for _, s in r["top_k"]], rtol=0, atol=1e-6)
        if r["embedding"] is None:
            assert g["embedding"] is None
        else:
            assert np.allclose(g["embedding"], r["embedding"], rtol=0, atol=1e-6)
    # a frame without a face takes recognize()'s path for it
    none = FD.FaceDetector(mtcnn_state=FD.synth_mtcnn_state(7), confidence_threshold=1.1)
    eng2 = RecognitionEngine(model_path=None, model=model, use_face_detection=True, face_detector=none)
    eng2.db = db
    a, b = eng2.recognize_frames(frames[:2]), [eng2.recognize(f) for f in frames[:2]]
    assert [(x["status"], x.get("message"), x["identity"]) for x in a] == \
           [(x["status"], x.get("message"), x["identity"]) for x in b]
    assert a[0]["status"] == "error"
