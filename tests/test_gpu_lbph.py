"""LBPH on the device against the numpy restatement of OpenCV's algorithm (tests/lbph_ref.py; not compared with a
cv2.face build): fr_lbph_hist counts integer-equal, fr_lbph_match distances within the float32-rounding bound and
indices equal wherever the reference is unambiguous, the recognizer's cv2 surface, and the database builder.

Distance bound, per distance d_ref (float64 chi-square on the reference's float32 histograms):
    |d - d_ref| <= 2^-21 * (d_ref + sqrt(cells * d_ref))
float32 rounding of count / P in the reference moves d by at most 2^-22 * sqrt(cells * d) (Cauchy-Schwarz over the
bins), one rounded float32 division per term on the device by at most 2^-24 * d; the test allows twice their sum.
An index is compared wherever the reference's gap to the next distinct distance exceeds twice that bound, and the
tests assert that this holds for every (probe, rank) of their inputs."""
import os

import numpy as np
import pytest

from tests import lbph_ref as R

pytestmark = pytest.mark.gpu


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


def _counts_dev(c, gpu):
    return _dev(np.asarray(c).astype(np.uint16).view(np.int16), gpu)


# ------------------------------------------------------------------------------------------------------ counts
#            H    W   r  n  gx gy
HIST_CASES = [(100, 100, 1, 8, 8, 8),
              (37, 53, 1, 8, 3, 5),    # odd width: band starts at every byte phase
              (37, 53, 1, 8, 5, 3),    # remainder row and columns ignored
              (24, 24, 2, 6, 2, 2),
              (21, 21, 4, 8, 1, 1),
              (140, 512, 1, 8, 2, 1)]  # a 138-row band: three LDS tiles per workgroup


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("H,W,r,n,gx,gy", HIST_CASES)
def test_counts_equal_the_reference(gpu, H, W, r, n, gx, gy, B):
    from facerecognition_amd.lbph import lbph_hist
    # noise, blurred noise (both with flat patches), checkerboard, ramp, noise
    imgs = R.make_images(5, H, W, seed=H + W)
    if B == 1:
        imgs = imgs[1:2]
    ref = np.stack([R.counts(im, r, n, gx, gy) for im in imgs])
    got = _u16(lbph_hist(_dev(imgs, gpu), r, n, gx, gy)).astype(np.int64)
    assert got.shape == ref.shape
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, (f"{len(bad)} bins differ, first (image, bin) {bad[0]}: "
                           f"{got[tuple(bad[0])]} vs {ref[tuple(bad[0])]}")
    cw, ch = R.cell_shape(H, W, r, gx, gy)
    assert np.all(got.reshape(B, gx * gy, 1 << n).sum(2) == cw * ch)


def test_flat_patch_codes_on_the_device(gpu):
    from facerecognition_amd.lbph import lbph_hist
    vals = (0, 1, 3, 100, 200, 255)
    imgs = np.stack([np.full((10, 10), v, np.uint8) for v in vals])
    got = _u16(lbph_hist(_dev(imgs, gpu), 1, 8, 1, 1))
    for v, row in zip(vals, got):
        code = 247 if v == 3 else 255
        assert row[code] == 64 and row.sum() == 64, (v, np.nonzero(row))


# ------------------------------------------------------------------------------------------------------- match
def _tol(d, cells):
    return 2.0 ** -21 * (d + np.sqrt(cells * d))


def _check_match(dist, idx, dref, cells, k):
    """Distances within the bound at every rank; indices equal where the reference is unambiguous.  Returns the
    number of (probe, rank) pairs whose index was not compared."""
    B, n = dref.shape
    order = np.argsort(dref, axis=1, kind="stable")
    excluded = 0
    for b in range(B):
        s = dref[b, order[b]]
        for j in range(k):
            if j >= n:
                assert np.isposinf(dist[b, j]) and idx[b, j] == -1, (b, j, dist[b, j], idx[b, j])
                continue
            tol = _tol(s[j], cells)
            print(f"probe {b} rank {j}: d {float(dist[b, j])!r} ref {float(s[j])!r} err {abs(dist[b, j] - s[j]):.3e} tol {tol:.3e}")
            assert abs(dist[b, j] - s[j]) <= tol, (b, j, dist[b, j], s[j], tol)
            nxt = s[s > s[j]]
            if len(nxt) and nxt[0] - s[j] <= 2 * tol:
                excluded += 1
            else:
                assert idx[b, j] == order[b, j], (b, j, idx[b, j], order[b, j])
        assert np.all(np.diff(dist[b, :min(k, n)]) >= 0)
    return excluded


@pytest.fixture(scope="module")
def match_set():
    """300 gallery and 17 probe count rows of blurred-noise 100x100 images (defaults: D = 16384, P = 144), and the
    reference's float64 distances on their float32 histograms."""
    rng = np.random.default_rng(0)
    imgs = np.stack([R.blurred_noise(rng, 100, 100, passes=1 + i % 3) for i in range(317)])
    c = np.stack([R.counts(im) for im in imgs])
    h = R.hist_from_counts(c, 144)
    dref = R.distances(h[300:], h[:300])
    dref.setflags(write=False)
    c.setflags(write=False)
    return c[:300], c[300:], dref


@pytest.mark.parametrize("k", [1, 5, 32])
@pytest.mark.parametrize("B", [1, 17])
@pytest.mark.parametrize("n", [1, 7, 300])
def test_match_against_the_reference(gpu, match_set, n, B, k):
    from facerecognition_amd.lbph import lbph_match
    g, q, dref = match_set
    dist, idx = lbph_match(_counts_dev(q[:B], gpu), _counts_dev(g[:n], gpu), 144, k)
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    assert dist.shape == (B, k) and dist.dtype == np.float64 and idx.dtype == np.int32
    assert _check_match(dist, idx, dref[:B, :n], 64, k) == 0  # no (probe, rank) of this set is ambiguous


@pytest.mark.parametrize("r,nb,gx,gy", [(1, 2, 3, 3),    # D = 36: rows not 16-byte multiples (scalar loads)
                                        (2, 6, 2, 2),    # D = 256: less than one 512-element pass
                                        (1, 7, 3, 2)])   # D = 768: one and a half passes
def test_match_other_row_lengths(gpu, r, nb, gx, gy):
    from facerecognition_amd.lbph import lbph_match
    rng = np.random.default_rng(7)
    imgs = np.stack([R.blurred_noise(rng, 40, 40, passes=1 + i % 2) for i in range(24)])
    c = np.stack([R.counts(im, r, nb, gx, gy) for im in imgs])
    cw, ch = R.cell_shape(40, 40, r, gx, gy)
    h = R.hist_from_counts(c, cw * ch)
    dref = R.distances(h[20:], h[:20])
    dist, idx = lbph_match(_counts_dev(c[20:], gpu), _counts_dev(c[:20], gpu), cw * ch, 5)
    assert _check_match(dist.cpu().numpy(), idx.cpu().numpy(), dref, gx * gy, 5) == 0


def _device_formula(q, g, P):
    """fr_lbph_match's documented arithmetic for one (probe, row) pair with IEEE float32 division: terms
    RN(RN(delta^2) / s) in float32, lane l of 64 adds its elements (8 consecutive bins every 512) in ascending
    order in float64, the lanes fold by xor-butterfly 32, 16, .. 1, and the sum is scaled by 2 / P."""
    pad = (-len(q)) % 512
    a = np.pad(q.astype(np.float32), (0, pad))
    b = np.pad(g.astype(np.float32), (0, pad))
    dl, sm = a - b, a + b
    term = np.where(sm > 0, (dl * dl) / np.where(sm > 0, sm, np.float32(1)), np.float32(0))
    assert term.dtype == np.float32
    t = term.astype(np.float64).reshape(-1, 64, 8)
    lane = np.zeros(64)
    for c in range(t.shape[0]):
        for e in range(8):
            lane = lane + t[c, :, e]
    for m in (32, 16, 8, 4, 2, 1):
        lane = lane + lane[np.arange(64) ^ m]
    return lane[0] * (2.0 / P)


def test_match_is_bitwise_the_documented_formula(gpu, match_set):
    """The device's division is its own expansion (no range scaling): its distances equal, bit for bit, the same
    sum with IEEE float32 division on the host, for full passes (D = 16384), a partial pass (768) and the scalar
    loads (36); one large-count pair (P = 65025, delta^2 past 2^24) too."""
    from facerecognition_amd.lbph import lbph_match
    g, q, _ = match_set
    sets = [(q[:5], g[:7], 144)]
    rng = np.random.default_rng(3)
    for D, P in ((768, 50), (36, 9), (1024, 65025)):
        used = 8 if P > 60000 else D // 4  # sparse rows summing to P; the large-P rows hold counts past 4096
        c = rng.multinomial(P, rng.dirichlet(np.full(used, 0.3)), size=9)
        c = np.concatenate([c, np.zeros((9, D - used), np.int64)], axis=1)
        c = np.stack([np.roll(row, 3 * i) for i, row in enumerate(c)])
        sets.append((c[:3], c[3:], P))
    for qs, gs, P in sets:
        n = len(gs)
        dist, idx = lbph_match(_counts_dev(qs, gpu), _counts_dev(gs, gpu), P, n)
        dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
        for b in range(len(qs)):
            for j in range(n):
                want = _device_formula(qs[b], gs[idx[b, j]], P)
                assert dist[b, j] == want, (len(qs[b]), P, b, j, dist[b, j], want)


def test_match_exact_zero_ties_and_batch_invariance(gpu, match_set):
    from facerecognition_amd.lbph import lbph_match
    g, q, _ = match_set
    g = g.copy()
    g[250] = g[3]                       # identical rows in different workgroups of the split
    g[9] = g[8]                         # and side by side in one wave's tile
    probes = np.concatenate([g[3:4], g[8:9], g[100:101], q[:14]])  # 17 probes; three are gallery rows
    G = _counts_dev(g, gpu)
    dist, idx = lbph_match(_counts_dev(probes, gpu), G, 144, 32)
    dist, idx = dist.cpu().numpy(), idx.cpu().numpy()
    # a probe that is a gallery row: exactly 0.0 at that row; equal distances keep the lower index first
    assert dist[0, 0] == 0.0 and dist[0, 1] == 0.0 and idx[0, :2].tolist() == [3, 250]
    assert dist[1, 0] == 0.0 and dist[1, 1] == 0.0 and idx[1, :2].tolist() == [8, 9]
    assert dist[2, 0] == 0.0 and idx[2, 0] == 100 and dist[2, 1] > 0.0
    # k = N = 300 is out of range, so find the twin rows through a 7-row gallery holding both
    small = np.concatenate([g[0:3], g[3:4], g[4:6], g[250:251]])
    d7, i7 = lbph_match(_counts_dev(q[:5], gpu), _counts_dev(small, gpu), 144, 7)
    d7, i7 = d7.cpu().numpy(), i7.cpu().numpy()
    for b in range(5):
        a, z = int(np.where(i7[b] == 3)[0][0]), int(np.where(i7[b] == 6)[0][0])
        assert z == a + 1 and d7[b, a] == d7[b, z], (b, i7[b], d7[b])
    # every probe alone gives bitwise its row of the batch (one probe per wave tile in place of four)
    for b in (0, 2, 5, 16):
        d1, i1 = lbph_match(_counts_dev(probes[b:b + 1], gpu), G, 144, 32)
        assert np.array_equal(d1.cpu().numpy().view(np.int64)[0], dist.view(np.int64)[b]), b
        assert np.array_equal(i1.cpu().numpy()[0], idx[b]), b


# -------------------------------------------------------------------------------------------------- recognizer
@pytest.fixture(scope="module")
def faces():
    """48 training images with 12 labels and 16 probes (perturbed training images), blurred noise 100x100; the
    reference's histograms, distances and predictions."""
    rng = np.random.default_rng(0)
    train = np.stack([R.blurred_noise(rng, 100, 100, passes=1 + i % 3) for i in range(48)])
    labels = (np.arange(48) % 12).astype(np.int32) + 100
    probes = []
    for i in range(16):
        im = train[3 * i].astype(np.int16) + rng.integers(-6, 7, (100, 100))
        probes.append(np.clip(im, 0, 255).astype(np.uint8))
    probes = np.stack(probes)
    hg = np.stack([R.histogram(im) for im in train])
    hq = np.stack([R.histogram(im) for im in probes])
    dref = R.distances(hq, hg)
    pred = [R.predict(row, labels) for row in dref]
    for a in (train, labels, probes, dref):
        a.setflags(write=False)
    return train, labels, probes, dref, np.array([p[0] for p in pred]), np.array([p[1] for p in pred])


def test_recognizer_predicts_as_the_reference(gpu, faces):
    import facerecognition_amd as fa
    train, labels, probes, dref, ref_l, ref_d = faces
    m = fa.LBPHFaceRecognizer_create()
    assert (m.getRadius(), m.getNeighbors(), m.getGridX(), m.getGridY(), m.getThreshold()) == (1, 8, 8, 8, R.DBL_MAX)
    m.train(list(train), labels)
    assert np.array_equal(m.getLabels(), labels)
    h = m.getHistograms()
    assert h.dtype == np.float32 and np.array_equal(h, np.stack([R.histogram(im) for im in train]))
    s = np.sort(dref, axis=1)
    assert np.all(s[:, 1] - s[:, 0] > 2 * _tol(s[:, 0], 64))  # the nearest row is unambiguous for every probe
    got_l, got_d = m.predict_batch(list(probes))
    assert np.array_equal(got_l, ref_l)
    assert np.all(np.abs(got_d - ref_d) <= _tol(ref_d, 64)), (got_d, ref_d)
    for i in (0, 7, 15):
        l, d = m.predict(probes[i])
        assert isinstance(l, int) and isinstance(d, float) and (l, d) == (int(got_l[i]), float(got_d[i]))
    with pytest.raises(ValueError):
        m.predict(probes[0][:, :90])
    with pytest.raises(ValueError):
        m.train([train[0], train[1][:50]], [1, 2])
    r = fa.recognize_face(m, probes[0], got_d[0] + 1.0)
    assert r == {"label": int(got_l[0]), "confidence": float(got_d[0]), "status": "known"}
    r = fa.recognize_face(m, probes[0], got_d[0])
    assert r["label"] is None and r["status"] == "unknown" and r["confidence"] == float(got_d[0])


def test_recognizer_threshold_is_strict(gpu, faces):
    import facerecognition_amd as fa
    train, labels, probes, _, _, _ = faces
    m = fa.train_lbph_model(list(train), labels)
    base_l, base_d = m.predict_batch(list(probes))
    i = int(np.argsort(base_d)[8])  # a probe in the middle: some distances below it, some above
    m.setThreshold(float(base_d[i]) * 0.999)
    assert m.getThreshold() == float(base_d[i]) * 0.999 and m.predict(probes[i]) == (-1, R.DBL_MAX)
    m.setThreshold(float(base_d[i]))  # equal: still rejected, the comparison is d < threshold
    l, d = m.predict_batch(list(probes))
    assert (l[i], d[i]) == (-1, R.DBL_MAX)
    below = base_d < base_d[i]
    assert below.sum() == 8 and np.array_equal(l[below], base_l[below]) and np.array_equal(d[below], base_d[below])
    assert np.all(l[~below] == -1) and np.all(d[~below] == R.DBL_MAX)
    m.setThreshold(float(np.nextafter(base_d[i], np.inf)))
    assert m.predict(probes[i]) == (int(base_l[i]), float(base_d[i]))


def test_recognizer_update_and_save_load(gpu, faces, tmp_path):
    import facerecognition_amd as fa
    train, labels, probes, _, _, _ = faces
    full = fa.train_lbph_model(list(train), labels, radius=1, neighbors=8, grid_x=8, grid_y=8)
    want = full.predict_batch(list(probes))
    part = fa.train_lbph_model(list(train[:30]), labels[:30])
    part.update(list(train[30:]), labels[30:])
    got = part.predict_batch(list(probes))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.int64), want[1].view(np.int64))
    assert np.array_equal(part.getLabels(), labels) and np.array_equal(part.getHistograms(), full.getHistograms())
    with pytest.raises(ValueError):
        part.update([train[0][:60, :60]], [1])
    full.setThreshold(90.5)
    path = str(tmp_path / "model.npz")
    full.save(path)
    with np.load(path) as z:
        assert z["counts"].dtype == np.uint16 and z["counts"].shape == (48, 16384)
        assert np.array_equal(z["labels"], labels)
    back = fa.LBPHFaceRecognizer.load(path)
    assert (back.getRadius(), back.getNeighbors(), back.getGridX(), back.getGridY(), back.getThreshold()) == \
        (1, 8, 8, 8, 90.5)
    a, b = full.predict_batch(list(probes)), back.predict_batch(list(probes))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int64), b[1].view(np.int64))


def test_find_optimal_threshold_equals_the_reference_formula(gpu, faces):
    import facerecognition_amd as fa
    train, labels, probes, dref, ref_l, ref_d = faces
    m = fa.train_lbph_model(list(train), labels)
    val_labels = labels[3 * np.arange(16)].copy()
    val_labels[::5] += 1  # some wrong on purpose: accuracy below 1
    rng = range(40, 121, 5)
    # no reference confidence sits within the distance bound of a swept threshold
    assert all(np.all(np.abs(ref_d - t) > _tol(ref_d, 64)) for t in rng)
    got = fa.find_optimal_threshold(m, list(probes), val_labels)
    want = R.find_optimal_threshold(ref_l, ref_d, val_labels)
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2] and len(got[2]) > 0
    got = fa.find_optimal_threshold(m, list(probes), val_labels, min_coverage=0.5, threshold_range=range(1, 4))
    assert got == (3, 0.0, []) and got == R.find_optimal_threshold(ref_l, ref_d, val_labels, 0.5, range(1, 4))


# ----------------------------------------------------------------------------------------------------- builder
def test_database_builder_lbph(gpu, tmp_path):
    from PIL import Image

    from facerecognition_amd import database_builder as DB
    from facerecognition_amd import lbph
    rng = np.random.default_rng(11)
    data = tmp_path / "data"
    for ident in ("10", "2", "bob"):
        os.makedirs(data / ident)
        for j in range(3):
            size = (120, 90) if (ident, j) == ("bob", 2) else (100, 100)  # one image goes through the resize
            g = R.blurred_noise(rng, size[1], size[0], passes=1 + j)
            rgb = np.stack([g, np.roll(g, 3, 0), np.roll(g, 5, 1)], axis=2)
            Image.fromarray(rgb).save(data / ident / f"img{j}.png")
    out = tmp_path / "out"
    b = DB.DatabaseBuilder()
    b.create_job("j", "lbph", {"data_dir": str(data), "output_dir": str(out), "use_face_detection": False})
    b.start_build("j").join(120)
    job = b.get_job("j")
    assert job.status == "completed", job.to_dict()
    model_path = str(out / "lbph_model.npz")  # the reference's default lbph_model.xml with the extension replaced
    assert job.output_files == {"LBPH Model": model_path}
    assert any("lbph_model.xml -> lbph_model.npz" in line for line in job.logs)
    assert any("Đang train LBPH từ" in line for line in job.logs) and job.progress == 100.0
    assert os.path.isfile(model_path) and os.path.isfile(out / "label_map.npy")
    assert not os.path.exists(out / "optimal_threshold.txt")
    label_map = np.load(out / "label_map.npy", allow_pickle=True).item()
    assert label_map == {0: "10", 1: "2", 2: "bob"}  # the reference's key: digit names first, compared as strings
    model = lbph.LBPHFaceRecognizer.load(model_path)
    faces, labels = lbph.load_faces_and_labels(str(data), label_map, use_face_detection=False)
    assert len(faces) == 9 and all(f.shape == (100, 100) and f.dtype == np.uint8 for f in faces)
    got_l, got_d = model.predict_batch(faces)
    assert np.array_equal(got_l, labels) and np.all(got_d == 0.0)
    # with a validation tree the threshold sweep is written in the reference's layout
    b.create_job("t", "lbph", {"data_dir": str(data), "output_dir": str(out), "model_name": "m.npz",
                               "use_face_detection": False, "find_threshold": True, "val_dir": str(data)})
    b.start_build("t").join(120)
    assert b.get_job("t").status == "completed", b.get_job("t").to_dict()
    text = open(out / "optimal_threshold.txt").read().splitlines()
    assert text[0].startswith("Optimal threshold: ") and text[1].startswith("Score (accuracy * coverage): 1.0000")
    assert text[4] == "Threshold | Accuracy | Coverage | Score" and text[5] == "-" * 50
    assert text[6].split("|")[0].strip() == "40" and len(text) == 6 + 17
