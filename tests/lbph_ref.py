"""numpy restatement of OpenCV's LBPHFaceRecognizer (opencv_contrib face/lbph_faces.cpp), the yardstick of the
LBPH tests: extended LBP in float32 in OpenCV's operation order, spatial histograms as float32 count / P,
HISTCMP_CHISQR_ALT in float64, nearest-neighbour predict.  ``cv2`` is not available where these tests were
written: this restatement has NOT been compared with a real cv2.face build.  A test helper only; the package has
no CPU compute path."""
import math
import sys

import numpy as np

DBL_MAX = sys.float_info.max
FLT_EPSILON = np.float32(np.finfo(np.float32).eps)
DBL_EPSILON = float(np.finfo(np.float64).eps)


def table(radius=1, neighbors=8):
    """(offs int32 [n][4] = fx, fy, cx, cy; w float32 [n][4] = w1..w4): x, y from a double product cast to float,
    the weights in float32 (libm cos / sin, as the C++ code)."""
    offs = np.zeros((neighbors, 4), np.int32)
    w = np.zeros((neighbors, 4), np.float32)
    one = np.float32(1)
    for n in range(neighbors):
        x = np.float32(radius * math.cos(2.0 * math.pi * n / float(neighbors)))
        y = np.float32(-radius * math.sin(2.0 * math.pi * n / float(neighbors)))
        fx, fy, cx, cy = int(math.floor(x)), int(math.floor(y)), int(math.ceil(x)), int(math.ceil(y))
        ty, tx = np.float32(y - np.float32(fy)), np.float32(x - np.float32(fx))
        offs[n] = (fx, fy, cx, cy)
        w[n] = ((one - tx) * (one - ty), tx * (one - ty), (one - tx) * ty, tx * ty)
    return offs, w


def elbp(img, radius=1, neighbors=8):
    """Codes [H - 2r][W - 2r] (int32) of a gray u8 image."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    H, W = img.shape
    r = radius
    offs, w = table(radius, neighbors)
    src = img.astype(np.float32)
    ctr = src[r:H - r, r:W - r]
    code = np.zeros(ctr.shape, np.int32)

    def sh(dy, dx):
        return src[r + dy:H - r + dy, r + dx:W - r + dx]

    for n in range(neighbors):
        fx, fy, cx, cy = (int(v) for v in offs[n])
        t = w[n, 0] * sh(fy, fx)  # float32 arrays: every product and sum rounds to float32, left to right
        t = t + w[n, 1] * sh(fy, cx)
        t = t + w[n, 2] * sh(cy, fx)
        t = t + w[n, 3] * sh(cy, cx)
        assert t.dtype == np.float32
        bit = (t > ctr) | (np.abs(t - ctr) < FLT_EPSILON)
        code |= bit.astype(np.int32) << n
    return code


def cell_shape(H, W, radius, grid_x, grid_y):
    return (W - 2 * radius) // grid_x, (H - 2 * radius) // grid_y  # cw, ch


def counts(img, radius=1, neighbors=8, grid_x=8, grid_y=8):
    """Integer cell counts [grid_y * grid_x * 2^neighbors], cells row-major; remainder pixels ignored."""
    code = elbp(img, radius, neighbors)
    nb = 1 << neighbors
    cw, ch = cell_shape(img.shape[0], img.shape[1], radius, grid_x, grid_y)
    out = np.zeros((grid_y * grid_x, nb), np.int64)
    for i in range(grid_y):
        for j in range(grid_x):
            cell = code[i * ch:(i + 1) * ch, j * cw:(j + 1) * cw]
            out[i * grid_x + j] = np.bincount(cell.ravel(), minlength=nb)
    return out.ravel()


def hist_from_counts(c, P):
    """OpenCV's float32 histogram: count / (float)P in float32."""
    return (np.asarray(c).astype(np.float32) / np.float32(P)).astype(np.float32)


def histogram(img, radius=1, neighbors=8, grid_x=8, grid_y=8):
    cw, ch = cell_shape(img.shape[0], img.shape[1], radius, grid_x, grid_y)
    return hist_from_counts(counts(img, radius, neighbors, grid_x, grid_y), cw * ch)


def chisqr_alt(a, b):
    """HISTCMP_CHISQR_ALT on float32 histograms, accumulated in float64."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    s = a + b
    d = a - b
    m = np.abs(s) > DBL_EPSILON
    return 2.0 * float(np.sum(d[m] * d[m] / s[m]))


def distances(probes, gallery):
    """[B][N] float64 chi-square distances between float32 histogram rows."""
    P = np.asarray(probes, np.float32).astype(np.float64)
    G = np.asarray(gallery, np.float32).astype(np.float64)
    out = np.empty((len(P), len(G)))
    for i, a in enumerate(P):
        s = a[None] + G
        d = a[None] - G
        m = np.abs(s) > DBL_EPSILON
        out[i] = 2.0 * np.where(m, d * d / np.where(m, s, 1.0), 0.0).sum(1)
    return out


def predict(dist_row, labels, threshold=DBL_MAX):
    """OpenCV's predict over one probe's distances: first minimum wins, accepted only when d < threshold."""
    best_d, best_l = DBL_MAX, -1
    for d, l in zip(dist_row, labels):
        if d < best_d and d < threshold:
            best_d, best_l = float(d), int(l)
    return best_l, best_d


def find_optimal_threshold(predictions, confidences, labels, min_coverage=0.3, threshold_range=None):
    """The reference's accuracy x coverage sweep (threshold_lbph.py) over already computed predictions."""
    if threshold_range is None:
        threshold_range = range(40, 121, 5)
    predictions, confidences, labels = np.asarray(predictions), np.asarray(confidences), np.asarray(labels)
    best_threshold, best_score, results = None, -1, []
    for thr in threshold_range:
        acc_mask = confidences < thr
        used = np.sum(acc_mask)
        accuracy = np.sum(predictions[acc_mask] == labels[acc_mask]) / used if used > 0 else 0.0
        coverage = used / len(labels) if len(labels) > 0 else 0.0
        if coverage >= min_coverage:
            score = accuracy * coverage
            results.append((thr, accuracy, coverage, score))
            if score > best_score:
                best_score, best_threshold = score, thr
    if best_threshold is None:
        best_threshold, best_score = max(threshold_range), 0.0
    return best_threshold, best_score, results


# ------------------------------------------------------------------------------------------------ test images
def blurred_noise(rng, H, W, passes=3):
    """Smooth u8 texture: uniform noise box-blurred a few times and stretched to the full range."""
    x = rng.random((H + 2 * passes, W + 2 * passes))
    for _ in range(passes):
        x = (x[:-2, :-2] + x[:-2, 1:-1] + x[:-2, 2:] + x[1:-1, :-2] + x[1:-1, 1:-1] + x[1:-1, 2:] + x[2:, :-2] +
             x[2:, 1:-1] + x[2:, 2:]) / 9.0
    x = (x - x.min()) / (x.max() - x.min())
    return np.round(x * 255).astype(np.uint8)


def make_images(B, H, W, seed=0):
    """B images that exercise the code rule: uniform noise and blurred noise carrying flat patches of 0, 1, 3, 200
    and 255 across cell borders, then a checkerboard and a horizontal ramp."""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        kind = b % 4
        if kind == 0:
            im = rng.integers(0, 256, (H, W), dtype=np.uint8)
        elif kind == 1:
            im = blurred_noise(rng, H, W)
        elif kind == 2:
            yy, xx = np.mgrid[0:H, 0:W]
            im = (((yy // 3 + xx // 2) % 2) * 255).astype(np.uint8)
        else:
            im = np.broadcast_to(np.linspace(0, 255, W).astype(np.uint8), (H, W)).copy()
        if kind < 2:  # flat patches at spread positions; sizes that straddle cells of every grid used
            ph, pw = max(3, H // 4), max(3, W // 4)
            for n, v in enumerate((0, 1, 3, 200, 255)):
                y0 = (n * (H - ph)) // 4
                x0 = ((4 - n) * (W - pw)) // 4 if b % 8 < 4 else (n * (W - pw)) // 4
                im[y0:y0 + ph, x0:x0 + pw] = v
        out.append(im)
    return np.stack(out)
