"""The numpy restatement of OpenCV's LBPH (tests/lbph_ref.py) against the facts the algorithm pins, and
fr_lbph_table (a host call) against its neighbour table, bit for bit.  No GPU."""
import ctypes

import numpy as np
import pytest

from facerecognition_amd import _native as N
from tests import lbph_ref as R


def test_neighbour_table_radius1_neighbors8():
    offs, w = R.table(1, 8)
    assert w.dtype == np.float32 and offs.dtype == np.int32
    # axis neighbours: one exact weight of 1 on the pixel itself (the others 0 up to sin(pi)'s 1e-16 residue)
    assert offs[0].tolist() == [1, 0, 1, 0] and w[0, 0] == 1.0 and np.all(np.abs(w[0, 1:]) == 0.0)
    assert offs[2].tolist()[:2] == [0, -1] and w[2, 0] == 1.0 and np.all(np.abs(w[2, 1:]) < 1e-16)
    assert offs[4].tolist() == [-1, -1, -1, 0] and w[4, 2] == 1.0 and np.all(w[4, [0, 1, 3]] == 0.0)
    assert offs[6].tolist() == [-1, 1, 0, 1] and w[6, 1] == 1.0 and np.all(w[6, [0, 2, 3]] == 0.0)
    # diagonal neighbours: the same three float32 values, in the slot the corner nearest the sample takes
    a, b, c = np.float32(0.20710678), np.float32(0.49999997), np.float32(0.08578645)
    assert w[1].tolist() == [a, b, c, a] and offs[1].tolist() == [0, -1, 1, 0]
    assert w[3].tolist() == [b, a, a, c] and offs[3].tolist() == [-1, -1, 0, 0]
    assert w[5].tolist() == [a, c, b, a] and offs[5].tolist() == [-1, 0, 0, 1]
    assert w[7].tolist() == [c, a, a, b] and offs[7].tolist() == [0, 0, 1, 1]


@pytest.mark.parametrize("value,code", [(0, 255), (1, 255), (3, 247), (100, 255), (200, 255), (255, 255)])
def test_flat_patch_codes(value, code):
    """The float32 rounding is part of the contract: a flat patch of 3 loses bit 3 (0.49999997 * 3 + ... < 3)."""
    got = R.elbp(np.full((7, 9), value, np.uint8), 1, 8)
    assert got.shape == (5, 7) and np.all(got == code)


@pytest.mark.parametrize("H,W,r,n,gx,gy", [(100, 100, 1, 8, 8, 8), (37, 53, 1, 8, 3, 5), (24, 24, 2, 6, 2, 2),
                                           (21, 21, 4, 8, 1, 1)])
def test_cell_counts_sum_to_P(H, W, r, n, gx, gy):
    img = R.make_images(2, H, W, seed=3)[1]
    cw, ch = R.cell_shape(H, W, r, gx, gy)
    c = R.counts(img, r, n, gx, gy).reshape(gx * gy, 1 << n)
    assert np.all(c.sum(1) == cw * ch)
    h = R.histogram(img, r, n, gx, gy)
    assert h.dtype == np.float32 and h.shape == (gx * gy * (1 << n),)
    assert np.array_equal(h, (c.ravel().astype(np.float32) / np.float32(cw * ch)))


def test_remainder_pixels_are_ignored():
    """37x53 (H x W) gives 35x51 codes.  With 5 cells across and 3 down the cells are 10 wide and 11 high, so code
    column 50 and code rows 33-34 belong to no cell (3 across and 5 down divides evenly: 17x7 cells)."""
    H, W = 37, 53
    assert R.cell_shape(H, W, 1, 3, 5) == (17, 7) and (3 * 17, 5 * 7) == (51, 35)
    gx, gy = 5, 3
    cw, ch = R.cell_shape(H, W, 1, gx, gy)
    assert (cw, ch) == (10, 11) and gx * cw == 50 and gy * ch == 33
    rng = np.random.default_rng(5)
    a = rng.integers(0, 256, (H, W), dtype=np.uint8)
    b = a.copy()
    b[H - 1, :] = 255 - b[H - 1, :]  # feeds code row 34 only
    b[:, W - 1] = 255 - b[:, W - 1]  # feeds code column 50 only
    code_a, code_b = R.elbp(a), R.elbp(b)
    assert np.array_equal(code_a[:33, :50], code_b[:33, :50]) and not np.array_equal(code_a, code_b)
    ca, cb = R.counts(a, 1, 8, gx, gy), R.counts(b, 1, 8, gx, gy)
    assert np.array_equal(ca, cb) and ca.sum() == gx * gy * cw * ch
    # cells are row-major, i * grid_x + j: cell (1, 2) counts code rows 11-21, columns 20-29
    cell = np.bincount(code_a[11:22, 20:30].ravel(), minlength=256)
    assert np.array_equal(ca.reshape(gy * gx, 256)[1 * gx + 2], cell)


def test_distance_to_itself_is_zero_and_predict_rules():
    imgs = R.make_images(4, 24, 24, seed=1)
    h = np.stack([R.histogram(im, 1, 8, 2, 2) for im in imgs])
    for a in h:
        assert R.chisqr_alt(a, a) == 0.0
    d = R.distances(h, h)
    assert np.all(np.diag(d) == 0.0) and np.allclose(d, d.T, rtol=1e-15)
    assert d[0, 1] == R.chisqr_alt(h[0], h[1])
    assert R.predict([3.0, 1.0, 1.0, 2.0], [7, 8, 9, 10]) == (8, 1.0)           # first of an exact tie
    assert R.predict([3.0, 1.0], [7, 8], threshold=1.0) == (-1, R.DBL_MAX)       # strict: d == threshold rejects
    assert R.predict([3.0, 1.0], [7, 8], threshold=1.5) == (8, 1.0)


@pytest.mark.parametrize("radius,neighbors", [(1, 8), (2, 6), (4, 8), (3, 5), (1, 1), (2, 7)])
def test_fr_lbph_table_equals_the_numpy_table_bitwise(radius, neighbors):
    L = N.lib()
    offs = np.full((neighbors, 4), 99, np.int32)
    w = np.full((neighbors, 4), 99, np.float32)
    assert L.fr_lbph_table(radius, neighbors, offs.ctypes.data, w.ctypes.data) == 0
    ro, rw = R.table(radius, neighbors)
    assert np.array_equal(offs, ro)
    assert np.array_equal(w.view(np.uint32), rw.view(np.uint32))
    assert np.all(np.abs(offs) <= radius)


def test_fr_lbph_table_rejects_bad_arguments():
    L = N.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    for args in ((0, 8, p, p), (5, 8, p, p), (1, 0, p, p), (1, 9, p, p), (1, 8, None, p), (1, 8, p, None)):
        assert L.fr_lbph_table(*args) == -1 and b"fr_lbph_table" in L.fr_last_error(), args
