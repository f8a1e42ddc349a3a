"""fr_match_range_* and fr_gallery_read at the C-ABI boundary, without a GPU: exported, bound, and bad
arguments rejected with FR_ERR_ARG and a message naming the entry point (no compute)."""
import ctypes

from facerecognition_amd import _native as N

NEW = {"fr_match_range_workspace": 2, "fr_match_range_count": 8, "fr_match_range_fill": 11, "fr_gallery_read": 5,
       "fr_debug_match_range_splits": 2}


def test_range_functions_are_exported_and_bound():
    L = N.lib()
    for name, nargs in NEW.items():
        assert name in N.header_functions(), name
        assert hasattr(L, name) and name in N._SIGS, name
        assert len(N._SIGS[name][1]) == nargs, name
    assert N._SIGS["fr_match_range_workspace"][0] is ctypes.c_size_t
    assert L.fr_abi_version() == 1  # additive change


def _other_message(L):
    L.fr_op_avgpool(None, 1, 1, 1, 8, None, 0, None)  # leaves another entry point's message behind


def test_range_count_rejects_bad_arguments():
    L = N.lib()
    buf = (ctypes.c_uint64 * 64)()  # host memory: never dereferenced on these paths
    p = ctypes.addressof(buf)

    def call(P=p, B=4, thresh=0.5, after=None, ws=p, lims=p, h=None):
        _other_message(L)
        return L.fr_match_range_count(h, P, B, thresh, after, ws, lims, None), L.fr_last_error()

    for kw in (dict(P=None), dict(ws=None), dict(lims=None), dict(B=0), dict(B=-3), dict(thresh=float("nan")),
               dict(after=p, thresh=float("nan")),
               dict(), dict(after=p), dict(thresh=float("-inf"))):  # everything valid but the handle
        rc, msg = call(**kw)
        assert rc == -1 and b"fr_match_range_count" in msg, (kw, rc, msg)


def test_range_fill_rejects_bad_arguments():
    L = N.lib()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)

    def call(P=p, B=4, thresh=0.5, after=None, ws=p, lims=p, s=p, i=p, cap=16, h=None):
        _other_message(L)
        return L.fr_match_range_fill(h, P, B, thresh, after, ws, lims, s, i, cap, None), L.fr_last_error()

    for kw in (dict(P=None), dict(ws=None), dict(lims=None), dict(s=None), dict(i=None), dict(B=0), dict(B=-1),
               dict(thresh=float("nan")), dict(cap=-1), dict(cap=-2 ** 40),
               dict(), dict(cap=0), dict(after=p)):  # everything valid but the handle
        rc, msg = call(**kw)
        assert rc == -1 and b"fr_match_range_fill" in msg, (kw, rc, msg)


def test_gallery_read_workspace_and_splits_reject_bad_arguments():
    L = N.lib()
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    for args in ((None, 0, -1, p, 0), (None, -1, 1, p, 0), (None, 0, 1, None, 0), (None, 0, 1, None, 1),
                 (None, 0, 1, p, 0), (None, 2 ** 40, 2 ** 40, p, 0)):  # the last two: valid but the handle
        _other_message(L)
        rc = L.fr_gallery_read(*args)
        assert rc == -1 and b"fr_gallery_read" in L.fr_last_error(), args
    assert buf[0] == 0.0
    _other_message(L)
    assert L.fr_match_range_workspace(None, 4) == 0 and b"fr_match_range_workspace" in L.fr_last_error()
    assert L.fr_match_range_workspace(None, 0) == 0
    _other_message(L)
    assert L.fr_debug_match_range_splits(None, 4) == -1 and b"fr_debug_match_range_splits" in L.fr_last_error()
