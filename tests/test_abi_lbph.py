"""The fr_lbph_* entry points at the C-ABI boundary, without a GPU: declared, exported, bound, and every
unsupported argument refused with FR_ERR_ARG and a message before any HIP call (the pointers below are host
memory and are never dereferenced)."""
import ctypes

import pytest

from facerecognition_amd import _native as N

NEW = {"fr_lbph_table": 4, "fr_lbph_hist": 10, "fr_lbph_match_workspace": 4, "fr_lbph_match": 12}


def _p():
    buf = (ctypes.c_uint64 * 64)()
    return buf, ctypes.addressof(buf)


def _other_message(L):
    L.fr_op_avgpool(None, 1, 1, 1, 8, None, 0, None)  # leaves another entry point's message behind


def test_lbph_functions_are_declared_exported_and_bound():
    L = N.lib()
    for name, nargs in NEW.items():
        assert name in N.header_functions(), name
        assert hasattr(L, name) and name in N._SIGS, name
        assert len(N._SIGS[name][1]) == nargs, name
    assert N._SIGS["fr_lbph_match_workspace"][0] is ctypes.c_size_t
    assert L.fr_abi_version() == 1  # additive change


HIST_OK = dict(B=2, H=100, W=100, radius=1, neighbors=8, grid_x=8, grid_y=8)
HIST_BAD = [dict(radius=0), dict(radius=5), dict(neighbors=0), dict(neighbors=9), dict(grid_x=0), dict(grid_x=17),
            dict(grid_y=0), dict(grid_y=17), dict(H=513), dict(W=513), dict(H=0), dict(W=-4), dict(B=0), dict(B=-1),
            dict(H=2, W=2),                      # not larger than 2 * radius
            dict(W=9, grid_x=8),                 # cw = 7 // 8 = 0
            dict(H=12, radius=4, grid_y=5),      # ch = 4 // 5 = 0
            dict(H=512, W=512, grid_x=1, grid_y=1),  # P = 510 * 510 > 65535
            dict(img=None), dict(counts=None), dict(counts_off=2)]


@pytest.mark.parametrize("kw", HIST_BAD, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_hist_rejects_unsupported_arguments(kw):
    L = N.lib()
    _, p = _p()
    a = dict(HIST_OK, img=p, counts=p, counts_off=0)
    a.update(kw)
    counts = None if a["counts"] is None else a["counts"] + a["counts_off"]
    _other_message(L)
    rc = L.fr_lbph_hist(a["img"], a["B"], a["H"], a["W"], a["radius"], a["neighbors"], a["grid_x"], a["grid_y"],
                        counts, None)
    assert rc == -1 and b"fr_lbph_hist" in L.fr_last_error(), (kw, rc, L.fr_last_error())


MATCH_OK = dict(B=4, N=10, D=16384, P=144, k=5)
MATCH_BAD = [dict(k=33), dict(k=0), dict(B=0), dict(B=65536), dict(N=0), dict(N=2 ** 30 + 1), dict(N=2 ** 31),
             dict(D=0), dict(D=65537), dict(P=0), dict(P=65536), dict(Q=None), dict(G=None), dict(dist=None),
             dict(idx=None), dict(ws=None), dict(ws_bytes=8)]


@pytest.mark.parametrize("kw", MATCH_BAD, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_match_rejects_unsupported_arguments(kw):
    L = N.lib()
    _, p = _p()
    a = dict(MATCH_OK, Q=p, G=p, dist=p, idx=p, ws=p, ws_bytes=1 << 40)
    a.update(kw)
    _other_message(L)
    rc = L.fr_lbph_match(a["Q"], a["B"], a["G"], a["N"], a["D"], a["P"], a["k"], a["dist"], a["idx"], a["ws"],
                         a["ws_bytes"], None)
    assert rc == -1 and b"fr_lbph_match" in L.fr_last_error(), (kw, rc, L.fr_last_error())


def test_match_workspace():
    L = N.lib()
    for B, n, D, k in ((1, 1, 2, 1), (17, 300, 1024, 32), (256, 10000, 16384, 1)):
        nws = L.fr_lbph_match_workspace(B, n, D, k)
        assert nws > 0 and nws % 4 == 0
        assert nws >= B * k * 12  # at least one (distance, index) list per probe
    for args in ((4, 10, 16384, 33), (4, 10, 16384, 0), (0, 10, 16384, 1), (4, 0, 16384, 1), (4, 10, 0, 1)):
        _other_message(L)
        assert L.fr_lbph_match_workspace(*args) == 0 and b"fr_lbph_match_workspace" in L.fr_last_error(), args
