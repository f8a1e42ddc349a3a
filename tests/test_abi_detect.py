"""The device NMS and MTCNN box-stage entry points at the C-ABI boundary, without a GPU: declared, exported, bound,
and every unsupported argument refused with FR_ERR_ARG and the entry point's own message before any HIP call (the
pointers below are host memory and are never dereferenced)."""
import ctypes

import pytest

from facerecognition_amd import _native as N

NEW = {"fr_nms_workspace": 2, "fr_nms": 12, "fr_mtcnn_compact_workspace": 1, "fr_mtcnn_candidates": 16,
       "fr_mtcnn_select": 15, "fr_mtcnn_crop_boxes": 19, "fr_mtcnn_final_boxes": 8}
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def p():
    buf = (ctypes.c_uint64 * 80)()
    a = ctypes.addressof(buf)
    a += (-a) % 16  # the box buffers are 16-byte aligned
    yield a
    del buf


def _other_message(L):
    L.fr_op_avgpool(None, 1, 1, 1, 8, None, 0, None)  # leaves another entry point's message behind


def _ids(kw):
    return ",".join(f"{k}={v}" for k, v in kw.items())


def test_detect_functions_are_declared_exported_and_bound():
    L = N.lib()
    for name, nargs in NEW.items():
        assert name in N.header_functions(), name
        assert hasattr(L, name) and name in N._SIGS, name
        assert len(N._SIGS[name][1]) == nargs, name
    assert N._SIGS["fr_nms_workspace"][0] is ctypes.c_size_t
    assert N._SIGS["fr_mtcnn_compact_workspace"][0] is ctypes.c_size_t
    assert L.fr_abi_version() == 1  # additive change


def _refused(L, name, rc):
    assert rc == -1 and name.encode() + b":" in L.fr_last_error(), (name, rc, L.fr_last_error())


NMS_BAD = [dict(boxes=None), dict(order=None), dict(seg_start=None), dict(keep=None), dict(seg_kept=None), dict(ws=None),
           dict(n=-1), dict(n=2 ** 30 + 1), dict(n_seg=-1), dict(thresh=NAN), dict(thresh=INF), dict(thresh=-INF),
           dict(thresh=-0.5), dict(min_mode=2), dict(ws_bytes=8), dict(boxes_off=4)]


@pytest.mark.parametrize("kw", NMS_BAD, ids=_ids)
def test_nms_rejects_unsupported_arguments(p, kw):
    L = N.lib()
    a = dict(boxes=p, order=p, seg_start=p, keep=p, seg_kept=p, ws=p, n=10, n_seg=2, thresh=0.5, min_mode=0,
             ws_bytes=1 << 40, boxes_off=0)
    a.update(kw)
    boxes = None if a["boxes"] is None else a["boxes"] + a["boxes_off"]
    _other_message(L)
    _refused(L, "fr_nms", L.fr_nms(boxes, a["n"], a["order"], a["seg_start"], a["n_seg"], a["thresh"], a["min_mode"],
                                   a["keep"], a["seg_kept"], a["ws"], a["ws_bytes"], None))


def test_nms_returns_before_any_launch(p):
    """n_seg == 0 is a no-op: FR_OK without touching the (host) pointers or the device."""
    L = N.lib()
    assert L.fr_nms(p, 10, p, p, 0, 0.5, 0, p, p, p, 1 << 40, None) == 0
    assert L.fr_nms(None, 0, None, p, 0, 0.5, 1, None, p, None, 0, None) == 0


def test_workspaces():
    L = N.lib()
    for n, n_seg in ((1, 1), (300, 5), (1 << 17, 192)):
        nws = L.fr_nms_workspace(n, n_seg)
        assert nws >= n * 24 + n_seg * 4 and nws % 16 == 0
    assert L.fr_nms_workspace(0, 0) > 0
    for args in ((-1, 1), (1, -1), (2 ** 30 + 1, 1)):
        _other_message(L)
        assert L.fr_nms_workspace(*args) == 0 and b"fr_nms_workspace:" in L.fr_last_error(), args
    assert L.fr_mtcnn_compact_workspace(1) >= 4
    assert L.fr_mtcnn_compact_workspace(3 * 70 * 90) >= 4 * (3 * 70 * 90 // 2048)
    for total in (0, -3, 2 ** 30 + 1):
        _other_message(L)
        assert L.fr_mtcnn_compact_workspace(total) == 0 and b"fr_mtcnn_compact_workspace:" in L.fr_last_error()


CAND_BAD = [dict(map=None), dict(box=None), dict(score=None), dict(reg=None), dict(seg=None), dict(counter=None),
            dict(ws=None), dict(B=0), dict(B=-1), dict(hh=0), dict(ww=-2), dict(B=2 ** 20, hh=2 ** 10, ww=2 ** 10),
            dict(scale=0.0), dict(scale=-1.0), dict(scale=NAN), dict(scale=INF), dict(thresh=NAN), dict(thresh=INF),
            dict(thresh=-0.1), dict(level=-1), dict(level=4096), dict(capacity=0), dict(capacity=-5),
            dict(capacity=2 ** 30 + 1), dict(ws_bytes=0)]


@pytest.mark.parametrize("kw", CAND_BAD, ids=_ids)
def test_candidates_rejects_unsupported_arguments(p, kw):
    L = N.lib()
    a = dict(map=p, B=2, hh=9, ww=13, scale=0.6, thresh=0.6, level=0, capacity=64, box=p, score=p, reg=p, seg=p,
             counter=p, ws=p, ws_bytes=1 << 20)
    a.update(kw)
    _other_message(L)
    _refused(L, "fr_mtcnn_candidates",
             L.fr_mtcnn_candidates(a["map"], a["B"], a["hh"], a["ww"], a["scale"], a["thresh"], a["level"], a["capacity"],
                                   a["box"], a["score"], a["reg"], a["seg"], a["counter"], a["ws"], a["ws_bytes"], None))


SEL_BAD = [dict(out=None), dict(box=None), dict(img=None), dict(obox=None), dict(oscore=None), dict(oreg=None),
           dict(oimg=None), dict(counter=None), dict(ws=None), dict(n=0), dict(n=-1), dict(C=5), dict(C=16),  # no opts
           dict(thresh=NAN), dict(thresh=-INF), dict(thresh=-1.0), dict(ws_bytes=0)]


@pytest.mark.parametrize("kw", SEL_BAD, ids=_ids)
def test_select_rejects_unsupported_arguments(p, kw):
    L = N.lib()
    a = dict(out=p, n=7, C=6, thresh=0.7, box=p, img=p, obox=p, oscore=p, oreg=p, oimg=p, opts=None, counter=p, ws=p,
             ws_bytes=1 << 20)
    a.update(kw)
    _other_message(L)
    _refused(L, "fr_mtcnn_select",
             L.fr_mtcnn_select(a["out"], a["n"], a["C"], a["thresh"], a["box"], a["img"], a["obox"], a["oscore"],
                               a["oreg"], a["oimg"], a["opts"], a["counter"], a["ws"], a["ws_bytes"], None))
    if not kw.get("C"):  # C = 6 with a landmark buffer is refused as well
        _other_message(L)
        _refused(L, "fr_mtcnn_select",
                 L.fr_mtcnn_select(a["out"], a["n"], 6, a["thresh"], a["box"], a["img"], a["obox"], a["oscore"],
                                   a["oreg"], a["oimg"], p, a["counter"], a["ws"], a["ws_bytes"], None))


CROP_BAD = [dict(box=None), dict(score=None), dict(reg=None), dict(img=None), dict(obox=None), dict(oscore=None),
            dict(oimg=None), dict(regions=None), dict(counter=None), dict(ws=None), dict(n=0), dict(n=-7), dict(B=0),
            dict(W=0), dict(H=-1), dict(plus1=2), dict(ws_bytes=0)]


@pytest.mark.parametrize("kw", CROP_BAD, ids=_ids)
def test_crop_boxes_rejects_unsupported_arguments(p, kw):
    L = N.lib()
    a = dict(box=p, score=p, reg=p, img=p, n=7, B=2, keep=None, n_keep=None, plus1=1, W=80, H=64, obox=p, oscore=p,
             oimg=p, regions=p, counter=p, ws=p, ws_bytes=1 << 20)
    a.update(kw)
    _other_message(L)
    _refused(L, "fr_mtcnn_crop_boxes",
             L.fr_mtcnn_crop_boxes(a["box"], a["score"], a["reg"], a["img"], a["n"], a["B"], a["keep"], a["n_keep"],
                                   a["plus1"], a["W"], a["H"], a["obox"], a["oscore"], a["oimg"], a["regions"],
                                   a["counter"], a["ws"], a["ws_bytes"], None))


FINAL_BAD = [dict(box=None), dict(reg=None), dict(pts=None), dict(obox=None), dict(opts=None), dict(n=0), dict(n=-1)]


@pytest.mark.parametrize("kw", FINAL_BAD, ids=_ids)
def test_final_boxes_rejects_unsupported_arguments(p, kw):
    L = N.lib()
    a = dict(box=p, reg=p, pts=p, n=3, n_dev=None, obox=p, opts=p)
    a.update(kw)
    _other_message(L)
    _refused(L, "fr_mtcnn_final_boxes",
             L.fr_mtcnn_final_boxes(a["box"], a["reg"], a["pts"], a["n"], a["n_dev"], a["obox"], a["opts"], None))
