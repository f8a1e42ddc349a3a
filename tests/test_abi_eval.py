"""fr_match_eval at the C-ABI boundary, without a GPU: exported, bound, and bad arguments rejected with
FR_ERR_ARG and a message naming the entry point (no compute)."""
import ctypes

from facerecognition_amd import _native as N


def test_match_eval_is_exported_and_bound():
    L = N.lib()
    assert "fr_match_eval" in N.header_functions()
    assert hasattr(L, "fr_match_eval") and "fr_match_eval" in N._SIGS
    assert len(N._SIGS["fr_match_eval"][1]) == 14
    assert hasattr(L, "fr_debug_match_eval_splits") and "fr_debug_match_eval_splits" in N._SIGS
    assert L.fr_abi_version() == 1  # additive change


def test_match_eval_rejects_bad_arguments():
    L = N.lib()
    buf = (ctypes.c_uint64 * 2048)()  # host memory: never dereferenced on these paths
    p = ctypes.addressof(buf)

    def call(P=p, B=4, t=p, k=0, s=None, i=None, ts=p, tr=p, hist=None, nbins=0, lo=-1.0, hi=1.0, h=None):
        L.fr_op_avgpool(None, 1, 1, 1, 8, None, 0, None)  # leaves another entry point's message behind
        rc = L.fr_match_eval(h, P, B, t, k, s, i, ts, tr, hist, nbins, lo, hi, None)
        return rc, L.fr_last_error()

    for kw in (dict(P=None), dict(t=None), dict(ts=None), dict(tr=None), dict(B=0), dict(B=-3),
               dict(k=5), dict(k=5, s=p), dict(k=5, i=p), dict(k=-1, s=p, i=p),
               dict(hist=p, nbins=0), dict(hist=p, nbins=2049), dict(hist=p, nbins=-1),
               dict(hist=p, nbins=512, lo=1.0, hi=1.0), dict(hist=p, nbins=512, lo=1.0, hi=-1.0),
               dict(hist=p, nbins=512, lo=0.0, hi=float("nan")),
               dict()):  # everything valid but the handle
        rc, msg = call(**kw)
        assert rc == -1 and b"fr_match_eval" in msg, (kw, rc, msg)
    assert L.fr_debug_match_eval_splits(None, 4) == -1
