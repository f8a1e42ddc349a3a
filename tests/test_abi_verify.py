"""The fr_verify_* entry points at the C-ABI boundary, without a GPU: declared, exported, bound, and every unsupported
argument refused with FR_ERR_ARG and a message naming the entry point before any HIP call (the pointers below are host
memory and are never dereferenced, the thresholds aside, which are a host array by contract).  Also the Python face's
names, defaults and its refusal of CPU tensors."""
import ctypes
import inspect

import numpy as np
import pytest

from facerecognition_amd import _native as N

NEW = {"fr_verify_workspace": 2, "fr_verify_pairs": 19}
INF, NAN = float("inf"), float("nan")


def _p():
    buf = (ctypes.c_uint64 * 64)()
    return buf, ctypes.addressof(buf)


def _other_message(L):
    L.fr_op_avgpool(None, 1, 1, 1, 8, None, 0, None)  # leaves another entry point's message behind


def _ids(kw):
    return ",".join(f"{k}={v}" for k, v in kw.items())


def min_ws(n):
    return 4 * 64 * ((n + 63) // 64) + 2048 * ((n + 1023) // 1024)


def test_verify_functions_are_declared_exported_and_bound():
    L = N.lib()
    for name, nargs in NEW.items():
        assert name in N.header_functions(), name
        assert hasattr(L, name) and name in N._SIGS, name
        assert len(N._SIGS[name][1]) == nargs, name
    assert N._SIGS["fr_verify_workspace"][0] is ctypes.c_size_t
    assert L.fr_abi_version() == 1  # additive change


N_BAD = [dict(N=1), dict(N=0), dict(N=-5), dict(N=2 ** 22 + 1), dict(N=2 ** 30)]
D_BAD = [dict(D=0), dict(D=2), dict(D=-4), dict(D=6), dict(D=510)]
PAIRS_BAD = N_BAD + D_BAD + [
    dict(normalize=2), dict(normalize=-1),
    dict(T=-1), dict(T=65), dict(T=3, thresholds=None), dict(T=3, counts=None),
    dict(thr=(0.1, INF, 0.3)), dict(thr=(NAN, 0.2, 0.3)), dict(thr=(0.1, 0.2, -INF)),
    dict(nbins=0), dict(nbins=-3), dict(nbins=2049), dict(lo=1.0, hi=1.0), dict(lo=1.0, hi=-1.0), dict(hi=INF),
    dict(lo=-INF), dict(lo=NAN), dict(hi=NAN),
    dict(E=None), dict(labels=None), dict(totals=None), dict(ws=None),
    dict(row_score=None), dict(row_idx=None),
    dict(ws_bytes=0), dict(ws_bytes=min_ws(1500) - 1),
]


@pytest.mark.parametrize("kw", PAIRS_BAD, ids=_ids)
def test_pairs_rejects_unsupported_arguments(kw):
    L = N.lib()
    _, p = _p()
    a = dict(N=1500, D=128, normalize=1, thr=(0.1, 0.2, 0.3), T=3, thresholds=True, counts=p, totals=p, hist=p, nbins=64,
             lo=-1.0, hi=1.0, E=p, labels=p, row_score=p, row_idx=p, row_sum=p, ws=p, ws_bytes=1 << 50)
    a.update(kw)
    thr = np.array(a["thr"], np.float32)
    _other_message(L)
    rc = L.fr_verify_pairs(a["E"], a["N"], a["D"], a["labels"], a["normalize"], thr.ctypes.data if a["thresholds"] else None,
                           a["T"], a["counts"], a["totals"], a["hist"], a["nbins"], a["lo"], a["hi"], a["row_score"],
                           a["row_idx"], a["row_sum"], a["ws"], a["ws_bytes"], None)
    assert rc == -1 and b"fr_verify_pairs" in L.fr_last_error(), (kw, rc, L.fr_last_error())


def test_workspace_sizes():
    L = N.lib()
    for n, d in ((2, 16), (70, 16), (1025, 512), (46715, 512)):
        rows, chunks = (n + 63) // 64 * 64, (n + 1023) // 1024
        assert L.fr_verify_workspace(n, d) == 4 * rows + 32 * rows * chunks  # the norms and every row's partials
        assert min_ws(n) <= L.fr_verify_workspace(n, d)
    n = 2 ** 22  # above 256 MiB: whole 64-row bands
    ws = L.fr_verify_workspace(n, 512)
    assert min_ws(n) <= ws <= (256 << 20) + 4 * n and (ws - 4 * n) % (2048 * 4096) == 0
    for kw in N_BAD + D_BAD:
        a = dict(N=70, D=128)
        a.update(kw)
        _other_message(L)
        assert L.fr_verify_workspace(a["N"], a["D"]) == 0
        assert b"fr_verify_workspace" in L.fr_last_error(), kw


def test_python_face_names_defaults_and_no_cpu_fallback():
    import torch

    import facerecognition_amd as fra
    from facerecognition_amd import verification as V

    for name in ("verify_pairs", "compute_verification_accuracy", "verification_report"):
        assert getattr(fra, name) is getattr(V, name)
    sig = inspect.signature(V.compute_verification_accuracy)  # the reference's names and order; all pairs by default
    assert list(sig.parameters) == ["embeddings", "labels", "num_pairs", "threshold"]
    assert sig.parameters["num_pairs"].default is None and sig.parameters["threshold"].default == 0.5
    sig = inspect.signature(V.verify_pairs)
    assert list(sig.parameters)[:7] == ["embeddings", "labels", "thresholds", "hist_bins", "hist_range", "normalize", "rows"]
    assert [sig.parameters[k].default for k in ("thresholds", "hist_bins", "hist_range", "normalize", "rows")] == \
        [(), 0, (-1, 1), True, True]
    sig = inspect.signature(V.verification_report)
    assert list(sig.parameters) == ["embeddings", "labels", "fars", "hist_bins"]
    assert sig.parameters["fars"].default == (1e-1, 1e-2, 1e-3, 1e-4) and sig.parameters["hist_bins"].default == 2048
    assert np.array_equal(V.SWEEP, np.arange(0.1, 0.9, 0.05))
    e, y = torch.randn(8, 16), torch.arange(8) // 2
    for call in (lambda: V.verify_pairs(e, y), lambda: V.compute_verification_accuracy(e, y),
                 lambda: V.compute_verification_accuracy(e, y, 10000, 0.5), lambda: V.verification_report(e, y)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    # the reference's early returns need no device
    assert V.compute_verification_accuracy(e[:1], y[:1]) == (0.0, 0.5, {})
    assert V.compute_verification_accuracy(e[:3], [0, 0, 1], threshold=0.3) == (0.0, 0.3, {"error": "Not enough valid labels"})


def test_report_helpers_on_the_host():
    """roc_from_histograms and far_candidates are host arithmetic: a hand case."""
    from facerecognition_amd import verification as V

    hist = np.array([[0, 0, 1, 3], [2, 1, 1, 0]])  # 4 bins over [-1, 1]: genuine high, impostor low
    roc = V.roc_from_histograms(hist, (-1.0, 1.0))
    assert roc["edges"].tolist() == [-1, -0.5, 0, 0.5, 1]
    assert roc["tar"].tolist() == [1, 1, 1, 0.75, 0] and roc["far"].tolist() == [1, 0.5, 0.25, 0, 0]
    # far ascending 0, 0, 0.25, 0.5, 1 with tar 0, 0.75, 1, 1, 1
    assert roc["auc"] == pytest.approx(0.25 * (0.75 + 1) / 2 + 0.25 + 0.5)
    assert roc["eer_bin"] == 2 and roc["eer_threshold"] == 0.0 and roc["eer"] == pytest.approx(0.125)
    assert roc["dprime"] > 1.0
    ks, thr = V.far_candidates(hist[1], 4, [0.5, 0.25, 0.01], (-1.0, 1.0))
    assert ks.tolist() == [2, 1, 0] and thr.shape == (3, 21) and thr.dtype == np.float32
    # at most 2 impostors above bin 0, at most 1 above bin 1, none above bin 2: those bins are subdivided
    assert thr[0, -1] == -0.5 and thr[1, -1] == 0.0 and thr[2, -1] == 0.5
    assert thr[0, 0] == pytest.approx(-1 + 0.5 / 21, abs=1e-6) and np.all(np.diff(thr, axis=1) > 0)
