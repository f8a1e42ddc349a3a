"""The fr_tsne_* entry points at the C-ABI boundary, without a GPU: declared, exported, bound, and every unsupported
argument refused with FR_ERR_ARG and a message naming the entry point before any HIP call (the pointers below are host
memory and are never dereferenced)."""
import ctypes

import pytest

from facerecognition_amd import _native as N

NEW = {"fr_tsne_knn_sqdist": 7, "fr_tsne_affinities_workspace": 2, "fr_tsne_affinities": 12,
       "fr_tsne_gradient_workspace": 1, "fr_tsne_gradient": 11, "fr_tsne_run": 16, "fr_op_tsne_repulsion": 5}
INF, NAN = float("inf"), float("nan")


def _p():
    buf = (ctypes.c_uint64 * 64)()
    return buf, ctypes.addressof(buf)


def _other_message(L):
    L.fr_op_avgpool(None, 1, 1, 1, 8, None, 0, None)  # leaves another entry point's message behind


def _ids(kw):
    return ",".join(f"{k}={v}" for k, v in kw.items())


def test_tsne_functions_are_declared_exported_and_bound():
    L = N.lib()
    for name, nargs in NEW.items():
        assert name in N.header_functions(), name
        assert hasattr(L, name) and name in N._SIGS, name
        assert len(N._SIGS[name][1]) == nargs, name
    assert N._SIGS["fr_tsne_affinities_workspace"][0] is ctypes.c_size_t
    assert N._SIGS["fr_tsne_gradient_workspace"][0] is ctypes.c_size_t
    assert L.fr_abi_version() == 1  # additive change


SHAPE_BAD = [dict(N=1), dict(N=0), dict(N=-5), dict(k=0), dict(k=-1), dict(k=100), dict(k=101),
             dict(N=5000, k=4096), dict(N=2 ** 30, k=1), dict(N=300000, k=4000)]


@pytest.mark.parametrize("kw", SHAPE_BAD + [dict(D=0), dict(D=-3), dict(X=None), dict(idx=None), dict(d2=None)],
                         ids=_ids)
def test_knn_sqdist_rejects_unsupported_arguments(kw):
    L = N.lib()
    _, p = _p()
    a = dict(N=100, D=64, k=31, X=p, idx=p, d2=p)
    a.update(kw)
    _other_message(L)
    rc = L.fr_tsne_knn_sqdist(a["X"], a["N"], a["D"], a["idx"], a["k"], a["d2"], None)
    assert rc == -1 and b"fr_tsne_knn_sqdist" in L.fr_last_error(), (kw, rc, L.fr_last_error())


AFF_BAD = SHAPE_BAD + [dict(perplexity=0.0), dict(perplexity=-1.0), dict(perplexity=INF), dict(perplexity=NAN),
                       dict(idx=None), dict(d2=None), dict(indptr=None), dict(col=None), dict(val=None),
                       dict(beta=None), dict(ws=None), dict(ws_bytes=8)]


@pytest.mark.parametrize("kw", AFF_BAD, ids=_ids)
def test_affinities_rejects_unsupported_arguments(kw):
    L = N.lib()
    _, p = _p()
    a = dict(N=100, k=31, perplexity=10.0, idx=p, d2=p, indptr=p, col=p, val=p, beta=p, ws=p, ws_bytes=1 << 40)
    a.update(kw)
    _other_message(L)
    rc = L.fr_tsne_affinities(a["idx"], a["d2"], a["N"], a["k"], a["perplexity"], a["indptr"], a["col"], a["val"],
                              a["beta"], a["ws"], a["ws_bytes"], None)
    assert rc == -1 and b"fr_tsne_affinities" in L.fr_last_error(), (kw, rc, L.fr_last_error())


GRAD_BAD = [dict(N=1), dict(N=0), dict(N=-1), dict(N=2 ** 30), dict(e=0.0), dict(e=-2.0), dict(e=INF), dict(e=NAN),
            dict(indptr=None), dict(col=None), dict(val=None), dict(Y=None), dict(grad=None), dict(stats=None),
            dict(ws=None), dict(ws_bytes=8)]


@pytest.mark.parametrize("kw", GRAD_BAD, ids=_ids)
def test_gradient_rejects_unsupported_arguments(kw):
    L = N.lib()
    _, p = _p()
    a = dict(N=100, e=12.0, indptr=p, col=p, val=p, Y=p, grad=p, stats=p, ws=p, ws_bytes=1 << 40)
    a.update(kw)
    _other_message(L)
    rc = L.fr_tsne_gradient(a["indptr"], a["col"], a["val"], a["N"], a["Y"], a["e"], a["grad"], a["stats"], a["ws"],
                            a["ws_bytes"], None)
    assert rc == -1 and b"fr_tsne_gradient" in L.fr_last_error(), (kw, rc, L.fr_last_error())


RUN_BAD = GRAD_BAD + [dict(momentum=0.0), dict(momentum=-0.5), dict(momentum=NAN), dict(momentum=INF), dict(lr=0.0),
                      dict(lr=-1.0), dict(lr=INF), dict(lr=NAN), dict(n_steps=0), dict(n_steps=-1), dict(update=None),
                      dict(gains=None)]


@pytest.mark.parametrize("kw", RUN_BAD, ids=_ids)
def test_run_rejects_unsupported_arguments(kw):
    L = N.lib()
    _, p = _p()
    a = dict(N=100, e=12.0, momentum=0.5, lr=200.0, n_steps=50, indptr=p, col=p, val=p, Y=p, update=p, gains=p,
             grad=p, stats=p, ws=p, ws_bytes=1 << 40)
    a.update(kw)
    _other_message(L)
    rc = L.fr_tsne_run(a["indptr"], a["col"], a["val"], a["N"], a["Y"], a["update"], a["gains"], a["e"], a["momentum"],
                       a["lr"], a["n_steps"], a["grad"], a["stats"], a["ws"], a["ws_bytes"], None)
    assert rc == -1 and b"fr_tsne_run" in L.fr_last_error(), (kw, rc, L.fr_last_error())


@pytest.mark.parametrize("kw", [dict(N=1), dict(N=0), dict(N=2 ** 30), dict(Y=None),
                                dict(ws=None), dict(ws_bytes=8)], ids=_ids)
def test_op_repulsion_rejects_unsupported_arguments(kw):
    L = N.lib()
    _, p = _p()
    a = dict(N=100, Y=p, ws=p, ws_bytes=1 << 40)
    a.update(kw)
    _other_message(L)
    rc = L.fr_op_tsne_repulsion(a["Y"], a["N"], a["ws"], a["ws_bytes"], None)
    assert rc == -1 and b"fr_op_tsne_repulsion" in L.fr_last_error(), (kw, rc, L.fr_last_error())


def test_workspaces():
    L = N.lib()
    for n, k in ((2, 1), (257, 91), (46715, 91), (5000, 4095)):
        nws = L.fr_tsne_affinities_workspace(n, k)
        assert nws >= n * k * 20 and nws % 4 == 0  # P_cond, two transposed copies (columns and values)
        gws = L.fr_tsne_gradient_workspace(n)
        assert gws >= n * 32 and gws % 8 == 0      # one split of {fx, fy, z} partials and the per-row sums
    for args in ((1, 1), (100, 0), (100, 100), (5000, 4096), (2 ** 30, 1)):
        _other_message(L)
        assert L.fr_tsne_affinities_workspace(*args) == 0 and b"fr_tsne_affinities_workspace" in L.fr_last_error(), args
    for n in (1, 0, -7, 2 ** 30):
        _other_message(L)
        assert L.fr_tsne_gradient_workspace(n) == 0 and b"fr_tsne_gradient_workspace" in L.fr_last_error(), n
