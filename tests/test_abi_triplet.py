"""The fr_triplet_* entry points at the C-ABI boundary, without a GPU: declared, exported, bound, and every unsupported
argument refused with FR_ERR_ARG and a message naming the entry point before any HIP call (the pointers below are host
memory and are never dereferenced).  Also the Python face's names, defaults and its refusal of CPU tensors."""
import ctypes
import inspect

import pytest

from facerecognition_amd import _native as N

NEW = {"fr_triplet_workspace": 2, "fr_triplet_count": 5, "fr_triplet_mine": 15, "fr_triplet_loss_forward": 11,
       "fr_triplet_loss_backward": 13}
INF, NAN = float("inf"), float("nan")


def _p():
    buf = (ctypes.c_uint64 * 64)()
    return buf, ctypes.addressof(buf)


def _other_message(L):
    L.fr_op_avgpool(None, 1, 1, 1, 8, None, 0, None)  # leaves another entry point's message behind


def _ids(kw):
    return ",".join(f"{k}={v}" for k, v in kw.items())


def test_triplet_functions_are_declared_exported_and_bound():
    L = N.lib()
    for name, nargs in NEW.items():
        assert name in N.header_functions(), name
        assert hasattr(L, name) and name in N._SIGS, name
        assert len(N._SIGS[name][1]) == nargs, name
    assert N._SIGS["fr_triplet_workspace"][0] is ctypes.c_size_t
    assert L.fr_abi_version() == 1  # additive change


N_BAD = [dict(N=1), dict(N=0), dict(N=-5), dict(N=32769), dict(N=2 ** 30)]
D_BAD = [dict(D=0), dict(D=2), dict(D=-4), dict(D=6), dict(D=510)]
MARGIN_BAD = [dict(margin=0.0), dict(margin=-0.2), dict(margin=INF), dict(margin=NAN)]
MODE_BAD = [dict(mode=-1), dict(mode=3), dict(mode=17)]


def _args(kw):
    _, p = _p()
    a = dict(N=70, D=128, mode=0, margin=0.2, T=33, u=1.0, capacity=1 << 40, E=p, labels=p, lims=p, a=p, p=p, n=p,
             semi=None, terms=p, stats=p, dE=p, ws=p, ws_bytes=1 << 50)
    a.update(kw)
    return a


@pytest.mark.parametrize("kw", N_BAD + MODE_BAD + [dict(labels=None), dict(lims=None)], ids=_ids)
def test_count_rejects_unsupported_arguments(kw):
    L = N.lib()
    a = _args(kw)
    _other_message(L)
    rc = L.fr_triplet_count(a["labels"], a["N"], a["mode"], a["lims"], None)
    assert rc == -1 and b"fr_triplet_count" in L.fr_last_error(), (kw, rc, L.fr_last_error())


MINE_BAD = N_BAD + D_BAD + MODE_BAD + MARGIN_BAD + [dict(E=None), dict(labels=None), dict(lims=None), dict(a=None),
                                                    dict(p=None), dict(n=None), dict(ws=None), dict(capacity=-1),
                                                    dict(ws_bytes=0), dict(ws_bytes=4 * (64 * 70 + 128) - 1)]


@pytest.mark.parametrize("kw", MINE_BAD, ids=_ids)
def test_mine_rejects_unsupported_arguments(kw):
    L = N.lib()
    a = _args(kw)
    _other_message(L)
    rc = L.fr_triplet_mine(a["E"], a["N"], a["D"], a["labels"], a["mode"], a["margin"], a["lims"], a["a"], a["p"],
                           a["n"], a["capacity"], a["semi"], a["ws"], a["ws_bytes"], None)
    assert rc == -1 and b"fr_triplet_mine" in L.fr_last_error(), (kw, rc, L.fr_last_error())


LOSS_BAD = N_BAD + D_BAD + MARGIN_BAD + [dict(T=0), dict(T=-3), dict(E=None), dict(a=None), dict(p=None), dict(n=None)]


@pytest.mark.parametrize("kw", LOSS_BAD + [dict(terms=None), dict(stats=None)], ids=_ids)
def test_loss_forward_rejects_unsupported_arguments(kw):
    L = N.lib()
    a = _args(kw)
    _other_message(L)
    rc = L.fr_triplet_loss_forward(a["E"], a["N"], a["D"], a["a"], a["p"], a["n"], a["T"], a["margin"], a["terms"],
                                   a["stats"], None)
    assert rc == -1 and b"fr_triplet_loss_forward" in L.fr_last_error(), (kw, rc, L.fr_last_error())


@pytest.mark.parametrize("kw", LOSS_BAD + [dict(u=INF), dict(u=NAN), dict(dE=None), dict(ws=None),
                                           dict(ws_bytes=8 * 33 - 1)], ids=_ids)
def test_loss_backward_rejects_unsupported_arguments(kw):
    L = N.lib()
    a = _args(kw)
    _other_message(L)
    rc = L.fr_triplet_loss_backward(a["E"], a["N"], a["D"], a["a"], a["p"], a["n"], a["T"], a["margin"], a["u"],
                                    a["dE"], a["ws"], a["ws_bytes"], None)
    assert rc == -1 and b"fr_triplet_loss_backward" in L.fr_last_error(), (kw, rc, L.fr_last_error())


def test_workspace_sizes():
    L = N.lib()
    for n, d in ((2, 16), (70, 16), (130, 512), (8192, 512)):
        pad = (n + 63) // 64 * 64
        assert L.fr_triplet_workspace(n, d) == 4 * (pad * n + pad)  # the whole matrix, with the norms
    n = 32768  # above 256 MiB: whole 64-anchor bands, never the whole matrix
    ws = L.fr_triplet_workspace(n, 512)
    assert 4 * (64 * n + n) <= ws <= (256 << 20) + 4 * n and (ws - 4 * n) % (4 * 64 * n) == 0
    for kw in N_BAD + D_BAD:
        a = dict(N=70, D=128)
        a.update(kw)
        _other_message(L)
        assert L.fr_triplet_workspace(a["N"], a["D"]) == 0
        assert b"fr_triplet_workspace" in L.fr_last_error(), kw


def test_python_face_names_defaults_and_no_cpu_fallback():
    import torch

    import facerecognition_amd as fra
    from facerecognition_amd import triplet as T

    for name in ("TripletLoss", "mine_triplets", "mine_semi_hard_triplets", "mine_batch_hard_triplets", "triplet_loss",
                 "online_triplet_loss", "compute_triplet_metrics"):
        assert getattr(fra, name) is getattr(T, name)
    assert inspect.signature(T.mine_semi_hard_triplets).parameters["margin"].default == 0.2
    assert inspect.signature(T.mine_triplets).parameters["margin"].default == 0.5
    assert list(inspect.signature(T.mine_batch_hard_triplets).parameters) == ["embeddings", "labels"]
    assert inspect.signature(T.online_triplet_loss).parameters["mining"].default == "semi_hard"
    crit = T.TripletLoss()
    assert crit.margin == 0.5 and T.TripletLoss(margin=0.2).margin == 0.2 and not list(crit.parameters())
    e, y = torch.randn(8, 16), torch.arange(8) // 2
    for call in (lambda: T.mine_semi_hard_triplets(e, y), lambda: T.mine_batch_hard_triplets(e, y),
                 lambda: T.mine_triplets(e, y), lambda: crit(e, e, e), lambda: T.online_triplet_loss(e, y),
                 lambda: T.triplet_loss(e, [0], [1], [2], 0.5), lambda: T.compute_triplet_metrics(e, e, e)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
