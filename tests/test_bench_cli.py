"""bench.py's command line without a GPU: a plain run measures the headline only, --full switches the extra
measurements on (each still has its --no-* switch), and --dump-outputs writes float .npy files."""
import numpy as np
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr("sys.argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_measures_the_headline_only(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_prof and a.no_pmc and a.no_n1_1m and a.no_cpu_baseline


def test_full_switches_the_extras_on(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert not (a.no_prof or a.no_pmc or a.no_n1_1m or a.no_cpu_baseline)
    a = _parse(monkeypatch, "--full", "--no-pmc", "--no-cpu-baseline")
    assert a.no_pmc and a.no_cpu_baseline and not a.no_prof and not a.no_n1_1m


def test_dump_outputs_writes_float_npy(tmp_path):
    emb = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    s = torch.tensor([[0.5, 0.25], [1.0, 0.0], [0.75, 0.5]])
    i = torch.tensor([[7, 2 ** 30 + 1], [0, 1], [5, 3]], dtype=torch.int32)
    d = tmp_path / "out" / "dump"
    bench.dump_outputs(str(d), emb, s, i)
    got = {p.name: np.load(p) for p in d.iterdir()}
    assert sorted(got) == ["embeddings.npy", "topk_indices.npy", "topk_scores.npy"]
    assert got["embeddings.npy"].dtype == np.float32 and np.array_equal(got["embeddings.npy"], emb.numpy())
    assert got["topk_scores.npy"].dtype == np.float32 and np.array_equal(got["topk_scores.npy"], s.numpy())
    assert got["topk_indices.npy"].dtype == np.float64 and np.array_equal(got["topk_indices.npy"], i.numpy())
