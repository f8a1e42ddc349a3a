"""The device t-SNE (fr_tsne_*, facerecognition_amd.tsne) against the float64 restatement tests/tsne_ref.py.
eps = 2^-24 in every tolerance.  Measured values are recorded in the docstrings of the tests that print them."""
import functools
import os

import numpy as np
import pytest

from tests import tsne_ref as R

pytestmark = pytest.mark.gpu
EPS = R.EPS32
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "tsne_golden.npz")


def _torch():
    import torch
    return torch


def _dev(a, dtype):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _native():
    from facerecognition_amd import _native as N
    return N, N.lib()


def knn_sqdist(x, idx):
    torch = _torch()
    N, L = _native()
    n, d = x.shape
    k = idx.shape[1]
    xd, idd = _dev(x, np.float32), _dev(idx, np.int32)
    out = torch.empty((n, k), dtype=torch.float32, device="cuda")
    N.check(L.fr_tsne_knn_sqdist(N.ptr(xd), n, d, N.ptr(idd), k, N.ptr(out), N.stream_ptr()), "fr_tsne_knn_sqdist")
    return out.cpu().numpy()


def affinities(idx, d2, perplexity):
    """-> (indptr, col, val, beta) as numpy, and the device CSR tensors."""
    torch = _torch()
    N, L = _native()
    n, k = idx.shape
    idd, dd = _dev(idx, np.int32), _dev(d2, np.float32)
    nws = L.fr_tsne_affinities_workspace(n, k)
    assert nws > 0
    ws = torch.empty((nws,), dtype=torch.uint8, device="cuda")
    indptr = torch.empty((n + 1,), dtype=torch.int32, device="cuda")
    col = torch.full((2 * n * k,), -7, dtype=torch.int32, device="cuda")
    val = torch.full((2 * n * k,), -7.0, dtype=torch.float32, device="cuda")
    beta = torch.empty((n,), dtype=torch.float32, device="cuda")
    N.check(L.fr_tsne_affinities(N.ptr(idd), N.ptr(dd), n, k, float(perplexity), N.ptr(indptr), N.ptr(col), N.ptr(val),
                                 N.ptr(beta), N.ptr(ws), nws, N.stream_ptr()), "fr_tsne_affinities")
    ip = indptr.cpu().numpy()
    nnz = int(ip[n])
    assert np.all(col[nnz:].cpu().numpy() == -7) and np.all(val[nnz:].cpu().numpy() == -7.0)  # nothing past the end
    return ip, col[:nnz].cpu().numpy(), val[:nnz].cpu().numpy(), beta.cpu().numpy(), (indptr, col, val)


class Csr:
    """A CSR P on the device with its dense float64 copy (of the float32 values the device reads)."""

    def __init__(self, indptr, col, val, n):
        self.n = n
        val32 = np.asarray(val, np.float32)
        self.dense = R.csr_to_dense(indptr, col, val32.astype(np.float64), n)
        self.indptr, self.col, self.val = _dev(indptr, np.int32), _dev(col, np.int32), _dev(val32, np.float32)


@functools.lru_cache(maxsize=None)
def random_csr(n):
    rng = np.random.RandomState(n)
    x = rng.standard_normal((n, 8))
    k = min(n - 1, 10)
    idx, d2 = R.knn_bruteforce(x, k)
    _, p = R.binary_search_perplexity(d2, min(3.0, max(k / 2.0, 1.0)))
    return Csr(*R.joint_csr(idx, p), n)


def _workspace(n):
    torch = _torch()
    _, L = _native()
    gws = L.fr_tsne_gradient_workspace(n)
    assert gws > 0
    return torch.empty((gws,), dtype=torch.uint8, device="cuda"), gws


def gradient(csr, y, e):
    torch = _torch()
    N, L = _native()
    n = csr.n
    yd = _dev(y, np.float32)
    ws, gws = _workspace(n)
    grad = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    stats = torch.empty((3,), dtype=torch.float64, device="cuda")
    N.check(L.fr_tsne_gradient(N.ptr(csr.indptr), N.ptr(csr.col), N.ptr(csr.val), n, N.ptr(yd), float(e), N.ptr(grad),
                               N.ptr(stats), N.ptr(ws), gws, N.stream_ptr()), "fr_tsne_gradient")
    return grad.cpu().numpy(), stats.cpu().numpy()


def run(csr, state, e, momentum, lr, n_steps):
    """state = (Y, update, gains) device tensors, updated in place; returns (grad, stats) as numpy."""
    torch = _torch()
    N, L = _native()
    n = csr.n
    ws, gws = _workspace(n)
    grad = torch.empty((n, 2), dtype=torch.float32, device="cuda")
    stats = torch.empty((3,), dtype=torch.float64, device="cuda")
    y, u, g = state
    N.check(L.fr_tsne_run(N.ptr(csr.indptr), N.ptr(csr.col), N.ptr(csr.val), n, N.ptr(y), N.ptr(u), N.ptr(g), float(e),
                          float(momentum), float(lr), int(n_steps), N.ptr(grad), N.ptr(stats), N.ptr(ws), gws,
                          N.stream_ptr()), "fr_tsne_run")
    return grad.cpu().numpy(), stats.cpu().numpy()


# ---- 1. squared distances ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [4, 64, 512])
@pytest.mark.parametrize("k", [1, 31, 69])
def test_knn_sqdist(d, k):
    n = 70
    rng = np.random.RandomState(d * 100 + k)
    x = rng.standard_normal((n, d)).astype(np.float32)
    idx = np.stack([rng.permutation(np.delete(np.arange(n), i))[:k] for i in range(n)]).astype(np.int32)
    ref = R.sqdist(x, idx)
    got = knn_sqdist(x, idx)
    assert np.all(np.abs(got - ref) <= (d + 4) * EPS * ref), np.abs((got - ref) / ref).max() / EPS


# ---- 2. neighbour sets -------------------------------------------------------------------------------------------------
def _neighbour_sets(x, k, min_gap):
    from facerecognition_amd.tsne import TSNE

    ref_idx, d2 = R.knn_bruteforce(x, k + 1)
    assert (d2[:, k] - d2[:, k - 1]).min() >= min_gap  # the cluster boundary: the sets are well defined in float32
    got = TSNE()._neighbors(x, k).cpu().numpy()
    assert got.shape == (x.shape[0], k) and got.dtype == np.int32
    for i in range(x.shape[0]):
        assert i not in got[i] and len(set(got[i])) == k
        assert set(got[i]) == set(ref_idx[i, :k]), i


def test_neighbour_sets_unit_rows():
    x, _ = R.planted_clusters(8, 32, 512, 0.6, 0)
    _neighbour_sets(x, 31, 1.0)


def test_neighbour_sets_unnormalised_rows():
    """Centres of norm 1 to 3, rows not renormalised: the augmented search.  The gap asserted (0.5) is far above the
    float32 rounding of the augmented inner products (about 1e-5 at these norms)."""
    x, _ = R.planted_clusters(8, 32, 512, 0.6, 1, centre_norms=np.linspace(1, 3, 8), normalise=False)
    assert np.abs(np.linalg.norm(x, axis=1) - 1).max() > 0.1
    _neighbour_sets(x, 31, 0.5)


def test_neighbour_sets_odd_dimension():
    """D = 30 is no multiple of 4: unit rows still go through the zero-padded augmented search."""
    x, _ = R.planted_clusters(4, 16, 30, 0.3, 2)
    _neighbour_sets(x, 15, 0.2)


# ---- 3. affinities -----------------------------------------------------------------------------------------------------
def _affinity_case(name):
    if name == "special":  # two duplicate rows (a zero distance) and a row whose k distances are all equal
        x, _ = R.planted_clusters(4, 10, 16, 0.6, 9)
        x[5] = x[4]
        idx, d2 = R.knn_bruteforce(x, 8)
        d2[7, :] = 0.5
        return idx, d2.astype(np.float32), 4.0
    n, k, perplexity = name
    x, _ = R.planted_clusters(max(n // 32, 1), n // max(n // 32, 1) + 1, 16, 0.6, n)
    idx, d2 = R.knn_bruteforce(x[:n], k)
    return idx, d2.astype(np.float32), float(perplexity)


@pytest.mark.parametrize("case", [(2, 1, 1), (33, 32, 10), (256, 31, 10), (257, 91, 30), (600, 15, 5), "special"],
                         ids=str)  # (600, 15, 5): two source-row splits per transpose
def test_affinities(case):
    """Entropy slack: the search stops at |H - log perplexity| <= 1e-5 in float64 and beta is then rounded to float32,
    a relative change of at most eps, which moves H by beta^2 Var_p(d) eps to first order; the slack allowed per row
    is twice that.  A row whose distances are all equal has H = log k whatever beta is, so it is checked for
    p = 1 / k instead.  Measured on an MI355X: the largest |H - log perplexity| - 1e-5 over these cases is negative,
    -0.15 of the slack (no row left the 1e-5 band, so the slack was not used)."""
    idx, d2, perplexity = _affinity_case(case)
    n, k = idx.shape
    indptr, col, val, beta, _ = affinities(idx, d2, perplexity)
    assert np.all(np.isfinite(beta)) and np.all(beta > 0)
    p = R.p_from_beta(d2, beta.astype(np.float64))
    ref_indptr, ref_col, ref_val = R.joint_csr(idx, p)
    assert np.array_equal(indptr, ref_indptr) and np.array_equal(col, ref_col)
    rel = (np.abs(beta.astype(np.float64)[:, None] * d2) + 16) * 2 * EPS
    _, _, tol = R.joint_csr(idx, p * rel)
    assert np.all(np.abs(val - ref_val) <= tol), (np.abs(val - ref_val) / tol).max()
    assert abs(float(val.astype(np.float64).sum()) - 1.0) <= (len(val) + 16) * EPS
    if k > perplexity:
        d = d2.astype(np.float64)
        mean = (p * d).sum(1, keepdims=True)
        var = (p * (d - mean) ** 2).sum(1)
        flat = d2.max(1) == d2.min(1)
        if case == "special":
            assert flat[7] and flat.sum() == 1
            np.testing.assert_allclose(p[7], 1.0 / k, rtol=1e-12)
        slack = 2 * EPS * beta.astype(np.float64) ** 2 * var + 1e-12
        excess = np.abs(R.entropy(p) - np.log(perplexity)) - 1e-5
        print("entropy: largest excess over 1e-5 as a share of the slack: %.3g" % (excess[~flat] / slack[~flat]).max())
        assert np.all(excess[~flat] <= slack[~flat])


# ---- 4. gradient and KL ------------------------------------------------------------------------------------------------
def _check_gradient(csr, y, e):
    n = csr.n
    ref = R.gradient(csr.dense, y.astype(np.float64), e)
    grad, (kl, z, gnorm) = gradient(csr, y, e)
    bound = (n + 16) * EPS * ref["bound"]
    ok = np.abs(grad - ref["grad"]) <= bound
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.nanmax(np.where(bound > 0, np.abs(grad - ref["grad"]) / bound, 0.0))
    rz = abs(z - ref["z"]) / ((n + 16) * EPS * ref["z_abs"])
    rk = abs(kl - ref["kl"]) / ((n + 16) * EPS * ref["kl_abs"])
    rn = abs(gnorm - ref["gnorm"]) / ((n + 16) * EPS * np.sqrt((ref["bound"] ** 2).sum()) + 1e-300)
    print("N %d e %g: largest error / bound: grad %.3g Z %.3g KL %.3g |grad| %.3g" % (n, e, ratio, rz, rk, rn))
    assert ok.all(), ratio
    assert rz <= 1 and rk <= 1 and rn <= 1, (rz, rk, rn)
    return ratio


@pytest.mark.parametrize("e", [1.0, 12.0])
@pytest.mark.parametrize("scale", [1e-4, 1.0, 30.0])
@pytest.mark.parametrize("n", [2, 63, 64, 65, 257, 1000])
def test_gradient_and_kl(n, scale, e):
    """Per component |g - g64| <= (N + 16) eps S_i (the any-order summation bound plus 16 roundings per term); Z and KL
    the same against their own absolute sums.  Measured on an MI355X, largest error / bound over these cases: gradient
    0.112 (N = 64, scale 30, e = 1), Z 0.054, KL 0.0079."""
    y = (scale * np.random.RandomState(n).standard_normal((n, 2))).astype(np.float32)
    _check_gradient(random_csr(n), y, e)


def test_gradient_with_two_identical_points():
    n = 65
    y = np.random.RandomState(3).standard_normal((n, 2)).astype(np.float32)
    y[4] = y[3]
    _check_gradient(random_csr(n), y, 12.0)


def test_gradient_repulsion_over_several_j_tiles():
    """N = 16645 is the smallest size class at which a repulsion block walks more than one 256-point j tile (64 splits
    of 261 points).  P is empty here, so g = -4 rep / Z; the float64 reference is torch's, in row chunks, on the GPU."""
    torch = _torch()
    n = 16645
    y = (30 * np.random.RandomState(8).standard_normal((n, 2))).astype(np.float32)
    y[100] = y[99]
    empty = Csr.__new__(Csr)  # no dense copy at this size
    empty.n = n
    empty.indptr, empty.col, empty.val = _dev(np.zeros(n + 1), np.int32), _dev(np.zeros(1), np.int32), _dev(
        np.zeros(1), np.float32)
    grad, (kl, z, gnorm) = gradient(empty, y, 1.0)
    yd = _dev(y, np.float64)
    rep, rep_abs, zref = torch.zeros_like(yd), torch.zeros_like(yd), 0.0
    for r0 in range(0, n, 2048):
        diff = yd[r0:r0 + 2048, None, :] - yd[None, :, :]
        w = 1.0 / (1.0 + (diff ** 2).sum(-1))
        w[torch.arange(diff.shape[0]), torch.arange(r0, r0 + diff.shape[0])] = 0.0
        zref += float(w.sum())
        rep[r0:r0 + 2048] = ((w * w)[:, :, None] * diff).sum(1)
        rep_abs[r0:r0 + 2048] = ((w * w)[:, :, None] * diff.abs()).sum(1)
    ref = (-4.0 * rep / zref).cpu().numpy()
    bound = (n + 16) * EPS * (4.0 * rep_abs / zref).cpu().numpy()
    ratio = float((np.abs(grad - ref) / bound).max())
    print("N %d: largest error / bound: grad %.3g Z %.3g" % (n, ratio, abs(z - zref) / ((n + 16) * EPS * zref)))
    assert ratio <= 1 and abs(z - zref) <= (n + 16) * EPS * zref
    assert abs(kl - np.log(zref)) <= (n + 16) * EPS * abs(np.log(zref))


# ---- 5. one optimiser step ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e,momentum", [(12.0, 0.5), (1.0, 0.8)])
@pytest.mark.parametrize("n", [65, 1000])
def test_one_optimiser_step(n, e, momentum):
    """gains, update and Y after one step, on every component whose reference |g| exceeds 4 x the gradient bound (on
    the rest the sign of update * g is not decided in float32; at most 1 % may be skipped).  Tolerances: gains 4 eps;
    update lr gains bound + 4 eps per operation; Y that plus 4 eps (|y| + |update|).  Measured on an MI355X, largest
    error / tolerance: gains 0.30, update 0.031, Y 0.048; skipped at most 0.15 % (the reference alone: the same set)."""
    lr = 200.0
    rng = np.random.RandomState(n + int(e))
    y = rng.standard_normal((n, 2)).astype(np.float32)
    u = (0.1 * rng.standard_normal((n, 2))).astype(np.float32)
    g = rng.uniform(0.01, 2.0, (n, 2)).astype(np.float32)
    csr = random_csr(n)
    ref = R.gradient(csr.dense, y.astype(np.float64), e)
    bound = (n + 16) * EPS * ref["bound"]
    y1, u1, g1 = R.step(ref["grad"], y.astype(np.float64), u.astype(np.float64), g.astype(np.float64), momentum, lr)
    state = (_dev(y, np.float32), _dev(u, np.float32), _dev(g, np.float32))
    run(csr, state, e, momentum, lr, 1)
    yd, ud, gd = (t.cpu().numpy() for t in state)
    decided = np.abs(ref["grad"]) > 4 * bound
    assert (~decided).mean() <= 0.01, (~decided).mean()
    tol_g = 4 * EPS * np.abs(g1)
    tol_u = lr * g1 * bound + 4 * EPS * (np.abs(momentum * u) + 3 * np.abs(lr * g1 * ref["grad"]))
    tol_y = tol_u + 4 * EPS * (np.abs(y) + np.abs(u1))
    r = [float((np.abs(a - b) / t)[decided].max()) for a, b, t in ((gd, g1, tol_g), (ud, u1, tol_u), (yd, y1, tol_y))]
    print("N %d e %g: skipped %.4f; largest error / tolerance: gains %.3g update %.3g Y %.3g" % (
        n, e, (~decided).mean(), *r))
    assert max(r) <= 1, r


# ---- 6. repeatability --------------------------------------------------------------------------------------------------
def test_runs_are_bitwise_repeatable():
    n = 1000
    csr = random_csr(n)
    rng = np.random.RandomState(11)
    y0 = (1e-2 * rng.standard_normal((n, 2))).astype(np.float32)

    def fresh():
        return _dev(y0, np.float32), _dev(np.zeros((n, 2)), np.float32), _dev(np.ones((n, 2)), np.float32)

    a, b, c = fresh(), fresh(), fresh()
    ga, sa = run(csr, a, 12.0, 0.5, 200.0, 100)
    gb, sb = run(csr, b, 12.0, 0.5, 200.0, 100)
    run(csr, c, 12.0, 0.5, 200.0, 50)
    gc, sc = run(csr, c, 12.0, 0.5, 200.0, 50)
    for ta, tb, tc in zip(a, b, c):
        va, vb, vc = ta.cpu().numpy(), tb.cpu().numpy(), tc.cpu().numpy()
        assert np.all(np.isfinite(va))
        assert va.tobytes() == vb.tobytes()
        assert va.tobytes() == vc.tobytes()
    assert ga.tobytes() == gb.tobytes() == gc.tobytes() and sa.tobytes() == sb.tobytes() == sc.tobytes()
    assert not np.array_equal(a[0].cpu().numpy(), y0)


def test_repulsion_op_writes_the_partials_only():
    """fr_op_tsne_repulsion (the timing entry): the same bits twice, {fx, fy, z, 0} records and nothing else in a
    zeroed workspace."""
    N, L = _native()
    n = 1000
    y = _dev(30 * np.random.RandomState(5).standard_normal((n, 2)), np.float32)
    outs = []
    for _ in range(2):
        ws, gws = _workspace(n)
        ws.zero_()
        N.check(L.fr_op_tsne_repulsion(N.ptr(y), n, N.ptr(ws), gws, N.stream_ptr()), "fr_op_tsne_repulsion")
        outs.append(ws.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    part = outs[0].view(np.float32)
    assert np.all(part.reshape(-1, 4)[:, 3] == 0)
    assert np.all(np.isfinite(part)) and np.count_nonzero(part) >= 3 * n
    # the z partials add up to the float64 Z: word 2 of each {fx, fy, z, 0} record, the records being all that is written
    ref = R.gradient(np.zeros((n, n)), y.cpu().numpy().astype(np.float64))
    z = part[:part.size // 4 * 4].reshape(-1, 4)[:, 2].astype(np.float64).sum()
    assert abs(z - ref["z"]) <= (n + 16) * EPS * ref["z"]


# ---- 7. end to end -----------------------------------------------------------------------------------------------------
def test_end_to_end_layout_separates_the_clusters():
    """The device run is one more draw from the local optima the float64 restatement's 8 seeded runs sample
    (tests/golden/tsne_golden.npz, tools/gen_tsne_golden.py): KL and trustworthiness must lie within their range
    widened by 3 x that range on each side, and every point's nearest 2-D neighbour must share its cluster."""
    from facerecognition_amd.tsne import TSNE

    with np.load(GOLDEN) as z:
        gold = {k: z[k] for k in z.files}
    x, labels = R.planted_clusters(int(gold["clusters"]), int(gold["per"]), int(gold["dim"]), float(gold["noise"]),
                                   int(gold["data_seed"]))
    t = TSNE(perplexity=float(gold["perplexity"]), max_iter=int(gold["max_iter"]), init="random", random_state=0)
    y = t.fit_transform(x)
    assert y.shape == (x.shape[0], 2) and y.dtype == np.float32 and np.all(np.isfinite(y))
    assert t.n_iter_ == int(gold["max_iter"]) - 1 and t.learning_rate_ == 50.0
    assert np.all(gold["purity"] == 1.0)
    assert R.nearest_neighbour_purity(y, labels) == 1.0

    def within(v, ref):
        lo, hi = ref.min(), ref.max()
        return lo - 3 * (hi - lo) <= v <= hi + 3 * (hi - lo)

    print("KL %.4f (restatement %.4f .. %.4f)" % (t.kl_divergence_, gold["kl"].min(), gold["kl"].max()))
    assert within(t.kl_divergence_, gold["kl"])
    try:
        from sklearn.manifold import trustworthiness
    except ImportError:
        return
    tw = trustworthiness(x, y, n_neighbors=5)
    print("trustworthiness %.4f (restatement %.4f .. %.4f)" % (tw, gold["trustworthiness"].min(),
                                                               gold["trustworthiness"].max()))
    assert within(tw, gold["trustworthiness"])


# ---- 8. visualize_tsne / full_pipeline ---------------------------------------------------------------------------------
def test_visualize_tsne_and_full_pipeline(tmp_path, monkeypatch, capsys):
    from facerecognition_amd import extract_embeddings as E

    x, labels = R.planted_clusters(6, 50, 64, 0.6, 4)
    out = tmp_path / "tsne.png"
    y = E.visualize_tsne(x, labels, str(out), num_samples=200)
    assert y.shape == (200, 2) and np.all(np.isfinite(y))
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        assert not out.exists()
    else:
        assert out.stat().st_size > 0
    capsys.readouterr()
    # full_pipeline with its earlier stages stubbed: it lays the embeddings out instead of printing "skipped"
    monkeypatch.setattr(E, "extract_embeddings_from_csv", lambda *a, **k: {"embeddings": x[:64], "labels": labels[:64]})
    monkeypatch.setattr(E, "compute_prototypes", lambda *a, **k: x[:2])
    monkeypatch.setattr(E, "build_faiss_index", lambda *a, **k: None)
    E.full_pipeline("model.pth", "faces.csv", output_dir=str(tmp_path))
    text = capsys.readouterr().out
    assert "skipped" not in text and "Running t-SNE on 64 samples..." in text
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        return
    assert (tmp_path / "tsne_visualization.png").stat().st_size > 0
