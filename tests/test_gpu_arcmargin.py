"""fr_arcmargin_forward / fr_arcmargin_backward and facerecognition_amd.arcmargin on the GPU against the float64
restatement tests/arcmargin_ref.py, which also supplies every bound (eps = 2^-24; derivations in its docstring).
Each assertion is error / bound <= 1; the largest ratio of every quantity is printed.

Measured largest ratios (MI355X; per case in DESIGN.md §4 "ArcFace margin loss"):
  grid  (70, 4167, 512): non-label logits bitwise; label z 0.0035, lse 0.0011, loss 0.0021, dE 0.0008, dW 0.0089
  float, over the five shapes: z 0.175 (at (130, 4167, 16)), lse 0.032, loss 0.023, dE 0.0067, dW 0.059
  options: z 0.059, lse 0.035, loss 0.033, dE 0.005, dW 0.031; module path with dense dlogits: dE 0.0022, dW 0.012

Shapes: the smallest that cross each boundary of a 64 x 64 tile and of the class split (B 1 / 70 / 130,
C 2 / 333 / 4167, D 16 / 128 / 512).  Every raw C call allocates its outputs 64 sentinel elements too long and
checks that the sentinels survive.
"""
import numpy as np
import pytest

from tests.arcmargin_ref import arcmargin_ref
from tests.test_gpu_match_eval import grid_rows

pytestmark = pytest.mark.gpu

GUARD, SENT = 64, 7.5
S, M = 64.0, 0.5
PLANT = [0.9, 0.5, 0.2, -0.2, -0.6, -0.95, 0.7, -0.92, 0.35, -0.4, 0.8, -0.3]  # label cosines of the float cases
SHAPES = [(1, 2, 16), (70, 333, 128), (130, 4167, 16), (130, 333, 512), (70, 4167, 512),
          (3, 70, 576)]  # D > 512: the backward kernels run 512-column slices
worst = {}


def note(name, err, bound):
    r = float(np.max(np.abs(err) / bound))
    worst[name] = max(worst.get(name, 0.0), r)
    print(f"  {name}: largest error / bound = {r:.3g}")
    return r


def labels_for(rng, B, C):
    """Classes 0 and C - 1, the tile edges 63 and 64, one label shared by two samples, the ignored labels -1 and C;
    most classes stay unlabelled."""
    lab = rng.integers(0, C, B)
    want = [0, C - 1, 63, 64, 64, -1, C]
    if B >= 2 * len(want) and C > 64:
        lab[1:2 * len(want):2] = want
    return lab.astype(np.int64)


def float_case(seed, B, C, D):
    """Unnormalised E with row norms over [0.3, 5], Xavier W scaled per row by [0.5, 2]; every valid label's cosine
    is planted from PLANT (float64 construction, then rounded to float32)."""
    rng = np.random.default_rng(seed)
    a = np.sqrt(6.0 / (C + D))
    W = rng.uniform(-a, a, (C, D)) * rng.uniform(0.5, 2.0, (C, 1))
    lab = labels_for(rng, B, C)
    lab_b = labels_for(rng, B, C)[::-1].copy()
    E = rng.standard_normal((B, D))
    for b in range(B):
        if 0 <= lab[b] < C:
            w = W[lab[b]] / np.linalg.norm(W[lab[b]])
            n = E[b] - (E[b] @ w) * w
            n /= np.linalg.norm(n)
            c = PLANT[b % len(PLANT)]
            E[b] = c * w + np.sqrt(1 - c * c) * n
    E *= (rng.uniform(0.3, 5.0, (B, 1)) / np.linalg.norm(E, axis=1, keepdims=True))
    return E.astype(np.float32), W.astype(np.float32), lab, lab_b


def grid_case(seed=5, B=70, C=4167):
    """Exact grid (256 entries of +-1/16 among 512: norms exactly 1, cosines multiples of 1/256) with planted label
    cosines +1, -1, 0.75, 0.5, 0.953125, -0.90625, -0.953125 (copies of the class row with k sign flips, each
    worth 1/128, or of its negation)."""
    rng = np.random.default_rng(seed)
    W, E = grid_rows(rng, C), grid_rows(rng, B)
    lab = labels_for(rng, B, C)
    plant = {0: (1, 0), 2: (-1, 0), 4: (1, 32), 6: (1, 64), 8: (1, 6), 10: (-1, 12), 12: (-1, 6)}
    for b, (sign, k) in plant.items():
        E[b] = sign * W[lab[b]]
        nz = np.flatnonzero(E[b])
        flip = rng.choice(nz, k, replace=False)
        E[b, flip] = -E[b, flip]
    return E, W, lab, plant


def run_c(dev, E, W, lab, lab_b=None, lam=1.0, scale=S, margin=M, easy=False, ls=0.0, u=None, dlogits=None,
          want_logits=False, want=("dE", "dW")):
    """The two raw C calls with sentinel-guarded outputs; returns numpy results."""
    import torch
    from facerecognition_amd import _native as NL

    L = NL.lib()
    B, D = E.shape
    C = W.shape[0]
    e, w = torch.from_numpy(E).to(dev), torch.from_numpy(W).to(dev)
    y = torch.from_numpy(lab.astype(np.int32)).to(dev)
    yb = None if lab_b is None else torch.from_numpy(lab_b.astype(np.int32)).to(dev)

    def guarded(n):
        return torch.full((n + GUARD,), SENT, dtype=torch.float32, device=dev)

    nbytes = L.fr_arcmargin_workspace(B, C, D)
    assert 0 < nbytes
    ws = guarded(nbytes // 4)
    loss, lse, inv_e, inv_w = guarded(B), guarded(B), guarded(B), guarded(C)
    logits = guarded(B * C) if want_logits else None
    st = NL.stream_ptr(dev)
    NL.check(L.fr_arcmargin_forward(NL.ptr(e), B, D, NL.ptr(w), C, NL.ptr(y), NL.ptr(yb), lam, scale, margin, int(easy),
                                    ls, NL.ptr(loss), NL.ptr(lse), NL.ptr(inv_e), NL.ptr(inv_w), NL.ptr(logits),
                                    NL.ptr(ws), nbytes, st), "fr_arcmargin_forward")
    out = {}
    dE = guarded(B * D) if "dE" in want else None
    dW = guarded(C * D) if "dW" in want else None
    if want:
        ut = None if dlogits is not None else torch.from_numpy(
            (np.ones(B) if u is None else u).astype(np.float32)).to(dev)
        dl = None if dlogits is None else torch.from_numpy(dlogits.astype(np.float32)).to(dev).contiguous()
        NL.check(L.fr_arcmargin_backward(NL.ptr(e), B, D, NL.ptr(w), C, NL.ptr(y), NL.ptr(yb), lam, scale, margin,
                                         int(easy), ls, NL.ptr(lse), NL.ptr(inv_e), NL.ptr(inv_w), NL.ptr(ut),
                                         NL.ptr(dl), NL.ptr(dE), NL.ptr(dW), NL.ptr(ws), nbytes, st),
                 "fr_arcmargin_backward")
    torch.cuda.synchronize()
    for name, t, n in (("loss", loss, B), ("lse", lse, B), ("inv_e", inv_e, B), ("inv_w", inv_w, C),
                       ("z", logits, B * C), ("dE", dE, B * D), ("dW", dW, C * D), ("ws", ws, nbytes // 4)):
        if t is not None:
            h = t.cpu().numpy()
            assert np.all(h[n:] == SENT), f"{name}: a sentinel past the end was overwritten"
            out[name] = h[:n]
    for name, shape in (("z", (B, C)), ("dE", (B, D)), ("dW", (C, D))):
        if name in out:
            out[name] = out[name].reshape(shape)
    return out


def check_forward(tag, got, r):
    z = got["z"].astype(np.float64)
    ok = note(f"{tag} z", z - r["z"], r["z_bound"]) <= 1
    ok &= note(f"{tag} lse", got["lse"] - r["lse"], r["lse_bound"]) <= 1
    ok &= note(f"{tag} loss", got["loss"] - r["loss"], r["loss_bound"]) <= 1
    return ok


def check_condition(r, lab, C):
    """Every label cosine is at least 1e-3 from the branch point, and 1 - c^2 >= 1e-3 unless c is exactly +-1."""
    v = (lab >= 0) & (lab < C)
    c, q = r["c_label"][v], r["q_label"][v]
    assert np.all(np.abs(c - r["th"]) >= 1e-3), np.abs(c - r["th"]).min()
    assert np.all((q >= 1e-3) | (np.abs(c) == 1.0)), q.min()


@pytest.fixture(scope="module")
def grid(gpu):
    E, W, lab, plant = grid_case()
    r = arcmargin_ref(E, W, lab, scale=S, margin=M, label_smoothing=0.1)
    got = run_c(gpu, E, W, lab, ls=0.1, want_logits=True)
    return dict(E=E, W=W, lab=lab, plant=plant, ref=r, got=got)


# 1
def test_exact_grid(grid):
    r, got, lab, C = grid["ref"], grid["got"], grid["lab"], grid["W"].shape[0]
    want = {0: 1.0, 2: -1.0, 4: 0.75, 6: 0.5, 8: 0.953125, 10: -0.90625, 12: -0.953125}
    for b, c in want.items():
        assert r["c_label"][b] == c, (b, r["c_label"][b])
    assert np.sum(r["c_label"][list(want)] < r["th"]) == 3
    assert np.all(got["inv_e"] == 1.0) and np.all(got["inv_w"] == 1.0)
    mask = np.ones(r["z"].shape, bool)
    v = (lab >= 0) & (lab < C)
    mask[np.arange(len(lab))[v], lab[v]] = False
    assert np.array_equal(got["z"].astype(np.float64)[mask], r["z"][mask])  # bit for bit: multiples of 1/4
    assert check_forward("grid", got, r)
    assert np.all(got["loss"][~v] == 0)
    assert note("grid dE", got["dE"] - r["dE"], r["dE_bound"] + 1e-300) <= 1
    assert note("grid dW", got["dW"] - r["dW"], r["dW_bound"] + 1e-300) <= 1


# 2
@pytest.mark.parametrize("B,C,D", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("easy", [False, True], ids=["margin", "easy"])
def test_float_inputs(gpu, B, C, D, easy):
    E, W, lab, _ = float_case(100 + B + C + D, B, C, D)
    u = np.linspace(0.5, 2.0, B) * np.where(np.arange(B) % 5 == 3, -1.0, 1.0)
    r = arcmargin_ref(E, W, lab, scale=S, margin=M, easy_margin=easy, label_smoothing=0.1, u=u)
    check_condition(r, lab, C)
    got = run_c(gpu, E, W, lab, easy=easy, ls=0.1, u=u, want_logits=True)
    tag = f"float{(B, C, D)}{'e' if easy else ''}"
    assert note(f"{tag} inv_e", got["inv_e"] - r["inv_e"], (D + 4) * 2.0 ** -24 * r["inv_e"]) <= 1
    assert check_forward(tag, got, r)
    assert note(f"{tag} dE", got["dE"] - r["dE"], r["dE_bound"] + 1e-300) <= 1
    assert note(f"{tag} dW", got["dW"] - r["dW"], r["dW_bound"] + 1e-300) <= 1


# 3
@pytest.mark.parametrize("easy", [False, True], ids=["margin", "easy"])
@pytest.mark.parametrize("ls", [0.0, 0.1])
@pytest.mark.parametrize("lam", [1.0, 0.3])
def test_options(gpu, easy, ls, lam):
    B, C, D = 70, 333, 128
    E, W, lab, lab_b = float_case(7, B, C, D)
    mix = lab_b if lam < 1 else None
    u = np.linspace(2.0, 0.25, B) * np.where(np.arange(B) % 4 == 1, -1.0, 1.0)
    r = arcmargin_ref(E, W, lab, mix, lam=lam, scale=S, margin=M, easy_margin=easy, label_smoothing=ls, u=u)
    check_condition(r, lab, C)
    got = run_c(gpu, E, W, lab, mix, lam=lam, easy=easy, ls=ls, u=u, want_logits=True)
    assert check_forward("options", got, r)
    assert note("options dE", got["dE"] - r["dE"], r["dE_bound"] + 1e-300) <= 1
    assert note("options dW", got["dW"] - r["dW"], r["dW_bound"] + 1e-300) <= 1
    only_e = run_c(gpu, E, W, lab, mix, lam=lam, easy=easy, ls=ls, u=u, want=("dE",))
    only_w = run_c(gpu, E, W, lab, mix, lam=lam, easy=easy, ls=ls, u=u, want=("dW",))
    assert "dW" not in only_e and "dE" not in only_w
    assert np.array_equal(only_e["dE"], got["dE"]) and np.array_equal(only_w["dW"], got["dW"])
    assert np.array_equal(only_e["loss"], got["loss"])  # with and without the optional logits


# 4
def test_module_path(gpu):
    import torch
    from facerecognition_amd.arcmargin import ArcMarginProduct, arcface_loss

    B, C, D = 70, 333, 128
    E, W, lab, lab_b = float_case(7, B, C, D)
    head = ArcMarginProduct(D, C, scale=S, margin=M).to(gpu)
    head.load_state_dict({"weight": torch.from_numpy(W)})
    x = torch.from_numpy(E).to(gpu).requires_grad_(True)
    y = torch.from_numpy(lab).to(gpu)
    z = head(x, y)
    raw = run_c(gpu, E, W, lab, want_logits=True, want=())
    assert np.array_equal(z.detach().cpu().numpy(), raw["z"])  # bit for bit
    dl = np.random.default_rng(3).standard_normal((B, C)).astype(np.float32)
    z.backward(torch.from_numpy(dl).to(gpu))
    r = arcmargin_ref(E, W, lab, scale=S, margin=M, dlogits=dl)
    assert note("module dE", x.grad.cpu().numpy() - r["dE"], r["dE_bound"] + 1e-300) <= 1
    assert note("module dW", head.weight.grad.cpu().numpy() - r["dW"], r["dW_bound"] + 1e-300) <= 1

    u = np.linspace(0.5, 2.0, B).astype(np.float32)
    for red, uu in (("none", u), ("sum", np.ones(B, np.float32))):
        x.grad = None
        head.zero_grad()
        loss = head.loss(x, y, torch.from_numpy(lab_b).to(gpu), lam=0.3, label_smoothing=0.1, reduction=red)
        (loss * torch.from_numpy(uu).to(gpu)).sum().backward() if red == "none" else loss.backward()
        c = run_c(gpu, E, W, lab, lab_b, lam=0.3, ls=0.1, u=uu.astype(np.float64))
        assert np.array_equal(x.grad.cpu().numpy(), c["dE"]) and np.array_equal(head.weight.grad.cpu().numpy(), c["dW"])
        want = c["loss"] if red == "none" else None
        if want is not None:
            assert np.array_equal(loss.detach().cpu().numpy(), want)
    free = float(arcface_loss(x, head.weight, y, reduction="mean").detach())
    assert abs(free - float(run_c(gpu, E, W, lab, want=())["loss"].astype(np.float64).mean())) <= 1e-5 * free


# 5
def test_ignored_labels(gpu):
    B, C, D = 70, 333, 128
    E, W, lab, _ = float_case(7, B, C, D)
    ign = (lab < 0) | (lab >= C)
    assert np.any(lab == -1) and np.any(lab == C)
    full = run_c(gpu, E, W, lab, ls=0.1)
    assert np.all(full["loss"][ign] == 0) and np.all(full["dE"][ign] == 0)
    kept = run_c(gpu, E[~ign], W, lab[~ign], ls=0.1)
    rf = arcmargin_ref(E, W, lab, scale=S, margin=M, label_smoothing=0.1)
    rk = arcmargin_ref(E[~ign], W, lab[~ign], scale=S, margin=M, label_smoothing=0.1)
    assert note("ignored dW", full["dW"].astype(np.float64) - kept["dW"], rf["dW_bound"] + rk["dW_bound"] + 1e-300) <= 1
    assert note("ignored dE", full["dE"][~ign].astype(np.float64) - kept["dE"],
                rf["dE_bound"][~ign] + rk["dE_bound"] + 1e-300) <= 1


# 6
def test_repeatable(gpu, grid):
    a = grid["got"]
    b = run_c(gpu, grid["E"], grid["W"], grid["lab"], ls=0.1, want_logits=True)
    for k in ("z", "lse", "loss", "dE", "dW"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


# 7
def test_one_optimisation_step(gpu, grid):
    import torch
    from facerecognition_amd.arcmargin import ArcMarginProduct

    head = ArcMarginProduct(512, grid["W"].shape[0], scale=S, margin=M).to(gpu)
    head.load_state_dict({"weight": torch.from_numpy(grid["W"])})
    x, y = torch.from_numpy(grid["E"]).to(gpu), torch.from_numpy(grid["lab"]).to(gpu)
    opt = torch.optim.SGD([head.weight], lr=0.005)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = head.loss(x, y)
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    assert losses[5] < losses[0], losses
    acc = head.class_accuracy(x, y)
    assert 0.0 <= acc <= 1.0


def test_report():
    print("largest error / bound per quantity:", {k: round(v, 4) for k, v in sorted(worst.items())})
