"""CPU checks of tests/fused_ref.py, before a GPU sees it: the float64 restatements of the six fused groups
reproduce the fp32 oracle, the selection weights have the properties that make test_gpu_fused_exact.py's
equality exact, and slice_stats sees the localized faults that the whole-tensor Frobenius bar of
test_gpu_chain.py does not."""
import functools

import numpy as np
import pytest
import torch

from tests import fused_ref as FR
from facerecognition_amd import weights as Wt
from facerecognition_amd.synthetic import synthetic_crops

SEED = {"resnet50_arcface": 29, "irv1_facenet": 13}
DT = {"bf16": torch.bfloat16, "f16": torch.float16}


@functools.lru_cache(maxsize=None)
def state_dict(arch, which):
    return Wt.synth_state_dict(arch) if which == "synth" else FR.selection_state_dict(arch, 0)


@functools.lru_cache(maxsize=None)
def folded(arch, which):
    return Wt.fold_state_dict(arch, state_dict(arch, which))


@functools.lru_cache(maxsize=None)
def oracle_tensors(arch, which):
    """(u8 crops, {module name: NHWC f32 output}) of one oracle forward on 3 crops."""
    from oracle import models as M
    u8 = synthetic_crops(3, Wt.INPUT_SIZE[arch], seed=SEED[arch])
    om = M.build_model(arch, state_dict(arch, which))
    names = {n for a, _, i, o in FR.KINDS.values() if a == arch for n in ((i,) if i else ()) + o}
    got, hooks = {}, []
    for n in sorted(names):
        hooks.append(om.get_submodule(n).register_forward_hook(
            lambda _m, _i, o, n=n: got.__setitem__(n, o.detach().permute(0, 2, 3, 1).contiguous().clone())))
    M.embed(om, arch, u8)
    for h in hooks:
        h.remove()
    return u8, got


def group_input(kind, which):
    arch, _, tin, _ = FR.KINDS[kind]
    u8, got = oracle_tensors(arch, which)
    return u8 if tin is None else got[tin]


def rounded(x, dtype):
    return x.to(dtype).to(torch.float64)


# ---- the restatements are the network: unrounded, each group reproduces the oracle's hooked output from its hooked
# input to fp32 noise.  Measured max|diff| / max|out| (synth / selection): stem_r50 5.9e-7 / 5.9e-7, bneck28 5.1e-7 /
# 8.3e-8, chain_r50 3.4e-7 / 9.4e-8, stem160 8.7e-7 / 8.7e-7, chain35 1.6e-7 / 1.4e-7, chain17 2.1e-7 / 1.9e-7 (1.4e-6
# absolute on a maximum of 6.7) -- none above 1e-6.
@pytest.mark.parametrize("which", ["synth", "selection"])
@pytest.mark.parametrize("kind", sorted(FR.KINDS))
def test_restatement_matches_oracle(kind, which):
    arch, _, _, touts = FR.KINDS[kind]
    _, got = oracle_tensors(arch, which)
    out = FR.RESTATE[kind](group_input(kind, which), folded(arch, which), None)
    assert sorted(out) == sorted(touts)
    for n in touts:
        want = got[n].double()
        err = (out[n] - want).abs().max().item()
        print(f"{kind} {which} {n}: max|diff| {err:.2e} on max|out| {want.abs().max().item():.3g} "
              f"(rel {err / want.abs().max().item():.1e})")
        assert out[n].shape == want.shape
        assert err <= 1e-5 * want.abs().max().item(), f"{kind} {n}: restatement differs from the oracle by {err:.3e}"


# ---- selection weights
@pytest.mark.parametrize("arch", ["resnet50_arcface", "irv1_facenet"])
def test_selection_state_dict_properties(arch):
    sd, base, fw = state_dict(arch, "selection"), state_dict(arch, "synth"), folded(arch, "selection")
    convs = FR.selection_convs(arch)
    touched = set()
    for key, bn, role, blk in convs:
        touched.add(key)
        touched |= {bn + s for s in (".weight", ".bias", ".running_mean", ".running_var")} if bn else {key[:-6] + "bias"}
        name = key[:-len(".conv.weight")] if key.endswith(".conv.weight") else key[:-len(".weight")]
        name = name.replace(".downsample.0", ".downsample")
        w, b = fw[name + ".w"], fw[name + ".b"]  # [Cout, kh, kw, Cin], [Cout]
        cout, kh, kw, cin = w.shape
        want = 0.25 if role == "res" else 1.0
        for dt in DT.values():  # the 16-bit weights are exactly 0 and one `want` per output channel
            wq = torch.from_numpy(w).to(dt).double().numpy().reshape(cout, -1)
            assert set(np.unique(wq)) == {0.0, want}, f"{name}: 16-bit weights {np.unique(wq)}"
            assert np.all((wq != 0).sum(axis=1) == 1), f"{name}: not one nonzero weight per output channel"
        b64 = b.astype(np.float64)
        if role == "plain":
            assert np.all(b64 * 16 == np.round(b64 * 16)) and np.all(np.abs(b64) <= 0.5), f"{name}: bias {b64[:8]}"
            assert np.unique(b64).size > 8, f"{name}: the biases do not vary"
        else:
            assert np.all(b64 == 0), f"{name}: a bias on a conv that adds a residual / carries the downsample"
        # coverage: every tap of a spatial conv, every 32-channel K-step of a 1x1 conv
        o, r, s, c = np.nonzero(w)
        if kh * kw > 1:
            assert set(r * kw + s) == set(range(kh * kw)), f"{name}: taps {sorted(set(r * kw + s))} of {kh * kw}"
        else:
            assert set(c // 32) == set(range(cin // 32)), f"{name}: K-steps {sorted(set(c // 32))} of {cin // 32}"
    # the Block35 residual conv: 0.25 / 0.17 folds to exactly 2^-2 (Block17: 2.5)
    if arch == "irv1_facenet":
        assert np.unique(sd["model.repeat_1.0.conv2d.weight"]).tolist() == [0.0, np.float32(0.25 / 0.17)]
        assert np.unique(sd["model.repeat_2.0.conv2d.weight"]).tolist() == [0.0, 2.5]
        for n in ("model.repeat_1.0.conv2d.w", "model.repeat_2.0.conv2d.w"):
            for dt in DT.values():
                assert torch.from_numpy(fw[n]).to(dt).double().unique().tolist() == [0.0, 0.25]
    # nothing else changed (the stems fold 1/255 and a hi/lo split, which is not exact: they stay synthetic)
    assert set(sd) == set(base)
    for k in base:
        if k not in touched:
            assert np.array_equal(sd[k], base[k]), f"{k} changed"
    assert len(touched) > 20 and all(k in sd for k in touched)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("kind", ["bneck28", "chain_r50", "chain35", "chain17"])
def test_selection_not_vacuous(kind, dtype):
    """The rounded restatement with selection weights, on the oracle-captured input: at least half of every output's
    elements are nonzero, and moving one conv's taps by one position changes the result."""
    arch, _, _, touts = FR.KINDS[kind]
    fw, dt = folded(arch, "selection"), DT[dtype]
    x = rounded(group_input(kind, "selection"), dt)
    out = FR.RESTATE[kind](x, fw, dt)
    for n in touts:
        frac = (out[n] != 0).double().mean().item()
        print(f"{kind} {dtype} {n}: nonzero {frac:.3f}, max {out[n].max().item():.4g}")
        assert frac >= 0.5, f"{kind} {n}: only {frac:.3f} of the elements are nonzero"
        assert torch.isfinite(out[n]).all() and torch.equal(out[n], rounded(out[n], dt))
    conv = {"bneck28": "backbone.layer1.2.conv2", "chain_r50": "backbone.layer3.5.conv2",
            "chain35": "model.repeat_1.4.branch2.2", "chain17": "model.repeat_2.9.branch1.2"}[kind]
    w = fw[conv + ".w"]
    moved = dict(fw)
    moved[conv + ".w"] = np.roll(w.reshape(w.shape[0], -1, w.shape[3]), 1, axis=1).reshape(w.shape)
    out2 = FR.RESTATE[kind](x, moved, dt)
    n = touts[-1]
    assert not torch.equal(out2[n], out[n]), f"{kind}: shifting the taps of {conv} is invisible"


# ---- the detectors: two legitimate f32 summation orders of the ten Block17 against the float64 reference, and
# two planted faults.  Measured (bf16 / f16), elem, pixel, channel statistic:
#   order 1          4.5e-2, 6.5e-3, 8.3e-3   /   7.5e-3, 7.8e-4, 1.3e-3
#   order 2          6.0e-2, 6.3e-3, 9.7e-3   /   8.3e-3, 7.7e-4, 1.4e-3      (ratios 1.33, 1.04, 1.17 / 1.10, 1.02, 1.13)
#   fragment x 1.10  channel statistic 8.7e-2 / 8.7e-2;  Frobenius against order 2: 6.2e-3 (bf16), 5.0e-3 (f16)
#   column x 1.05    pixel statistic 6.8e-2 / 6.8e-2
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_slice_stats_see_localized_faults(dtype):
    dt = DT[dtype]
    fw = folded("irv1_facenet", "synth")
    x = rounded(group_input("chain17", "synth"), dt)
    n = "model.repeat_2.9"
    ref = FR.chain17(x, fw, dt)[n]
    a = FR.chain17(x, fw, dt, compute=torch.float32)[n]
    b = FR.chain17(x, fw, dt, compute=torch.float32, perm_seed=1)[n]
    sa, sb = FR.slice_stats(a, ref), FR.slice_stats(b, ref)
    print(f"{dtype}: order 1 {sa}, order 2 {sb}")
    assert not torch.equal(a, b), "the two evaluations are the same order"
    for va, vb in zip(sa, sb):
        assert 0 < max(va, vb) <= 2 * min(va, vb), f"two legitimate orders differ by more than 2x: {sa} vs {sb}"
    clean = [max(va, vb) for va, vb in zip(sa, sb)]
    frag = a.clone()
    frag[1, :, :, 32:48] *= 1.10  # one 16-channel n-fragment of one image
    sf = FR.slice_stats(frag, ref)
    fro = ((frag - b).norm() / b.norm()).item()
    col = a.clone()
    col[1, :, 0, :] *= 1.05  # one border column of one image
    sc = FR.slice_stats(col, ref)
    print(f"{dtype}: fragment {sf} (Frobenius vs order 2 {fro:.2e}), column {sc}")
    assert sf[2] > 2 * clean[2], f"fragment fault: channel statistic {sf[2]:.3e} vs clean {clean[2]:.3e}"
    assert sc[1] > 2 * clean[1], f"column fault: pixel statistic {sc[1]:.3e} vs clean {clean[1]:.3e}"
    if dtype == "bf16":  # the record of the gap: test_gpu_chain.py's bf16 bar is rel < 6e-3
        assert fro <= 1.1 * 6e-3, f"fragment fault: Frobenius {fro:.3e}"
