"""Bit-for-bit comparison of two libfrhip builds on the same synthetic model and crops (dump), or on the
exact-score entry points over seeded float inputs (scores).

    FR_LIBFRHIP=<lib A> python tools/lib_bitcheck.py dump a.npz
    FR_LIBFRHIP=<lib B> python tools/lib_bitcheck.py dump b.npz
    python tools/lib_bitcheck.py cmp a.npz b.npz

    FR_LIBFRHIP=<lib> python tools/lib_bitcheck.py scores a.npz             every call at every shape
    FR_LIBFRHIP=<lib> FR_AB=match_tiles=5 python tools/lib_bitcheck.py scores a5.npz 70,8269,512
                                                                            the match calls at one (B, N, D)

Write the .npz files outside gpurun_out/ (they are tens of MB; gpurun copies back at most 64 MiB).
Used when a kernel is restructured without changing any product's summation order (e.g. the layer3
stage's 13-fragment layout): the embeddings and the kept stage intermediates must be identical."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def dump(path, arch="iresnet100", B=6):
    import ctypes
    import torch
    from facerecognition_amd import _native as N
    from facerecognition_amd.model import FRModel
    from facerecognition_amd.synthetic import synthetic_crops
    L = N.lib()
    out = {}
    for stage in (2, 1):
        m = FRModel.synthetic(arch)
        m.set_option(N.FR_OPT_STAGE, stage)
        m.set_option(N.FR_OPT_KEEP_INTERMEDIATES, 1)
        x = torch.from_numpy(synthetic_crops(B, 112, seed=11))
        out[f"emb_stage{stage}"] = m.embed(x).cpu().numpy()
        for t in range(L.fr_debug_tensor_count(m.handle)):
            name = L.fr_debug_tensor_name(m.handle, t).decode()
            if not name.startswith("layer3"):
                continue
            H, W, C = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            N.check(L.fr_debug_tensor_shape(m.handle, t, ctypes.byref(H), ctypes.byref(W), ctypes.byref(C)))
            buf = torch.empty((B, H.value, W.value, C.value), dtype=torch.bfloat16, device="cuda")
            N.check(L.fr_debug_copy_tensor(m.handle, t, B, buf.data_ptr(), N.stream_ptr()))
            torch.cuda.synchronize()
            out[f"s{stage}_{name}"] = buf.view(torch.int16).cpu().numpy()
        m.close()
    np.savez(path, **out)
    print(f"dumped {len(out)} arrays to {path}")


MATCH_SHAPES = [(70, 333, 512), (70, 8269, 512), (130, 1000, 128), (9, 200, 36)]


def unit_rows(rng, n, d):
    x = rng.standard_normal((n, d)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def dump_scores(path, shapes=None):
    """fr_match_topk (k = 5, 8, 16, 100), fr_match_eval with a 512-bin histogram and fr_match_range (count + fill,
    with and without `after`) at MATCH_SHAPES; without `shapes` also fr_verify_pairs with row outputs, the triplet
    mining outputs of each mode and the ArcFace forward and backward outputs at their suites' largest float shapes."""
    import torch
    from facerecognition_amd import triplet as T
    from facerecognition_amd.arcmargin import arcface_logits, arcface_loss
    from facerecognition_amd.gallery import DeviceGallery
    from facerecognition_amd.verification import verify_pairs
    out = {}

    def put(name, t):
        if t is not None:
            out[name] = t.detach().cpu().numpy()

    for B, N, D in shapes or MATCH_SHAPES:
        rng = np.random.default_rng(B + N + D)
        G = unit_rows(rng, N, D)
        true = rng.integers(0, N, B)
        P = unit_rows(rng, B, D)
        P[::2] = G[true[::2]] + 0.08 * P[::2]  # noisy matches: low ranks and high scores occur
        P /= np.linalg.norm(P, axis=1, keepdims=True)
        gal = DeviceGallery(G, dim=D)
        p = torch.from_numpy(P).to(gal.device)
        tag = f"{B}x{N}x{D}"
        for k in (5, 8, 16, 100):
            s, i = gal.search_device(p, k)
            put(f"topk{k}_s_{tag}", s)
            put(f"topk{k}_i_{tag}", i)
        r = gal.evaluate_device(p, torch.from_numpy(true.astype(np.int32)), 5, 512, (-0.25, 1.0))
        for key, v in r.items():
            put(f"eval_{key}_{tag}", v)
        thresh = float(np.median(out[f"topk16_s_{tag}"]))
        after = torch.from_numpy(rng.integers(-1, N, B).astype(np.int32))
        for name, a in (("range", None), ("range_after", after)):
            lims, s, i = gal.range_search_device(p, thresh, a)
            put(f"{name}_lims_{tag}", lims)
            put(f"{name}_s_{tag}", s)
            put(f"{name}_i_{tag}", i)
        gal.close()
    if shapes is None:
        dev = torch.device("cuda", 0)
        # verification: 300 x 64, rows not of unit length, 12 classes
        rng = np.random.default_rng(1)
        y = rng.integers(0, 12, 300).astype(np.int32)
        E = rng.standard_normal((12, 64))[y] + 1.5 * rng.standard_normal((300, 64))
        E = (E * rng.uniform(0.5, 2.0, (300, 1)) / 8.0).astype(np.float32)
        r = verify_pairs(torch.from_numpy(E).to(dev), y, thresholds=(0.0, 0.3, 0.6), hist_bins=32, rows=True)
        for key, v in r.items():
            put(f"verify_{key}", v)
        # triplet mining: 257 x 512, unit rows around 40 class centres
        rng = np.random.default_rng(7)
        y = rng.integers(0, 40, 257).astype(np.int32)
        E = unit_rows(rng, 40, 512)[y] + 0.6 * unit_rows(rng, 257, 512)
        e = torch.from_numpy((E / np.linalg.norm(E, axis=1, keepdims=True)).astype(np.float32)).to(dev)
        for mode in (0, 1, 2):  # FR_TRIPLET_SEMI_HARD, _BATCH_HARD, _FIRST
            for key, v in zip(("a", "p", "n", "semi", "lims"), T._mine(e, torch.from_numpy(y), mode, 0.2)):
                put(f"triplet{mode}_{key}", v)
        # ArcFace: (70, 4167, 512), the fused loss and the dense logits, each with dE and dW
        rng = np.random.default_rng(5)
        B, C, D = 70, 4167, 512
        W = rng.standard_normal((C, D)).astype(np.float32)
        lab = rng.integers(0, C, B)
        E = (W[lab] / 20 + 0.7 * rng.standard_normal((B, D))).astype(np.float32)
        lab_t = torch.from_numpy(lab)
        for name, f in (("loss", lambda e, w: arcface_loss(e, w, lab_t, label_smoothing=0.1, reduction="none")),
                        ("logits", lambda e, w: arcface_logits(e, w, lab_t))):
            e = torch.from_numpy(E).to(dev).requires_grad_(True)
            w = torch.from_numpy(W).to(dev).requires_grad_(True)
            z = f(e, w)
            g = torch.from_numpy(np.random.default_rng(9).standard_normal(tuple(z.shape)).astype(np.float32)).to(dev)
            z.backward(g)
            put(f"arc_{name}", z)
            put(f"arc_{name}_dE", e.grad)
            put(f"arc_{name}_dW", w.grad)
    torch.cuda.synchronize()
    np.savez(path, **out)
    print(f"dumped {len(out)} arrays to {path}")


def cmp(a, b):
    A, Bz = np.load(a), np.load(b)
    bad = [k for k in A.files if k not in Bz.files or A[k].dtype != Bz[k].dtype or A[k].shape != Bz[k].shape
           or A[k].tobytes() != Bz[k].tobytes()]
    print(f"{len(A.files) - len(bad)}/{len(A.files)} identical" + (f"; differ: {bad[:10]}" if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif sys.argv[1] == "scores":
        dump_scores(sys.argv[2], [tuple(int(v) for v in a.split(",")) for a in sys.argv[3:]] or None)
    else:
        sys.exit(cmp(sys.argv[2], sys.argv[3]))
