#!/usr/bin/env python3
"""Write tests/golden/augment_golden.npz: a few tiny images, op lists and what Pillow (and torch, for the blur and the
normalisation) make of them, so the restatement and the device can be held to Pillow's results where Pillow is not
installed.  Data only: images u8 [N][12][16][3], ops i32 [N][16], args f64 [N][16][8], out_u8, out_f32, and the
versions that produced it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import PIL
    import torch

    from facerecognition_amd import augment as A
    from tests import augment_pil as P
    from tests import augment_ref as R

    H, W = 12, 16
    c = (W * 0.5, H * 0.5)
    progs = [
        [],
        [(R.FLIP_H,)],
        [(R.AFFINE_NEAREST, *A.rotation_matrix(17.0, W, H))],
        [(R.AFFINE_NEAREST, *A.inverse_affine_matrix(c, -9.0, (1, -2), 0.9, (5.0, 0.0)))],
        [(R.PERSPECTIVE_BILINEAR, 1.05, 0.04, -0.5, -0.03, 0.95, 0.8, 2e-3, -3e-3)],
        [(R.CROP_RESIZE, 2, 3, 8, 11)],
        [(R.BRIGHTNESS, 1.4)], [(R.CONTRAST, 0.6)], [(R.SATURATION, 1.3)], [(R.HUE, -0.07)], [(R.GRAYSCALE,)],
        [(R.GAUSS_BLUR, 3, *A.gaussian_kernel1d(3, 1.0))],
        [(R.CROP_RESIZE, 1, 1, 10, 14), (R.FLIP_H,), (R.AFFINE_NEAREST, *A.rotation_matrix(-8.0, W, H)), (R.HUE, 0.1),
         (R.CONTRAST, 1.2), (R.BRIGHTNESS, 0.8), (R.SATURATION, 0.7), (R.ERASE, 0, 10, 5, 6)],
    ]
    rng = np.random.default_rng(0)
    images = np.stack([P.rand_image(rng, H, W) for _ in progs])
    ops = np.zeros((len(progs), R.MAX_OPS), np.int32)
    args = np.zeros((len(progs), R.MAX_OPS, R.NARGS), np.float64)
    for b, prog in enumerate(progs):
        for k, (op, *v) in enumerate(prog):
            ops[b, k] = op
            args[b, k, :len(v)] = v
    outs = [P.run_program(images[b], ops[b], args[b]) for b in range(len(progs))]
    path = os.path.join(ROOT, "tests", "golden", "augment_golden.npz")
    np.savez_compressed(path, images=images, ops=ops, args=args, out_u8=np.stack([o[0] for o in outs]),
                        out_f32=np.stack([o[1] for o in outs]),
                        versions=np.array([f"Pillow {PIL.__version__}", f"torch {torch.__version__}"]))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
