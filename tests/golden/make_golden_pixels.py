#!/usr/bin/env python
"""G25: the reference's dct_manip.quantize_at_quality / decode_coeff (libjpeg behind them) on small images, through the compiled
reference module (oracle.build_ref.load_ref()).  Inputs and the reference's outputs only:

  img_<name>                          uint8 (C,H,W): noise 3x32x48, smooth 3x64x64, a 0/255 image 3x32x32, all-0 and all-255
                                      3x16x16, gray 1x24x40, and photo 3x224x224 (smooth; quality 100 only)
  enc_<name>_q<Q>_{quant,Y,C}         quantize_at_quality(img, Q), Q in 30 / 75 / 95 / 100 (no C for gray)
  dec_<name>_q<Q>                     decode_coeff of those coefficients, Q in 100 / 75 (not for photo)
  syn_<k>_{Y,C,quant,rgb}             two synthetic draws at quant 2: DC uniform in +-100 (64x64) and +-150 (32x16), AC an eighth

Survey container only (needs the reference build)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import build_ref  # noqa: E402

QUALITIES = (30, 75, 95, 100)


def images():
    r = np.random.RandomState(2501)
    yy, xx = np.mgrid[0:64, 0:64]
    smooth = np.stack([127.5 + 120 * np.sin(xx / 9.0 + c) * np.cos(yy / 13.0 - c) for c in range(3)])
    yy, xx = np.mgrid[0:224, 0:224]
    photo = np.stack([128 + 90 * np.sin(xx / (17.0 + 5 * c)) * np.cos(yy / (23.0 - 4 * c)) + 20 * np.sin((xx + 2 * yy) / 19.0)
                      for c in range(3)])
    return {"noise": r.randint(0, 256, (3, 32, 48)).astype(np.uint8),
            "smooth": np.clip(np.rint(smooth), 0, 255).astype(np.uint8),
            "binary": (255 * r.randint(0, 2, (3, 32, 32))).astype(np.uint8),
            "zeros": np.zeros((3, 16, 16), np.uint8),
            "ones": np.full((3, 16, 16), 255, np.uint8),
            "gray": r.randint(0, 256, (1, 24, 40)).astype(np.uint8),
            "photo": np.clip(np.rint(photo), 0, 255).astype(np.uint8)}


def dim_of(H, W):
    return torch.tensor([[H, W], [H // 2, W // 2], [H // 2, W // 2]], dtype=torch.int32)


def main():
    build_ref.build()
    dm = build_ref.load_ref()
    assert dm is not None, "oracle/_ref is not built"
    out = {}
    for name, img in images().items():
        out[f"img_{name}"] = img
        H, W = img.shape[1:]
        for q in QUALITIES if name != "photo" else (100,):
            dim, quant, Y, C = dm.quantize_at_quality(torch.from_numpy(img.copy()), q)
            assert dim[0].tolist() == [H, W]
            out[f"enc_{name}_q{q}_quant"] = quant.numpy()
            out[f"enc_{name}_q{q}_Y"] = Y.numpy()
            if C is not None:
                out[f"enc_{name}_q{q}_C"] = C.numpy()
            if q in (100, 75) and name != "photo":
                out[f"dec_{name}_q{q}"] = dm.decode_coeff(dim, quant, Y, C).numpy()
    r = np.random.RandomState(2502)
    for k, (amp, H, W) in enumerate([(100, 64, 64), (150, 32, 16)]):
        Y = r.randint(-amp // 8, amp // 8 + 1, (1, H // 8, W // 8, 8, 8))
        C = r.randint(-amp // 8, amp // 8 + 1, (2, H // 16, W // 16, 8, 8))
        Y[..., 0, 0] = r.randint(-amp, amp + 1, Y.shape[:3])
        C[..., 0, 0] = r.randint(-amp, amp + 1, C.shape[:3])
        Y, C = Y.astype(np.int16), C.astype(np.int16)
        quant = np.full((3, 8, 8), 2, np.int16)
        rgb = dm.decode_coeff(dim_of(H, W), torch.from_numpy(quant), torch.from_numpy(Y), torch.from_numpy(C)).numpy()
        out.update({f"syn_{k}_Y": Y, f"syn_{k}_C": C, f"syn_{k}_quant": quant, f"syn_{k}_rgb": rgb})
    path = os.path.join(HERE, "g25_pixels.npz")
    np.savez_compressed(path, **out)
    print("G25 done", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
