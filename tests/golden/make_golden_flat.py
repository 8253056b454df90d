#!/usr/bin/env python
"""G24: AutoContrast / AutoSaturation / Equalize on FLAT images (every DC of the plane set equal) through the reference's own
dispatcher (utils/custom_transforms.py:_apply_op_dct, with its per-op clamp).  The reference keeps the DCs only when
min = max = 0; a flat non-zero image divides 0 by 0 in fp32 and what the int16 cast makes of the NaN is whatever the
reference's CPU kernels do -- recorded here, because that is what decides what the oracle and the HIP kernel must give.
Small grids (4 x 4 luma, 2 x 2 chroma): the ops reduce over the DC set and treat every block alike.  Survey container only."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402
from rgb_no_more_amd import detfill  # noqa: E402

FLAT_DCS = [0, 1, -1, 100, -333, 1016, -1024]


def main():
    mg._stub_modules()
    sys.path.insert(0, mg.REF)
    import utils.custom_transforms as ctrans
    Y = detfill.integers((1, 4, 4, 8, 8), 241, -1024, 1016, np.int16)
    C = detfill.integers((2, 2, 2, 8, 8), 242, -1024, 1016, np.int16)
    out = {"Y": Y, "C": C, "flat_dcs": np.array(FLAT_DCS, np.int16)}
    k = 0
    for name in ("AutoContrast", "AutoSaturation", "Equalize"):
        for dy in FLAT_DCS:
            for dc in (0, dy):                       # chroma flat at zero and at the luma's value
                y, c = Y.copy(), C.copy()
                y[..., 0, 0] = dy
                c[..., 0, 0] = dc
                oy, oc = ctrans._apply_op_dct([torch.from_numpy(y.copy()), torch.from_numpy(c.copy())], name, 0.0, None,
                                              [None, None], [None, None])
                out[f"case{k}_name"] = np.array(name)
                out[f"case{k}_dcs"] = np.array([dy, dc], np.int16)
                out[f"case{k}_Y"] = oy.numpy()
                out[f"case{k}_C"] = oc.numpy()
                k += 1
    out["ncases"] = np.int64(k)
    np.savez_compressed(os.path.join(HERE, "g24_flat.npz"), **out)
    print("G24 done", k)


if __name__ == "__main__":
    main()
