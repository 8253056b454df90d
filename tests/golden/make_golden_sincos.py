"""G10: the reference's sin-cos table (models/plainvit.py SinCosEmbedding) at E = 192 and E = 384, generated under MKL's conditional
numerical reproducibility mode COMPATIBLE.

torch's CPU exp / sin / cos run on MKL's vector math, whose code path -- and so the last bit of a result -- follows the CPU: in the
default mode one of the 96 frequencies of E = 384 rounds differently on an AVX-512 CPU than on others, and every table entry that
uses it follows.  In COMPATIBLE mode every x86 CPU gives the same bits, so tests/test_oracle_golden.py evaluates the oracle in that
mode as well.  MKL reads the mode once, when it starts: it is set here before torch is imported.

Run:  python tests/golden/make_golden_sincos.py   (needs /root/reference; same stubs as make_golden.py)
"""
import os

os.environ["MKL_CBWR"] = "COMPATIBLE"

import sys  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402


def main():
    MG._stub_modules()
    sys.path.insert(0, MG.REF)
    import models.plainvit as pvit
    sc = pvit.SinCosEmbedding()
    t192 = sc(torch.zeros((1, 14, 14, 192))).reshape(196, 192).numpy()
    t384 = sc(torch.zeros((1, 14, 14, 384))).reshape(196, 384).numpy()
    np.savez_compressed(os.path.join(HERE, "g10_sincos.npz"), t192=t192, t384_rows=t384[[0, 1, 13, 14, 97, 195]])


if __name__ == "__main__":
    main()
