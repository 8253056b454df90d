#!/usr/bin/env python
"""G26: the files the reference's dct_manip.write_coefficients (libjpeg's jpeg_write_coefficients behind it) writes from given
coefficients, through the compiled reference module (oracle.build_ref.load_ref()).  Inputs and the reference's output only:

  <case>_dim     int32 (C,2)  [[H,W],[H/2,W/2],[H/2,W/2]] as the reference's read_coefficients would give it ([[H,W]] for gray)
  <case>_quant   int16 (C,8,8)
  <case>_Y       int16 (1,Hb,Wb,8,8)            <case>_C   int16 (2,Hbc,Wbc,8,8) (absent for gray)
  <case>_file    uint8: the bytes of the file the reference wrote

Cases (4:2:0 unless gray): r64x64, r24x40, r17x9, r8x8, g24x40, g8x8 random coefficients; range_edge: AC values +-1023 and DC steps of
+-2047 between neighbours in scan order; sparse: blocks whose only non-zero coefficient sits at zig-zag position 63, 48, 32, 17 or 16
(3, 2, 1, 1, 0 ZRLs; position 63 has no EOB); stuffing: 32x32, the first seed whose scan holds at least 20 FF bytes AND ends in FF.

Survey container only (needs the reference build)."""
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import build_ref  # noqa: E402
from jpeg_ref import ZIGZAG  # noqa: E402


def grids(h, w):
    return (-(-h // 8), -(-w // 8)), (-(-h // 16), -(-w // 16))


def dim_of(h, w, gray):
    return np.array([[h, w]] if gray else [[h, w], [(h + 1) // 2, (w + 1) // 2], [(h + 1) // 2, (w + 1) // 2]], np.int32)


def random_coefficients(r, h, w, gray, amp=60, keep=0.25, dc=300):
    (hb, wb), (hc, wc) = grids(h, w)

    def plane(*lead):
        x = r.randint(-amp, amp + 1, lead + (8, 8)) * (r.rand(*lead, 8, 8) < keep)
        x[..., 0, 0] = r.randint(-dc, dc + 1, lead)
        return x.astype(np.int16)

    return plane(1, hb, wb), None if gray else plane(2, hc, wc)


def quant_of(r, gray):
    return r.randint(1, 256, (1 if gray else 3, 8, 8)).astype(np.int16)


def write(dm, tmp, dim, quant, Y, C):
    path = os.path.join(tmp, "out.jpg")
    args = [torch.from_numpy(dim.copy()), torch.from_numpy(quant.copy()), torch.from_numpy(Y.copy())]
    if C is not None:
        args.append(torch.from_numpy(C.copy()))
    dm.write_coefficients(path, *args)
    with open(path, "rb") as fh:
        return np.frombuffer(fh.read(), np.uint8).copy()


def scan_of(data):
    b = data.tobytes()
    i = b.index(b"\xff\xda")
    return b[i + 2 + int.from_bytes(b[i + 2:i + 4], "big"):-2]


def main():
    build_ref.build()
    dm = build_ref.load_ref()
    assert dm is not None, "oracle/_ref is not built"
    out = {}
    r = np.random.RandomState(2601)
    with tempfile.TemporaryDirectory() as tmp:
        def case(name, h, w, quant, Y, C):
            dim = dim_of(h, w, C is None)
            out.update({f"{name}_dim": dim, f"{name}_quant": quant, f"{name}_Y": Y, f"{name}_file": write(dm, tmp, dim, quant, Y, C)})
            if C is not None:
                out[f"{name}_C"] = C
            got = dm.read_coefficients(os.path.join(tmp, "out.jpg"))
            assert np.array_equal(got[2].numpy(), Y) and (C is None or np.array_equal(got[3].numpy(), C)), name

        for name, h, w, gray in (("r64x64", 64, 64, False), ("r24x40", 24, 40, False), ("r17x9", 17, 9, False), ("r8x8", 8, 8, False),
                                 ("g24x40", 24, 40, True), ("g8x8", 8, 8, True)):
            Y, C = random_coefficients(r, h, w, gray)
            case(name, h, w, quant_of(r, gray), Y, C)

        # range_edge, 32x32: DC -1023 / +1024 by column parity, so that neighbours in scan order differ by 2047; AC at both limits
        Y, C = random_coefficients(r, 32, 32, False, amp=1023, keep=0.5)
        for p in (Y, C):
            p[..., 0, 0] = np.where(np.arange(p.shape[2]) % 2 == 0, -1023, 1024)[None, None, :]
            p[..., 7, 7] = 1023
            p[..., 0, 1] = -1023
        case("range_edge", 32, 32, quant_of(r, False), Y, C)

        # sparse, 32x32: one coefficient per block at the listed zig-zag positions, DC zero; a few blocks entirely zero
        Y = np.zeros((1, 4, 4, 64), np.int16)
        C = np.zeros((2, 2, 2, 64), np.int16)
        for k, pos in enumerate([63, 48, 32, 17, 16, 63, 48, 32, 17, 16, 1, 63]):
            Y[0, k // 4, k % 4, ZIGZAG[pos]] = (-1) ** k * (1 + 37 * k)
        for k, pos in enumerate([63, 48, 32, 17, 16, 63]):
            C[k // 4, (k % 4) // 2, k % 2, ZIGZAG[pos]] = (-1) ** k * (3 + 101 * k)
        case("sparse", 32, 32, quant_of(r, False), Y.reshape(1, 4, 4, 8, 8), C.reshape(2, 2, 2, 8, 8))

        # stuffing, 32x32: search
        quant = quant_of(r, False)
        for seed in range(200000):
            rs = np.random.RandomState(seed)
            Y, C = random_coefficients(rs, 32, 32, False, amp=1023, keep=0.35, dc=900)
            scan = scan_of(write(dm, tmp, dim_of(32, 32, False), quant, Y, C))
            if scan.endswith(b"\xff\x00") and scan.count(b"\xff\x00") >= 20:
                print("stuffing: seed", seed, len(scan), "scan bytes,", scan.count(b"\xff\x00"), "FF")
                break
        else:
            raise SystemExit("no stuffing case found")
        case("stuffing", 32, 32, quant, Y, C)
    path = os.path.join(HERE, "g26_jpeg_write.npz")
    np.savez_compressed(path, **out)
    print("G26 done", len(out), "arrays,", os.path.getsize(path), "bytes;", sum(v.size for k, v in out.items() if k.endswith("_file")),
          "file bytes")


if __name__ == "__main__":
    main()
