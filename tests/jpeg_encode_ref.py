"""What the tests of the device JPEG encode share (test_jpeg_encode_cpu.py, test_jpeg_encode_kernels.py): the cases of the fixture
tests/golden/g26_jpeg_write.npz, and the independent oracle -- tests/jpeg_writer.py given the T.81 Annex K tables and planes padded by
the rule of libjpeg's transcoder.  Not imported by the package."""
import numpy as np

import jpeg_cases as JC
import jpeg_writer as JW

CASES = ("r64x64", "r24x40", "r17x9", "r8x8", "g24x40", "g8x8", "range_edge", "sparse", "stuffing")


def case(g, name):
    """(height, width, quant (C,8,8), Y (1,Hb,Wb,8,8), C (2,Hbc,Wbc,8,8) | None, file bytes)"""
    h, w = (int(v) for v in g[f"{name}_dim"][0])
    return h, w, g[f"{name}_quant"], g[f"{name}_Y"], g[f"{name}_C"] if f"{name}_C" in g.files else None, g[f"{name}_file"].tobytes()


def scan_start(data):
    i = data.index(b"\xff\xda")
    return i + 2 + int.from_bytes(data[i + 2:i + 4], "big")


def padded_planes(h, w, Y, Cc):
    """The planes jpeg_writer.write codes, [Hp, Wp, 64] on the MCU-padded grid, filled by the rule of libjpeg's transcoder: a block
    beyond the kept grid has zero AC and the DC of the block before it in the MCU's block order."""
    if Cc is None:
        return [Y.reshape(Y.shape[1], Y.shape[2], 64).astype(np.int64)]
    (hp, wp), _, _ = JW.padded_grids(w, h, JC.S420)
    hb, wb = Y.shape[1:3]
    P = np.zeros((hp, wp, 64), np.int64)
    P[:hb, :wb] = Y.reshape(hb, wb, 64)
    for my in range(hp // 2):
        for mx in range(wp // 2):
            order = [(2 * my, 2 * mx), (2 * my, 2 * mx + 1), (2 * my + 1, 2 * mx), (2 * my + 1, 2 * mx + 1)]
            for j in range(1, 4):
                if order[j][0] >= hb or order[j][1] >= wb:
                    P[order[j]][0] = P[order[j - 1]][0]
    return [P] + [Cc[c].reshape(Cc.shape[1], Cc.shape[2], 64).astype(np.int64) for c in (0, 1)]


def writer_file(h, w, quant, Y, Cc, restart):
    nc = 1 if Cc is None else 3
    q = [quant[min(c, 1)].reshape(64) for c in range(nc)]
    return JW.write(padded_planes(h, w, Y, Cc), q, JC.S420[:nc] if nc == 3 else [(1, 1)], JC.std3()[:nc], w, h, restart=restart,
                    split_dht=True, split_dqt=True)
