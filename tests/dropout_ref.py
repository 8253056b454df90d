"""numpy restatement of the dropout mask contract of include/rgbnm.h (csrc/philox.h): Philox4x32-10 and keep . scale.

A plain module, imported by name from the tests (like kernel_check.py).  Element (row, col) of site `site` of block `block` is kept
when word (col & 3) of Philox4x32-10(counter = (col >> 2, row, 4 block + site, 0), key = (seed low 32 bits, seed high 32 bits)) is
>= thr = llround(p 2^32); kept elements are multiplied by the fp32 scale 1 / (1 - p), dropped ones are 0.
"""
import math

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised over numpy arrays of counters (any broadcastable shapes); k0, k1 Python ints.  Returns four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _LO for x in (c0, c1, c2, c3)]
    c = np.broadcast_arrays(*c)
    c0, c1, c2, c3 = (x.copy() for x in c)
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0 = M0 * c0
        p1 = M1 * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & _LO
        hi1, lo1 = p1 >> np.uint64(32), p1 & _LO
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0 = (k0 + W0) & 0xFFFFFFFF
        k1 = (k1 + W1) & 0xFFFFFFFF
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def threshold(p):
    """(thr, scale) of the contract for the fp32 value of p (the C entries take p as a float)."""
    pf = float(np.float32(p))
    thr = min(int(math.floor(pf * 4294967296.0 + 0.5)), 0xFFFFFFFF)
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(pf))
    return thr, scale


def seed_key(seed):
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s & 0xFFFFFFFF, s >> 32


def words(seed, site, block, M, N):
    """[M, N] uint32 mask words."""
    k0, k1 = seed_key(seed)
    rows = np.arange(M, dtype=np.uint64)[:, None]
    c4 = (np.arange((N + 3) // 4, dtype=np.uint64))[None, :]
    w = philox4x32_10(c4, rows, np.uint64(4 * block + site), np.uint64(0), k0, k1)
    out = np.stack(w, axis=-1).reshape(M, -1)          # column 4 j + q = word q of counter j
    return out[:, :N]


def keep(seed, p, site, block, M, N):
    """[M, N] bool."""
    thr, _ = threshold(p)
    return words(seed, site, block, M, N) >= np.uint32(thr) if thr else np.ones((M, N), dtype=bool)


def factor(seed, p, site, block, M, N):
    """[M, N] float32 keep . scale (0 or scale)."""
    _, scale = threshold(p)
    return np.where(keep(seed, p, site, block, M, N), scale, np.float32(0)).astype(np.float32)
