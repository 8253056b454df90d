"""numpy restatement of RGB pixels <-> quantised DCT coefficients as libjpeg (IJG 9, 4:2:0) computes them behind the reference's
dct_manip.quantize_at_quality / decode_coeff: the yardstick of csrc/pixel_dct.hip.  A plain module, imported by name from the tests.

- Luma of the encoder is integer arithmetic and equals libjpeg bit for bit (fixed-point RGB -> YCbCr, the "islow" forward DCT with
  13-bit constants and 2 pass-1 bits, the quantiser sign(c) (|c| + 4 q) / (8 q)).
- Chroma of the encoder is the low 8 x 8 of the 16 x 16-point DCT of each 16 x 16 square of integer Cb / Cr samples, in fp64, divided by
  the table entry and rounded half away from zero; libjpeg's fixed-point 16-point routine is within 0.08 of the exact value, so the
  two differ by at most 1, and only next to a rounding boundary.
- The decoder is the fp64 inverse DCT (8 x 8 for luma, 8 -> 16 for chroma), floor(x + 0.5) clamped to [0, 255] per plane, then
  libjpeg's fixed-point YCbCr -> RGB, clamped.  libjpeg's integer IDCT differs from it by a few units, and its range-limit table
  wraps where a sample leaves [-128, 383]; this model saturates.

Both directions also return the exact fp64 values before rounding, so that a test can tell a near-tie from an error.
"""
import numpy as np

LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64).reshape(8, 8)
CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                   47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64).reshape(8, 8)


def FIX(x, bits=16):
    return int(x * (1 << bits) + 0.5)


def quant_tables(quality, channels=3, baseline=True):
    """int16 (channels, 8, 8): the Annex-K tables scaled as jpeg_set_quality does (chroma twice for three channels)."""
    q = min(max(int(quality), 1), 100)
    s = 5000 // q if q < 50 else 200 - 2 * q
    t = [np.clip((b * s + 50) // 100, 1, 255 if baseline else 32767) for b in (LUMA, CHROMA, CHROMA)]
    return np.stack(t[:channels]).astype(np.int16)


def rgb_to_ycc(img):
    """uint8 (3,H,W) -> int64 Y, Cb, Cr planes (jccolor.c)."""
    R, G, B = (img[i].astype(np.int64) for i in range(3))
    off = (128 << 16) + 32767
    Y = (FIX(0.299) * R + FIX(0.587) * G + FIX(0.114) * B + 32768) >> 16
    Cb = (-FIX(0.168735892) * R - FIX(0.331264108) * G + FIX(0.5) * B + off) >> 16
    Cr = (FIX(0.5) * R - FIX(0.418687589) * G - FIX(0.081312411) * B + off) >> 16
    return Y, Cb, Cr


def _pass(d, first):
    """One 8-point pass of jfdctint.c's jpeg_fdct_islow along the LAST axis of d (int64 [..., 8])."""
    F = lambda x: FIX(x, 13)     # noqa: E731
    sh = 11 if first else 15
    d = [d[..., i] for i in range(8)]
    t0, t1, t2, t3 = d[0] + d[7], d[1] + d[6], d[2] + d[5], d[3] + d[4]
    t10, t12, t11, t13 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[0] - d[7], d[1] - d[6], d[2] - d[5], d[3] - d[4]
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        t10 = t10 + 2
        o[0], o[4] = (t10 + t11) >> 2, (t10 - t11) >> 2
    z1 = (t12 + t13) * F(0.541196100) + (1 << (sh - 1))
    o[2] = (z1 + t12 * F(0.765366865)) >> sh
    o[6] = (z1 - t13 * F(1.847759065)) >> sh
    t12, t13 = t0 + t2, t1 + t3
    z1 = (t12 + t13) * F(1.175875602) + (1 << (sh - 1))
    t12 = t12 * -F(0.390180644) + z1
    t13 = t13 * -F(1.961570560) + z1
    z1 = (t0 + t3) * -F(0.899976223)
    t0 = t0 * F(1.501321110) + z1 + t12
    t3 = t3 * F(0.298631336) + z1 + t13
    z1 = (t1 + t2) * -F(2.562915447)
    t1 = t1 * F(3.072711026) + z1 + t13
    t2 = t2 * F(2.053119869) + z1 + t12
    o[1], o[3], o[5], o[7] = t0 >> sh, t1 >> sh, t2 >> sh, t3 >> sh
    return np.stack(o, -1)


def _blocks(plane, n):
    """(H,W) -> (H/n, W/n, n, n)."""
    H, W = plane.shape
    return plane.reshape(H // n, n, W // n, n).transpose(0, 2, 1, 3)


def _unblocks(b):
    hb, wb, n, _ = b.shape
    return b.transpose(0, 2, 1, 3).reshape(hb * n, wb * n)


def luma_encode(Yplane, q):
    """int64 (H,W) samples, table (8,8) -> int16 (H/8,W/8,8,8), bit for bit libjpeg's."""
    b = _blocks(Yplane - 128, 8)
    b = _pass(b, True)                                           # rows
    b = _pass(b.swapaxes(-1, -2), False).swapaxes(-1, -2)        # columns
    q8 = 8 * q.astype(np.int64)
    mag = (np.abs(b) + (q8 >> 1)) // q8
    return (np.sign(b) * mag).astype(np.int16)


def basis(N, div):
    """[u][m] = c(u) / div cos((2m+1) u pi / (2N)), u < 8."""
    u, m = np.arange(8)[:, None], np.arange(N)[None, :]
    c = np.where(u == 0, np.sqrt(0.5), 1.0)
    return c / div * np.cos((2 * m + 1) * u * np.pi / (2 * N))


def chroma_encode(plane, q):
    """int64 (H,W) samples, table (8,8) -> (int16 (H/16,W/16,8,8), the exact quotient F / q as fp64 of the same shape)."""
    fb = basis(16, 4.0)
    x = _blocks(plane - 128, 16).astype(np.float64)
    F = np.einsum("um,hwmn,vn->hwuv", fb, x, fb)
    quo = F / q.astype(np.float64)
    return round_away(quo).astype(np.int16), quo


def round_away(x):
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def tie_distance(x):
    """Distance of x from the nearest rounding boundary k + 0.5."""
    return np.abs(np.abs(x) - np.floor(np.abs(x)) - 0.5)


def encode(img, quant):
    """uint8 (C,H,W), int16 (C,8,8) -> dict(Y int16 (1,Hb,Wb,8,8), C int16 (2,Hb/2,Wb/2,8,8) or None, Cq: exact chroma quotients)."""
    img = np.asarray(img)
    if img.shape[0] == 1:
        return {"Y": luma_encode(img[0].astype(np.int64), quant[0])[None], "C": None, "Cq": None}
    Y, Cb, Cr = rgb_to_ycc(img)
    cb, cbq = chroma_encode(Cb, quant[1])
    cr, crq = chroma_encode(Cr, quant[1])
    return {"Y": luma_encode(Y, quant[0])[None], "C": np.stack([cb, cr]), "Cq": np.stack([cbq, crq])}


def decode(Y, C, quant):
    """int16 Y (1,Hb,Wb,8,8), C (2,Hc,Wc,8,8) or None, table (C,8,8) -> dict(rgb uint8 (3 or 1,H,W), exact: fp64 (3 or 1,H,W), the
    plane samples Y / Cb / Cr at full size before rounding)."""
    b8 = basis(8, 2.0)
    y = np.einsum("um,hwuv,vn->hwmn", b8, Y[0].astype(np.float64) * quant[0].astype(np.float64), b8) + 128.0
    exact = [_unblocks(y)]
    if C is not None:
        b16 = basis(16, 2.0)
        for p in range(2):
            c = np.einsum("um,hwuv,vn->hwmn", b16, C[p].astype(np.float64) * quant[1].astype(np.float64), b16) + 128.0
            exact.append(_unblocks(c))
    exact = np.stack(exact)
    s = np.clip(np.floor(exact + 0.5), 0, 255).astype(np.int64)
    if C is None:
        return {"rgb": s.astype(np.uint8), "exact": exact}
    yy, cb, cr = s[0], s[1] - 128, s[2] - 128
    R = yy + ((FIX(1.402) * cr + 32768) >> 16)
    G = yy + ((-FIX(0.344136286) * cb - FIX(0.714136286) * cr + 32768) >> 16)
    B = yy + ((FIX(1.772) * cb + 32768) >> 16)
    return {"rgb": np.clip(np.stack([R, G, B]), 0, 255).astype(np.uint8), "exact": exact}


def in_range(exact):
    """(H,W) mask: the exact samples of every plane at the pixel lie in [-128, 383] (where libjpeg's range table does not wrap)."""
    return ((exact >= -128) & (exact <= 383)).all(0)


def near_half(exact, eps):
    """(H,W) mask: some plane's exact sample at the pixel is within eps of a k + 0.5 boundary."""
    return (np.abs(exact - np.floor(exact) - 0.5) <= eps).any(0)
