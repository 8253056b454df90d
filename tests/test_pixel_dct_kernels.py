"""The pixel <-> DCT kernels (csrc/pixel_dct.hip) at the C ABI (include/rgbnm.h: rgbnm_pixels_to_dct, rgbnm_dct_to_pixels) against
tests/pixel_ref.py, which tests/test_pixel_dct_cpu.py pins to the reference's libjpeg.  Every output lies between guard margins that
are checked untouched (uint8 outputs borrow kernel_check's int16 canary: their byte count is a multiple of 64).

Bounds.  Luma of the encoder is integer arithmetic: equal bit for bit.  Chroma is two 16-term fp32 basis products of values up to
128 * 16 = 2048 in magnitude; 32 roundings of 2^-24 relative on sums of that size bound the error of F by about 4e-3, so the kernel
may round the other way only where the fp64 quotient lies within 5e-3 of a rounding boundary: there it is within 1, elsewhere equal.
A window of +-5e-3 around the boundaries holds 1 % of uniformly spread quotients; at most 3 % of a plane may lie in it.  The decoder's
fp32 inverse DCT has the same bound on the samples these inputs give: a pixel may differ from pixel_ref only where one of its three
exact plane samples lies within 5e-3 of a k + 0.5 boundary (one unit of Cb or Cr moves a colour by up to 2: within 3), on at most
5 % of the pixels.  Pixels with a sample outside [-128, 383] (at most 2 %) are where libjpeg wraps and the kernel saturates, as
pixel_ref does: there the saturated value is asserted.

A launch is at most 2048 workgroups of four waves, one unit (MCU, or four gray blocks) per wave and pass: 8193 MCUs take the stride
and leave the last workgroup one unit."""
import numpy as np
import pytest
import torch

import kernel_check as KC
import pixel_ref as P
from rgb_no_more_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL = -1
UNITS_PER_LAUNCH = 4 * 2048
TIE = 5e-3

KINDS = {"noise": 100, "noise50": 50, "binary": 75, "zeros": 30, "ones": 95, "smooth": 100}      # input kind -> quality
SHAPES = [(1, 3, 16, 16), (3, 3, 32, 48), (2, 3, 16, 80), (5, 3, 48, 48), (2, 1, 24, 40)]
BIG = (3, 3, 16, 43696)
assert BIG[0] * (BIG[2] // 16) * (BIG[3] // 16) == UNITS_PER_LAUNCH + 1


def make(kind, shape, seed):
    r = np.random.RandomState(seed)
    B, C, H, W = shape
    if kind.startswith("noise"):
        return r.randint(0, 256, shape).astype(np.uint8)
    if kind == "binary":
        return (255 * r.randint(0, 2, shape)).astype(np.uint8)
    if kind == "zeros":
        return np.zeros(shape, np.uint8)
    if kind == "ones":
        return np.full(shape, 255, np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    img = [[127.5 + 120 * np.sin(xx / 9.0 + c + b) * np.cos(yy / 13.0 - c) for c in range(C)] for b in range(B)]
    return np.clip(np.rint(np.array(img)), 0, 255).astype(np.uint8)


def guarded_u8(n):
    assert n % 2 == 0
    g = KC.guarded(n // 2, None, torch.int16, device=DEV)
    return g, g.t.view(torch.uint8)


def run_encode(imgs, table, **over):
    """-> (rc, Y, C) through guarded outputs; over: arguments to replace (refusals)."""
    B, C, H, W = imgs.shape
    px = torch.from_numpy(np.ascontiguousarray(imgs)).to(DEV)
    gy = KC.guarded(B * (H // 8) * (W // 8) * 64, None, torch.int16, device=DEV)
    gc = KC.guarded(B * 2 * (H // 16) * (W // 16) * 64, None, torch.int16, device=DEV) if C == 3 else None
    table = np.ascontiguousarray(table, np.int16)
    a = dict(px=px.data_ptr(), B=B, C=C, H=H, W=W, q=table.ctypes.data, Y=gy.t.data_ptr(), Cc=gc.t.data_ptr() if gc else None)
    a.update(over)
    rc = L.lib().rgbnm_pixels_to_dct(a["px"], a["B"], a["C"], a["H"], a["W"], a["q"], a["Y"], a["Cc"], L.stream())
    torch.cuda.synchronize()
    ok = rc == 0
    gy.check("Y", written=ok)
    Y = gy.t.cpu().numpy().reshape(B, 1, H // 8, W // 8, 8, 8)
    Cc = None
    if gc is not None:
        gc.check("CbCr", written=ok)
        Cc = gc.t.cpu().numpy().reshape(B, 2, H // 16, W // 16, 8, 8)
    if not ok:
        assert (gy.raw == gy.canary).all() and (gc is None or (gc.raw == gc.canary).all()), "a refused call wrote"
    return rc, Y, Cc


def run_decode(coef_y, coef_c, table, **over):
    B, _, Hb, Wb = coef_y.shape[:4]
    C, H, W = (1 if coef_c is None else 3), 8 * Hb, 8 * Wb
    ty = torch.from_numpy(np.ascontiguousarray(coef_y)).to(DEV)
    tc = torch.from_numpy(np.ascontiguousarray(coef_c)).to(DEV) if coef_c is not None else None
    g, out = guarded_u8(B * C * H * W)
    table = np.ascontiguousarray(table, np.int16)
    a = dict(Y=ty.data_ptr(), Cc=L.ptr(tc), B=B, H=H, W=W, q=table.ctypes.data, px=out.data_ptr())
    a.update(over)
    rc = L.lib().rgbnm_dct_to_pixels(a["Y"], a["Cc"], a["B"], a["H"], a["W"], a["q"], a["px"], L.stream())
    torch.cuda.synchronize()
    g.check("pixels", written=False)
    if rc != 0:
        assert (g.raw == g.canary).all(), "a refused call wrote"
    return rc, out.cpu().numpy().reshape(B, C, H, W)


def check_encode(imgs, table, Y, Cc, where):
    worst = 0.0
    for b in range(imgs.shape[0]):
        e = P.encode(imgs[b], table)
        assert np.array_equal(Y[b], e["Y"]), (where, b, "luma", int(np.abs(Y[b].astype(int) - e["Y"]).max()))
        if e["C"] is None:
            continue
        window = P.tie_distance(e["Cq"]) <= TIE
        d = np.abs(Cc[b].astype(np.int32) - e["C"].astype(np.int32))
        assert not d[~window].any(), (where, b, "chroma differs away from a boundary", int(d[~window].max()))
        assert d.max() <= 1, (where, b, int(d.max()))
        worst = max(worst, float(window.mean()))
    assert worst <= 0.03, (where, worst)
    return worst


def check_decode(Y, Cc, table, got, where, ranged=True):
    """ranged: the case is one of those whose samples stay (but for 2 % of the pixels) inside libjpeg's range."""
    shares = [0.0, 0.0]
    for b in range(Y.shape[0]):
        r = P.decode(Y[b], None if Cc is None else Cc[b], table)
        window = P.near_half(r["exact"], TIE)
        inside = P.in_range(r["exact"])
        d = np.abs(got[b].astype(np.int32) - r["rgb"].astype(np.int32))
        # pixel_ref saturates too: away from a boundary the kernel equals it inside and outside the range
        assert not d[:, ~window].any(), (where, b, "differs away from a boundary", int(d[:, ~window].max()))
        assert d.max() <= 3, (where, b, int(d.max()))
        shares = [max(shares[0], float(window.mean())), max(shares[1], float(1.0 - inside.mean()))]
    assert shares[0] <= 0.05, (where, shares)
    assert not ranged or shares[1] <= 0.02, (where, shares)
    return shares


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_encode_against_the_model(shape, kind):
    imgs = make(kind, shape, 7 + sum(shape))
    table = P.quant_tables(KINDS[kind], shape[1])
    rc, Y, Cc = run_encode(imgs, table)
    assert rc == 0
    share = check_encode(imgs, table, Y, Cc, (shape, kind))
    if kind == "zeros":
        assert (Y[..., 0, 0] == P.round_away(np.array(-1024.0 / table[0, 0, 0]))).all() and not Y[..., 1:, 1:].any()
    print(f"{shape} {kind}: share of chroma quotients inside the window {share:.4f}")


def test_encode_extremes_at_the_all_ones_table():
    """All-0 and all-255 at quality 100: DC -1024 and +1016, every other coefficient 0; chroma of a gray image is 0."""
    table = P.quant_tables(100)
    for value, dc in ((0, -1024), (255, 1016)):
        rc, Y, Cc = run_encode(np.full((2, 3, 32, 16), value, np.uint8), table)
        assert rc == 0 and (Y[..., 0, 0] == dc).all() and np.count_nonzero(Y) == Y[..., 0, 0].size and not Cc.any(), value


def test_encode_one_unit_past_a_full_launch():
    imgs = make("noise", BIG, 99)
    table = P.quant_tables(90)
    rc, Y, Cc = run_encode(imgs, table)
    assert rc == 0
    check_encode(imgs, table, Y, Cc, "8193 MCUs")
    # gray: 4 * 8192 + 1 blocks -> the last unit holds one block
    gray = make("noise", (1, 1, 8, 8 * (4 * UNITS_PER_LAUNCH + 1)), 98)
    rc, Y, _ = run_encode(gray, table[:1])
    assert rc == 0
    check_encode(gray, table[:1], Y, None, "32769 gray blocks")


GOLDEN_SETS = [(n, q) for n in ("noise", "smooth", "binary", "zeros", "ones", "gray") for q in (100, 75)]


@pytest.mark.parametrize("name,q", GOLDEN_SETS, ids=[f"{n}-q{q}" for n, q in GOLDEN_SETS])
def test_decode_the_golden_coefficients(golden, name, q):
    """A batch of two: the reference's coefficients of the image and the same blocks in reversed grid order."""
    g = golden("g25_pixels.npz")
    k = f"enc_{name}_q{q}_"
    Y = np.stack([g[k + "Y"], g[k + "Y"][:, ::-1, ::-1]])
    Cc = np.stack([g[k + "C"], g[k + "C"][:, ::-1, ::-1]]) if name != "gray" else None
    rc, got = run_decode(Y, Cc, g[k + "quant"])
    assert rc == 0
    shares = check_decode(Y, Cc, g[k + "quant"], got, (name, q))
    # and the reference itself, under the CPU test's rule (the first sample is the golden's)
    d = np.abs(got[0].astype(int) - g[f"dec_{name}_q{q}"].astype(int))
    assert d.max() <= 3 and (d > 0).mean() <= 0.08, (int(d.max()), float((d > 0).mean()))
    print(f"{name} q{q}: pixels inside the window {shares[0]:.4f}, outside the range {shares[1]:.4f}")


def test_decode_the_synthetic_draws(golden):
    g = golden("g25_pixels.npz")
    for k in range(2):
        Y, Cc, table = g[f"syn_{k}_Y"], g[f"syn_{k}_C"], g[f"syn_{k}_quant"]
        Yb, Cb = np.stack([Y, -Y, Y[:, ::-1]]), np.stack([Cc, -Cc, Cc[:, ::-1]])
        rc, got = run_decode(Yb, Cb, table)
        assert rc == 0
        check_decode(Yb, Cb, table, got, ("syn", k))
        d = np.abs(got[0].astype(int) - g[f"syn_{k}_rgb"].astype(int))
        assert d.max() <= 3, int(d.max())


def test_decode_saturates_outside_the_range():
    """DC of +-400 at a table of eights (samples of 128 +- 400): many leave [-128, 383], where libjpeg's table wraps.  The kernel
    saturates, like pixel_ref; the 2 % rule of the in-range cases does not apply to this draw."""
    r = np.random.RandomState(77)
    Y = r.randint(-5, 6, (2, 1, 4, 6, 8, 8))
    Cc = r.randint(-5, 6, (2, 2, 2, 3, 8, 8))
    Y[..., 0, 0] = r.randint(-400, 401, Y.shape[:4])
    Cc[..., 0, 0] = r.randint(-400, 401, Cc.shape[:4])
    Y, Cc = Y.astype(np.int16), Cc.astype(np.int16)
    table = np.full((3, 8, 8), 8, np.int16)
    rc, got = run_decode(Y, Cc, table)
    assert rc == 0
    shares = check_decode(Y, Cc, table, got, "saturating", ranged=False)
    assert shares[1] > 0.2, shares
    assert (got == 0).any() and (got == 255).any()


def test_decode_one_unit_past_a_full_launch():
    r = np.random.RandomState(78)
    B, Hb, Wb = BIG[0], BIG[2] // 8, BIG[3] // 8
    Y = r.randint(-12, 13, (B, 1, Hb, Wb, 8, 8))
    Cc = r.randint(-12, 13, (B, 2, Hb // 2, Wb // 2, 8, 8))
    Y[..., 0, 0] = r.randint(-100, 101, Y.shape[:4])
    Cc[..., 0, 0] = r.randint(-100, 101, Cc.shape[:4])
    Y, Cc = Y.astype(np.int16), Cc.astype(np.int16)
    table = np.full((3, 8, 8), 2, np.int16)
    rc, got = run_decode(Y, Cc, table)
    assert rc == 0
    check_decode(Y, Cc, table, got, "8193 MCUs")
    Yg = Y.reshape(1, 1, 1, -1, 8, 8)[:, :, :, :4 * UNITS_PER_LAUNCH + 1]
    rc, got = run_decode(Yg, None, table)
    assert rc == 0
    check_decode(Yg, None, table, got, "32769 gray blocks")


def test_round_trip_through_both_kernels():
    """Encode at quality 100, decode: a smooth image comes back within a few units (nothing but rounding is lost)."""
    imgs = make("smooth", (2, 3, 32, 32), 5)
    table = P.quant_tables(100)
    rc, Y, Cc = run_encode(imgs, table)
    assert rc == 0
    rc, back = run_decode(Y, Cc, table)
    assert rc == 0
    assert np.abs(back.astype(int) - imgs.astype(int)).max() <= 8


def test_refusals_write_nothing():
    imgs = make("noise", (2, 3, 32, 32), 1)
    table = P.quant_tables(75)
    zero = table.copy()
    zero[1, 3, 3] = 0
    for where, over in (("C = 2", dict(C=2)), ("B = 0", dict(B=0)), ("H % 16", dict(H=24)), ("W % 16", dict(W=40)), ("H = 0", dict(H=0)),
                        ("no pixels", dict(px=None)), ("no table", dict(q=None)), ("no Y", dict(Y=None)), ("no CbCr", dict(Cc=None)),
                        ("zero table entry", dict(q=zero.ctypes.data)), ("2^31 bytes", dict(B=1 << 20, H=32, W=32)),
                        ("pixels off by one byte", dict(px=torch.zeros(8192, dtype=torch.uint8, device=DEV).data_ptr() + 1))):
        rc, _, _ = run_encode(imgs, table, **over)
        assert rc == EINVAL, where
    rc, _, _ = run_encode(imgs[:, :1], table[:1], H=28)
    assert rc == EINVAL, "gray H % 8"
    Y = np.zeros((2, 1, 4, 4, 8, 8), np.int16)
    Cc = np.zeros((2, 2, 2, 2, 8, 8), np.int16)
    for where, over in (("B = 0", dict(B=0)), ("H % 16", dict(H=24)), ("W = 0", dict(W=0)), ("no Y", dict(Y=None)),
                        ("no table", dict(q=None)), ("no pixels", dict(px=None)), ("2^31 bytes", dict(B=1 << 20))):
        rc, _ = run_decode(Y, Cc, table, **over)
        assert rc == EINVAL, where
    # one launch each, and nothing else
    (rc, _, _), names = KC.launched(lambda: run_encode(imgs, table))
    assert rc == 0 and sum("pixdct" in n for n in names) == 1, names
    (rc, _), names = KC.launched(lambda: run_decode(Y, Cc, table))
    assert rc == 0 and sum("pixdct" in n for n in names) == 1, names
