"""The yardstick of the pixel <-> DCT kernels (tests/pixel_ref.py) pinned to the reference's libjpeg-backed quantize_at_quality /
decode_coeff through the golden tests/golden/g25_pixels.npz, and the Python surface's refusals.  No GPU.

What libjpeg (IJG 9) and the model may differ by, measured when the golden was made (make_golden_pixels.py):
- luma and both tables: nothing.
- chroma: libjpeg's fixed-point 16-point DCT is within 0.088 of the exact value F (before the division by the table), so the
  two roundings differ by at most 1, only where F lies within 0.1 of a rounding boundary, on at most 8 % of a plane (6.6 % for noise
  at quality 100).
- decode: libjpeg's integer IDCT against fp64: within 3 on every value and at most 8 % of values differing (5.4 % measured),
  wherever the exact samples of all three planes lie in [-128, 383]; outside libjpeg wraps.  At most 2 % of pixels may be outside.
"""
import ctypes

import numpy as np
import pytest
import torch

import pixel_ref as P
import rgb_no_more_amd as rg
from rgb_no_more_amd import lib as L

IMAGES = ["noise", "smooth", "binary", "zeros", "ones", "gray"]
QUALITIES = [30, 75, 95, 100]


def check_encode(got_Y, got_C, gold_Y, gold_C, Cq, table, where):
    """The rules above for one image's coefficients; Cq: pixel_ref's exact chroma quotients."""
    assert np.array_equal(got_Y, gold_Y), (where, "luma")
    if gold_C is None:
        assert got_C is None
        return 0.0
    d = np.abs(got_C.astype(np.int32) - gold_C.astype(np.int32))
    assert d.max() <= 1, (where, int(d.max()))
    dist_F = P.tie_distance(Cq) * table.astype(np.float64)           # distance from the boundary in units of F
    assert not (d > 0).any() or dist_F[d > 0].max() <= 0.1, (where, float(dist_F[d > 0].max()))
    share = max(float((d[p] > 0).mean()) for p in range(2))
    assert share <= 0.08, (where, share)
    return share


def check_decode(got, gold, exact, where):
    m = P.in_range(exact)
    assert 1.0 - m.mean() <= 0.02, (where, float(1.0 - m.mean()))
    d = np.abs(got.astype(np.int32) - gold.astype(np.int32))[:, m]
    assert d.max() <= 3, (where, int(d.max()))
    assert (d > 0).mean() <= 0.08, (where, float((d > 0).mean()))
    return float((d > 0).mean())


@pytest.mark.parametrize("name", IMAGES + ["photo"])
def test_encoder_model_against_the_reference(golden, name):
    g = golden("g25_pixels.npz")
    img = g[f"img_{name}"]
    for q in QUALITIES if name != "photo" else [100]:
        k = f"enc_{name}_q{q}_"
        table = P.quant_tables(q, img.shape[0])
        assert np.array_equal(table, g[k + "quant"]), (name, q)
        assert np.array_equal(rg.dct_manip.quality_tables(q, img.shape[0]).numpy(), g[k + "quant"]), (name, q)
        e = P.encode(img, table)
        share = check_encode(e["Y"], e["C"], g[k + "Y"], g[k + "C"] if img.shape[0] == 3 else None, e["Cq"], table[-1], (name, q))
        print(f"{name} q{q}: chroma share differing {share:.4f}")


@pytest.mark.parametrize("name", IMAGES)
def test_decoder_model_against_the_reference(golden, name):
    g = golden("g25_pixels.npz")
    gray = g[f"img_{name}"].shape[0] == 1
    for q in (100, 75):
        k = f"enc_{name}_q{q}_"
        r = P.decode(g[k + "Y"], None if gray else g[k + "C"], g[k + "quant"])
        share = check_decode(r["rgb"], g[f"dec_{name}_q{q}"], r["exact"], (name, q))
        print(f"{name} q{q}: decoded share differing {share:.4f}")


@pytest.mark.parametrize("k", [0, 1])
def test_decoder_model_on_the_synthetic_draws(golden, k):
    g = golden("g25_pixels.npz")
    r = P.decode(g[f"syn_{k}_Y"], g[f"syn_{k}_C"], g[f"syn_{k}_quant"])
    check_decode(r["rgb"], g[f"syn_{k}_rgb"], r["exact"], ("syn", k))


def test_tables_beyond_the_goldens():
    assert np.array_equal(rg.dct_manip.quality_tables(100).numpy(), np.ones((3, 8, 8), np.int16))
    for q in (1, 10, 49, 50, 51, 99):
        for ch in (1, 3):
            assert np.array_equal(rg.dct_manip.quality_tables(q, ch).numpy(), P.quant_tables(q, ch)), (q, ch)
    assert rg.dct_manip.quality_tables(1).max() == 255 and rg.dct_manip.quality_tables(1, baseline=False).max() > 255
    assert np.array_equal(rg.dct_manip.quality_tables(1, baseline=False).numpy(), P.quant_tables(1, baseline=False))
    for bad in (0, 101, -1):
        with pytest.raises(L.RgbnmError, match="quality"):
            rg.dct_manip.quality_tables(bad)


def test_surface_and_refusals():
    dm, ct = rg.dct_manip, rg.custom_transforms
    for mod, name in ((dm, "quantize_at_quality"), (dm, "decode_coeff"), (ct, "rgb_to_dct"), (ct, "ycbcr_to_rgb")):
        assert callable(getattr(mod, name)), name
    dll = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(dll, "rgbnm_pixels_to_dct") and hasattr(dll, "rgbnm_dct_to_pixels")
    assert "rgbnm_pixels_to_dct" in L.PROTOTYPES and "rgbnm_dct_to_pixels" in L.PROTOTYPES
    px = torch.zeros(3, 32, 32, dtype=torch.uint8)
    Y, C = torch.zeros(1, 4, 4, 8, 8, dtype=torch.int16), torch.zeros(2, 2, 2, 8, 8, dtype=torch.int16)
    ones = torch.ones(3, 8, 8, dtype=torch.int16)
    # no CPU fallback
    with pytest.raises(L.RgbnmError, match="no CPU fallback"):
        dm.quantize_at_quality(px, 75)
    with pytest.raises(L.RgbnmError, match="no CPU fallback"):
        dm.quantize_at_quality(px[None, :1], 75)
    with pytest.raises(L.RgbnmError, match="no CPU fallback"):
        dm.decode_coeff(None, ones, Y, C)
    with pytest.raises(L.RgbnmError, match="no CPU fallback"):
        ct.rgb_to_dct()(px)
    with pytest.raises(L.RgbnmError, match="no CPU fallback"):
        ct.ycbcr_to_rgb()((Y.float(), C.float()))
    # sizes: 16 for colour, 8 for gray
    for shape in ((3, 24, 32), (3, 32, 40), (3, 8, 16), (1, 12, 16), (1, 16, 20), (2, 3, 30, 32)):
        with pytest.raises(L.RgbnmError, match="multiples of"):
            dm.quantize_at_quality(torch.zeros(shape, dtype=torch.uint8), 75)
    with pytest.raises(L.RgbnmError, match="channels"):
        dm.quantize_at_quality(torch.zeros(2, 16, 16, dtype=torch.uint8), 75)
    with pytest.raises(L.RgbnmError, match=r"\(C,H,W\)"):
        dm.quantize_at_quality(torch.zeros(16, 16, dtype=torch.uint8), 75)
    # dtypes
    for dt in (torch.float32, torch.int16, torch.int8):
        with pytest.raises(L.RgbnmError, match="uint8"):
            dm.quantize_at_quality(px.to(dt), 75)
    with pytest.raises(L.RgbnmError, match="int16"):
        dm.decode_coeff(None, ones, Y.float(), C.float())
    with pytest.raises(L.RgbnmError, match="CbCr must be"):
        dm.decode_coeff(None, ones, Y, torch.zeros(2, 4, 4, 8, 8, dtype=torch.int16))
    with pytest.raises(L.RgbnmError, match="dim says"):
        dm.decode_coeff(torch.tensor([[30, 32], [15, 16], [15, 16]], dtype=torch.int32), ones, Y, C)
    with pytest.raises(L.RgbnmError, match="quant must be"):
        dm.decode_coeff(None, ones.float(), Y, C)
    with pytest.raises(AssertionError, match="float32"):
        ct.ycbcr_to_rgb()((Y, C))
    with pytest.raises(AssertionError, match="float32"):
        ct.ycbcr_to_rgb()((Y.float(), C.double()))
    from PIL import Image
    with pytest.raises(TypeError, match="convert a PIL image"):
        ct.rgb_to_dct()(Image.new("RGB", (32, 32)))
