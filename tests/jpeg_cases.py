"""The JPEG files the device-decode tests share: the four of golden g1_reader.npz and Pillow-made ones (qualities, optimised
tables, restart markers).  A plain module, imported by name; files are made once per process."""
import functools
import io
import os

import numpy as np
from PIL import Image

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g1_reader.npz")


def noisy(h, w, seed, gray=False):
    """Smooth colour patches plus noise, like the loader tests' files: long and short codes, zero runs and EOBs all occur."""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, (max(2, h // 16), max(2, w // 16), 3), dtype=np.uint8)
    img = np.asarray(Image.fromarray(small).resize((w, h), Image.BICUBIC), dtype=np.float32)
    img = np.clip(img + rng.normal(0, 8, img.shape), 0, 255).astype(np.uint8)
    return img[..., 0] if gray else img


def encode(img, **kw):
    kw.setdefault("subsampling", "4:2:0")
    if img.ndim == 2:
        kw.pop("subsampling")
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="JPEG", **kw)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def g1_files():
    g = np.load(GOLDEN)
    return {name: g[name + "_jpeg"].tobytes() for name in ("c64x64", "c48x80", "g40x56", "c37x53")}


@functools.lru_cache(maxsize=None)
def pillow_files():
    """name -> bytes.  72 x 104 pixels = 5 x 7 MCUs: intervals of 2 and 3 MCUs leave a short last run, 1 and 2 give more than eight
    runs (RSTn wraps from D7 to D0), partial MCUs on both edges."""
    a = noisy(72, 104, 1)
    out = {f"q{q}": encode(a, quality=q) for q in (30, 75, 100)}
    out["optimize"] = encode(a, quality=75, optimize=True)
    for k in (1, 2, 3):
        out[f"rst_blocks{k}"] = encode(a, quality=85, restart_marker_blocks=k)
    out["rst_rows1"] = encode(a, quality=85, restart_marker_rows=1)
    out["gray_rst"] = encode(noisy(72, 104, 2, gray=True), quality=85, restart_marker_blocks=4)
    return out


def small_batch():
    """Same-grid (8 x 8 luma blocks) files with different table sets and run counts: five colour files with a restart marker per
    MCU (16 runs each = 80), one with optimised tables (1 run), one without markers (1 run): 82 runs, not a multiple of 64."""
    files = [encode(noisy(64, 64, 10 + i), quality=60 + 8 * i, restart_marker_blocks=1) for i in range(5)]
    files.append(encode(noisy(64, 64, 20), quality=80, optimize=True))
    files.append(encode(noisy(64, 64, 21), quality=92))
    return files
