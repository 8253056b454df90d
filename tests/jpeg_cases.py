"""The JPEG files the device-decode tests share: the four of golden g1_reader.npz, Pillow-made ones (qualities, optimised
tables, restart markers) and synthetic ones that tests/jpeg_writer.py writes from chosen coefficients, for what Pillow's encoder
never emits.  A plain module, imported by name; files are made once per process."""
import collections
import functools
import io
import os

import numpy as np
from PIL import Image

import jpeg_ref as JR
import jpeg_writer as JW

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


# ---- synthetic files: coefficients chosen by the tests, written by tests/jpeg_writer.py ----------------------------------------------
# A Synth carries the file and the coefficients it was written from, cut to the kept grids: Y [Hb, Wb, 64], C [2, Hbc, Wbc, 64] or
# None, quant [components, 64], all int16 in natural order, as the host reader returns them.
Synth = collections.namedtuple("Synth", "name data Y C quant grid")

QUANT_Y = [1 + (5 * k) % 61 for k in range(64)]
QUANT_CB = [2 + (7 * k) % 97 for k in range(64)]
QUANT_CR = [255 - 3 * k for k in range(64)]
S420, S444, S422, S440 = [(2, 2), (1, 1), (1, 1)], [(1, 1)] * 3, [(2, 1), (1, 1), (1, 1)], [(1, 2), (1, 1), (1, 1)]
EOB, ZRL = 0x00, 0xF0


@functools.lru_cache(maxsize=None)
def standard_tables():
    """((DC, AC) of luma, (DC, AC) of chroma) as (bits, vals): the T.81 Annex K tables, read from a Pillow-made file, not typed in."""
    f = JR.parse(encode(noisy(16, 16, 0), quality=75))
    return tuple((JW.bits_vals(f["dc"][c]), JW.bits_vals(f["ac"][c])) for c in (0, 1))


def std3():
    luma, chroma = standard_tables()
    return [luma, chroma, chroma]


def make(name, planes, quant, sampling, tables, width, height, **kw):
    data = JW.write(planes, quant, sampling, tables, width, height, **kw)
    kept = JW.kept_grids(width, height, sampling) if len(planes) == 3 else JW.padded_grids(width, height, sampling)
    cut = [np.asarray(p)[:g[0], :g[1]].astype(np.int16) for p, g in zip(planes, kept)]
    assert len(planes) == 1 or (cut[1].shape == cut[2].shape == ((kept[0][0] + 1) // 2, (kept[0][1] + 1) // 2, 64)), "not a batch layout"
    return Synth(name, data, cut[0], np.stack(cut[1:]) if len(planes) == 3 else None, np.asarray(quant, np.int16), kept[0])


def scan_blocks(width, height, sampling, c):
    """(by, bx) of component c's blocks on its padded grid, in the order the interleaved scan codes them."""
    my, mx = JW.mcu_grid(width, height, sampling)
    h, v = sampling[c] if len(sampling) == 3 else (1, 1)
    return [(m // mx * v + y, m % mx * h + x) for m in range(my * mx) for y in range(v) for x in range(h)]


def pack(items):
    """[(zero run 0..62, value)] -> blocks [64] in natural order (DC left 0), each filled as far as the next item fits."""
    blocks, blk, k = [], np.zeros(64, np.int64), 1
    for r, val in items:
        if k + r > 63:
            blocks.append(blk)
            blk, k = np.zeros(64, np.int64), 1
        blk[JR.ZIGZAG[k + r]] = val
        k += r + 1
    if k > 1:
        blocks.append(blk)
    return blocks


def ends(s):
    """Both signs at both ends of size s: the four corners of HUFF_EXTEND."""
    return [1 << (s - 1), -(1 << (s - 1)), (1 << s) - 1, -((1 << s) - 1)]


def at(*pairs):
    blk = np.zeros(64, np.int64)
    for k, v in pairs:
        blk[JR.ZIGZAG[k]] = v
    return blk


def special_blocks():
    """[(AC content, extra ZRLs before the EOB)]: the block shapes of the sweep's list, in a fixed order; the first is all zero."""
    full = at(*[(k, (k % 3 + 1) * (-1) ** k) for k in range(1, 64)])              # all 63 AC non-zero: ends at 63 without EOB
    return [(at(), 0),                                                            # all zero (its DC difference is 0)
            (at(), 0),                                                            # DC only
            (full, 0),
            (at((17, 3), (55, -2)), 0),                                           # one ZRL, then two ZRLs, each before a coefficient
            (at((51, 5)), 0),                                                     # three ZRLs and a run of 2
            (at((63, -7)), 0),                                                    # three ZRLs, run 14, ends at 63 without EOB
            (at((5, 1)), 3),                                                      # three ZRLs followed by EOB
            (at((2, -1)), 1), (at(), 2)]                                          # one and two ZRLs followed by EOB


def dc_differences(c, full):
    """DC differences that reach categories 0..11 in both signs; full: both ends of every category in both signs."""
    d = [0]
    for s in range(1, 12):
        lo, hi = 1 << (s - 1), (1 << s) - 1
        if full:
            d += [hi, -hi, lo, -lo]
        else:
            d += [hi, -lo] if (s + c) % 2 else [lo, -hi]
            if c == 2:
                d[-2:] = [-d[-2], -d[-1]]
    return d


def fill_dc(planes, width, height, sampling, diffs, rng):
    """DC values: the running sum, in scan order over the padded grid, of diffs[c], then of small random steps."""
    for c, p in enumerate(planes):
        v = 0
        for j, (by, bx) in enumerate(scan_blocks(width, height, sampling, c)):
            v += diffs[c][j] if j < len(diffs[c]) else int(rng.integers(-2, 3))
            p[by, bx, 0] = v


def fill_padding(planes, kept, rng):
    """Blocks beyond the kept grid: all 63 AC coefficients of size 9 or 10, which a decoder has to walk and drop."""
    for p, (gh, gw) in zip(planes, kept):
        for by in range(p.shape[0]):
            for bx in range(p.shape[1]):
                if by >= gh or bx >= gw:
                    p[by, bx, 1:] = rng.integers(256, 1024, 63) * rng.choice([-1, 1], 63)


@functools.lru_cache(maxsize=None)
def sweep():
    """Three files from one set of planes: no restart interval, 1, and 4 (the MCU grid is 6 x 7).  4:2:0, standard tables,
    101 x 86 pixels: kept luma grid (11, 13), padded (12, 14).  Every component holds special_blocks() and every AC symbol (run
    0..15, size 1..10), each size with both signs at both ends of its range."""
    w, h, rng = 101, 86, np.random.default_rng(100)
    kept = JW.kept_grids(w, h, S420)
    planes = [np.zeros((gh, gw, 64), np.int64) for gh, gw in JW.padded_grids(w, h, S420)]
    extra = {}
    for c in range(3):
        items = [(r, ends(s)[(r + c) % 4]) for s in range(1, 11) for r in range(16)]
        content = special_blocks() + [(b, 0) for b in pack(items if c < 2 else items[::-1])]
        where = [(by, bx) for by, bx in scan_blocks(w, h, S420, c) if by < kept[c][0] and bx < kept[c][1]]
        assert len(content) <= len(where)
        for (by, bx), (blk, zrl) in zip(where, content):
            planes[c][by, bx] = blk
            if zrl:
                extra[(c, by, bx)] = zrl
    fill_padding(planes, kept, rng)
    fill_dc(planes, w, h, S420, [dc_differences(c, c == 0) for c in range(3)], rng)
    quant = [QUANT_Y, QUANT_CB, QUANT_CB]
    return [make(f"sweep_dri{ri}", planes, quant, S420, std3(), w, h, restart=ri, zrl_before_eob=extra) for ri in (0, 1, 4)]


AC_POOL = [EOB, ZRL] + [(r << 4) | s for r in range(6) for s in range(1, 6)]        # 32 symbols a custom AC table draws from
LONG_AC_COUNTS = [        # codes per length.  No table can hold every length 1..9 AND two codes of every length 10..16 (Kraft sum
    {1: 1, 2: 1, 3: 1, 4: 1, 5: 1, 6: 1, 7: 1, 9: 1, 10: 3, 11: 2, 12: 2, 13: 2, 14: 2, 15: 2, 16: 2},      # above 1): each leaves
    {2: 3, 3: 1, 4: 1, 5: 1, 6: 1, 8: 1, 9: 1, 10: 3, 11: 2, 12: 2, 13: 2, 14: 2, 15: 2, 16: 2},            # one short length out
    {1: 1, 3: 2, 4: 1, 5: 1, 6: 1, 7: 1, 8: 1, 9: 3, 10: 2, 11: 2, 12: 3, 13: 2, 14: 4, 15: 2, 16: 5}]
LONG_DC_LENGTHS = [[1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12], [2, 2, 2, 4, 4, 5, 6, 10, 10, 13, 16, 16], [3, 3, 3, 3, 3, 3, 3, 11, 11, 14, 15, 15]]


@functools.lru_cache(maxsize=None)
def long_tables():
    """Six distinct tables, (DC, AC) per component.  In Cb's AC table EOB has the last 16-bit code and ZRL the one before; in Cr's
    ZRL is last; the DC categories get the short codes from the other end in each component."""
    out = []
    for c in range(3):
        lengths = [n for n in sorted(LONG_AC_COUNTS[c]) for _ in range(LONG_AC_COUNTS[c][n])]
        k = len(lengths)
        syms = [AC_POOL[:k], AC_POOL[2:k] + [ZRL, EOB], AC_POOL[2:17] + [EOB] + AC_POOL[17:k - 1] + [ZRL]][c]
        cats = [list(range(12)), list(range(11, -1, -1)), list(range(6, 12)) + list(range(6))][c]
        out.append((JW.table_from_lengths(list(zip(cats, LONG_DC_LENGTHS[c]))), JW.table_from_lengths(list(zip(syms, lengths)))))
    return out


def table_items(ac, rng, rounds):
    """[(run, value)] that use every symbol of the AC table `ac` `rounds` times, in random order with random values."""
    items = []
    for _ in range(rounds):
        for sym in rng.permutation(ac[1]):
            sym = int(sym)
            if sym == EOB:
                continue                                  # every block with trailing zeros ends in one
            r, s = sym >> 4, sym & 15
            if sym == ZRL:                                # one or two ZRLs in front of a symbol the table holds
                r, s = 16 * int(rng.integers(1, 3)) + int(rng.integers(0, 6)), int(rng.integers(1, 6))
                while ((r & 15) << 4 | s) not in ac[1]:
                    r, s = 16 + int(rng.integers(0, 6)), int(rng.integers(1, 6))
            items.append((r, int(rng.integers(1 << (s - 1), 1 << s)) * int(rng.choice([-1, 1]))))
    return items


@functools.lru_cache(maxsize=None)
def long_codes():
    """One 4:2:0 file, 96 x 64 pixels (luma grid (8, 12)), behind long_tables(); three 16-bit quantisation tables; DHT and DQT one
    segment per table; an APP1 and a COM segment in front.  Every symbol of every table is coded, Cb and Cr with content of their own."""
    w, h, rng = 96, 64, np.random.default_rng(200)
    tables = long_tables()
    planes = [np.zeros((gh, gw, 64), np.int64) for gh, gw in JW.padded_grids(w, h, S420)]
    for c in range(3):
        blocks = pack(table_items(tables[c][1], rng, 3))
        where = scan_blocks(w, h, S420, c)
        assert len(blocks) < len(where)
        for (by, bx), blk in zip(where[1:], blocks):
            planes[c][by, bx] = blk
    fill_dc(planes, w, h, S420, [dc_differences(c, c == 0) for c in range(3)], rng)
    quant = [QUANT_Y, [300 + 9 * k for k in range(64)], QUANT_CR]
    return make("long_codes", planes, quant, S420, tables, w, h, dqt16=True, split_dht=True, split_dqt=True,
                app=b"Exif\0\0" + bytes(range(40)), com=b"six Huffman tables \xff\xd8\xff\xda in a comment")


def pool_planes(rng, grids, sizes=5, runs=5, most=5):
    """Sparse random blocks whose AC symbols stay inside AC_POOL (runs 0..5 or ZRL, sizes 1..5); DC random walk of small steps."""
    planes = []
    for gh, gw in grids:
        p, dc = np.zeros((gh, gw, 64), np.int64), 0
        for by in range(gh):
            for bx in range(gw):
                dc = int(np.clip(dc + int(rng.integers(-300, 301)), -1000, 1000))
                p[by, bx, 0] = dc
                k = 1
                for _ in range(int(rng.integers(0, most + 1))):
                    k += int(rng.integers(0, runs + 1)) + (16 if rng.integers(0, 8) == 0 else 0)
                    if k > 63:
                        break
                    s = int(rng.integers(1, sizes + 1))
                    p[by, bx, JR.ZIGZAG[k]] = int(rng.integers(1 << (s - 1), 1 << s)) * int(rng.choice([-1, 1]))
                    k += 1
        planes.append(p)
    return planes


def one_block_run(blk, tables):
    """The un-stuffed bytes that the block makes as a run of its own."""
    return JR.parse(JW.write([np.asarray(blk).reshape(1, 1, 64)], [QUANT_Y], [(1, 1)], [tables], 8, 8))["runs"][0]


def ones_block(rng, tail):
    """A block whose values have all bits set (2^s - 1, s = 8..10, and a DC of 2^s - 1, s = 8..11): data bytes FF are frequent.
    tail: the last one sits at coefficient 63, so the run's last byte, value bits and 1-padding, is FF."""
    blk = np.zeros(64, np.int64)
    blk[0] = (1 << int(rng.integers(8, 12))) - 1
    ks = sorted(int(k) for k in rng.choice(np.arange(1, 63), int(rng.integers(1, 9)), replace=False))
    for k in ks + ([63] if tail else []):
        blk[JR.ZIGZAG[k]] = (1 << int(rng.integers(8, 11))) - 1
    return blk


@functools.lru_cache(maxsize=None)
def stuffing():
    """Gray (5, 7) files with a restart marker per block, 0 and 2 fill bytes, and a 4:2:0 file of the same luma grid with 2.  The
    gray blocks are chosen by the run they make: the first is the one-byte run (DC difference 0, EOB), then for each residue of the
    run length mod 4 two runs that end in FF and two that do not; the last run, in front of EOI, ends in FF."""
    rng, luma = np.random.default_rng(300), standard_tables()[0]
    blocks, want = [np.zeros(64, np.int64)], [(tail, res) for tail in (True, False) for res in range(4) for _ in range(2)]
    while want:
        tail = want[0][0]
        blk = ones_block(rng, tail)
        run = one_block_run(blk, luma)
        assert (run[-1] == 0xFF) == tail
        if (tail, len(run) % 4) in want:
            want.remove((tail, len(run) % 4))
            blocks.append(blk)
    while len(blocks) < 35:
        blocks.append(ones_block(rng, len(blocks) == 34))
    plane = np.stack(blocks).reshape(5, 7, 64)
    out = [make(f"stuffing_gray_fill{f}", [plane], [QUANT_Y], [(1, 1)], [luma], 53, 37, restart=1, fill=f) for f in (0, 2)]
    w, h = 53, 37
    planes = [np.stack([ones_block(rng, bool(rng.integers(0, 2))) for _ in range(gh * gw)]).reshape(gh, gw, 64)
              for gh, gw in JW.padded_grids(w, h, S420)]
    for p in planes:                          # the DC values of neighbours in a run differ by less than 2^11
        p[..., 0] = np.minimum(p[..., 0], 1023)
    out.append(make("stuffing_420_fill2", planes, [QUANT_Y, QUANT_CB, QUANT_CR], S420, std3(), w, h, restart=1, fill=2))
    return out


@functools.lru_cache(maxsize=None)
def layouts():
    """name -> Synth, each a batch grid of its own: the sampling layouts and frame headers the grid check admits."""
    rng, luma = np.random.default_rng(400), standard_tables()[0]
    quant = [QUANT_Y, QUANT_CB, QUANT_CR]

    def colour(name, w, h, sampling, **kw):
        planes = pool_planes(rng, JW.padded_grids(w, h, sampling), sizes=8, runs=9)
        return make(name, planes, quant, sampling, std3(), w, h, **kw)

    def gray(name, w, h, byte):
        return make(name, pool_planes(rng, JW.padded_grids(w, h, [(1, 1)]), sizes=8, runs=9), [QUANT_CB], [(1, 1)], [luma], w, h,
                    gray_sampling=byte, restart=3)

    out = [colour("444_grid_1x1", 5, 7, S444), colour("422_grid_1x5", 37, 7, S422, restart=2), colour("440_grid_5x1", 7, 37, S440),
           gray("gray_0x22", 53, 37, 0x22), gray("gray_0x11", 53, 37, 0x11), gray("gray_0x41", 9, 61, 0x41),
           colour("420_ids", 53, 37, S420, comp_ids=[7, 200, 33], restart=5)]
    w, h = 83, 35                                                  # luma grid (5, 11), padded (6, 12): padding on both edges
    planes = pool_planes(rng, JW.padded_grids(w, h, S420), sizes=8, runs=9)
    fill_padding(planes, JW.kept_grids(w, h, S420), rng)
    out.append(make("420_padding", planes, quant, S420, std3(), w, h))
    return {s.name: s for s in out}


@functools.lru_cache(maxsize=None)
def many_runs():
    """241 files of luma grid (5, 7) with 8275 runs: 236 gray files with a restart marker per block (35 runs each, an odd number,
    so that runs paired in a wave straddle files), alternately behind the standard luma tables and behind long_tables()' luma pair,
    and after every 48th a 4:2:0 file with three runs, alternately behind the standard tables and all six of long_tables()."""
    rng, luma, w, h = np.random.default_rng(500), standard_tables()[0], 53, 37
    families, cfamilies = [luma, long_tables()[0]], [std3(), long_tables()]
    out = []
    for i in range(236):
        plane = pool_planes(rng, [(5, 7)], runs=3, most=3)
        out.append(make(f"many_gray{i}", plane, [QUANT_Y], [(1, 1)], [families[i % 2]], w, h, restart=1))
        if i % 48 == 47 or i == 0:
            j = len(out) - i
            planes = pool_planes(rng, JW.padded_grids(w, h, S420), runs=3, most=3)
            out.append(make(f"many_420_{j}", planes, [QUANT_Y, QUANT_CB, QUANT_CR], S420, cfamilies[j % 2], w, h, restart=5))
    return out


@functools.lru_cache(maxsize=None)
def three_scans():
    """A baseline file with one scan per component, which the device decode refuses and the host reader decodes."""
    rng, w, h = np.random.default_rng(600), 64, 64
    planes = pool_planes(rng, JW.padded_grids(w, h, S420))
    return make("three_scans", planes, [QUANT_Y, QUANT_CB, QUANT_CR], S420, std3(), w, h, scans="separate")


@functools.lru_cache(maxsize=None)
def standard_420(seed, w=64, h=64, restart=3):
    """A one-scan 4:2:0 file behind the standard tables."""
    planes = pool_planes(np.random.default_rng(seed), JW.padded_grids(w, h, S420), sizes=8, runs=9)
    return make(f"std_{w}x{h}_{seed}", planes, [QUANT_Y, QUANT_CB, QUANT_CR], S420, std3(), w, h, restart=restart)


@functools.lru_cache(maxsize=None)
def over_subscribed():
    """A 4:2:0 file of luma grid (8, 8) with the counts of the luma AC table changed to 162 codes of length 1: not a prefix code."""
    planes = pool_planes(np.random.default_rng(1), JW.padded_grids(64, 64, S420))
    data = JW.write(planes, [QUANT_Y, QUANT_CB, QUANT_CR], S420, std3(), 64, 64, split_dht=True)
    head = b"\xff\xc4\x00\xb5\x10"                       # DHT, 181 bytes, class 1 table 0
    at = data.index(head) + len(head)
    assert sum(data[at:at + 16]) == 162
    return data[:at] + bytes([162] + [0] * 15) + data[at + 16:]


def synthetic():
    """Every well-formed single-scan synthetic file but the many-runs batch: name -> Synth."""
    out = {s.name: s for s in sweep() + [long_codes()] + stuffing()}
    out.update(layouts())
    return out
