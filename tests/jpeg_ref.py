"""Baseline JPEG entropy decoding restated in plain Python: the yardstick of the device decode's host half.

Two entries.  parse(data) goes from file bytes to runs and canonical Huffman tables on its own -- marker parse, un-stuffing, split at
the restart markers.  decode_plan(plan, i) walks the buffers a dct_manip.JpegBatchPlan holds for file i -- stream, run records, image
record, look-up tables -- and so shows that the plan carries everything a decoder needs.  Both end in the same per-run Huffman walk
(ITU-T T.81 F.2.2; libjpeg jdhuff.c decode_mcu) and return (Y [Hb, Wb, 64], CbCr [2, Hbc, Wbc, 64] or None) as int16 numpy arrays in
natural order, blocks of the MCU padding dropped.  Slow and simple on purpose; not imported by the package."""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
          42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


class Table:
    """A Huffman table as {(length, code): symbol}."""

    def __init__(self, codes):
        self.codes = codes

    @classmethod
    def from_dht(cls, bits, vals):
        codes, code, k = {}, 0, 0
        for length in range(1, 17):
            for _ in range(bits[length - 1]):
                codes[(length, code)] = vals[k]
                code += 1
                k += 1
            code <<= 1
        return cls(codes)

    @classmethod
    def from_plan(cls, row):
        """row: the 1440 bytes of a rgbnm_jpeg_hufftab -- look uint16[512], maxcode int32[18], valoff int32[18], vals uint8[256]."""
        row = np.ascontiguousarray(row)
        look = row[:1024].view(np.uint16)
        maxcode = row[1024:1096].view(np.int32)
        valoff = row[1096:1168].view(np.int32)
        vals = row[1168:1424]
        codes = {}
        for i in range(512):                       # first level: every 9-bit pattern whose prefix is a code of length <= 9
            length = int(look[i]) >> 8
            if length:
                codes[(length, i >> (9 - length))] = int(look[i]) & 255
        index = len(codes)                         # values are stored in code order: the next value belongs to the next code
        for length in range(10, 17):               # longer codes: the canonical ranges [index - valoff, maxcode]
            if maxcode[length] >= 0:
                for c in range(index - int(valoff[length]), int(maxcode[length]) + 1):
                    codes[(length, c)] = int(vals[c + int(valoff[length])])
                    index += 1
        return cls(codes)


class Bits:
    def __init__(self, data):
        self.data, self.pos = data, 0

    def bit(self):
        byte = self.data[self.pos >> 3] if (self.pos >> 3) < len(self.data) else 0
        b = (byte >> (7 - (self.pos & 7))) & 1
        self.pos += 1
        return b

    def take(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if (length, code) in table.codes:
                return table.codes[(length, code)]
        raise ValueError("unassigned Huffman code")


def extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def walk_run(data, nmcu, mcu_blocks, dc_tables, ac_tables):
    """One run: `data` un-stuffed bytes, nmcu MCUs of blocks [component, ...].  Returns a list of (component, block[64] natural
    order) in scan order.  The DC predictors start at zero."""
    br = Bits(data)
    pred = [0, 0, 0]
    out = []
    for _ in range(nmcu):
        for comp in mcu_blocks:
            blk = [0] * 64
            s = br.symbol(dc_tables[comp])
            pred[comp] += extend(br.take(s), s)
            blk[0] = pred[comp]
            k = 1
            while k < 64:
                sym = br.symbol(ac_tables[comp])
                r, s = sym >> 4, sym & 15
                if s:
                    k += r
                    blk[ZIGZAG[k]] = extend(br.take(s), s)
                    k += 1
                elif r == 15:
                    k += 16
                else:
                    break
            out.append((comp, blk))
    assert 8 * len(data) - br.pos < 8, "more than the padding bits left over"
    return out


def place(blocks_per_run, ncomp, mcus_x, layout, hs, vs, grids):
    """Scan-order blocks -> planes.  blocks_per_run: [(mcu0, [(comp, blk), ...])]; layout: [(comp, dx, dy)] of one MCU; grids: kept
    (H, W) per component."""
    planes = [np.zeros((grids[c][0], grids[c][1], 64), np.int16) for c in range(ncomp)]
    for mcu0, blocks in blocks_per_run:
        for j, (comp, blk) in enumerate(blocks):
            mcu, b = mcu0 + j // len(layout), j % len(layout)
            c, dx, dy = layout[b]
            assert c == comp
            by, bx = (mcu // mcus_x) * vs[c] + dy, (mcu % mcus_x) * hs[c] + dx
            if by < grids[c][0] and bx < grids[c][1]:
                planes[c][by, bx] = np.asarray(blk, np.int64).astype(np.int16)
    return planes


def parse(data):
    """File bytes -> dict(ncomp, width, height, hs, vs, restart, runs [bytes], had_stuffing, dc, ac [Table per component], quant)."""
    assert data[:2] == b"\xff\xd8"
    pos, qt, ht, info = 2, {}, {}, {"restart": 0}
    while True:
        assert data[pos] == 0xFF
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        length = (data[pos] << 8) | data[pos + 1]
        seg = data[pos + 2:pos + length]
        pos += length
        if m == 0xDB:
            o = 0
            while o < len(seg):
                pq, t = seg[o] >> 4, seg[o] & 15
                vals = [(seg[o + 1 + 2 * k] << 8) | seg[o + 2 + 2 * k] if pq else seg[o + 1 + k] for k in range(64)]
                nat = [0] * 64
                for k in range(64):
                    nat[ZIGZAG[k]] = vals[k]
                qt[t] = nat
                o += 1 + 64 * (pq + 1)
        elif m == 0xC4:
            o = 0
            while o < len(seg):
                tc, t = seg[o] >> 4, seg[o] & 15
                bits = list(seg[o + 1:o + 17])
                n = sum(bits)
                ht[(tc, t)] = Table.from_dht(bits, list(seg[o + 17:o + 17 + n]))
                o += 17 + n
        elif m == 0xDD:
            info["restart"] = (seg[0] << 8) | seg[1]
        elif m in (0xC0, 0xC1):
            assert seg[0] == 8
            info["height"], info["width"], nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            info["ncomp"] = nc
            info["hs"] = [seg[7 + 3 * c] >> 4 for c in range(nc)]
            info["vs"] = [seg[7 + 3 * c] & 15 for c in range(nc)]
            info["quant"] = [seg[8 + 3 * c] for c in range(nc)]
        elif m == 0xDA:
            ns = seg[0]
            assert ns == info["ncomp"]
            info["dc"] = [ht[(0, seg[2 + 2 * c] >> 4)] for c in range(ns)]
            info["ac"] = [ht[(1, seg[2 + 2 * c] & 15)] for c in range(ns)]
            break
        else:
            assert not 0xC2 <= m <= 0xCF, "not a baseline Huffman file"
    info["quant"] = [qt[t] for t in info["quant"]]
    runs, cur, stuffed = [], bytearray(), False
    while True:
        b = data[pos]
        pos += 1
        if b != 0xFF:
            cur.append(b)
            continue
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        if m == 0:
            cur.append(0xFF)
            stuffed = True
        elif 0xD0 <= m <= 0xD7:
            assert m == 0xD0 + (len(runs) & 7), "restart marker out of sequence"
            runs.append(bytes(cur))
            cur = bytearray()
        else:
            assert m == 0xD9, "one scan expected"
            runs.append(bytes(cur))
            break
    info["runs"], info["had_stuffing"] = runs, stuffed
    return info


def _geometry(ncomp, width, height, hs, vs):
    if ncomp == 1:
        gw, gh = -(-width // 8), -(-height // 8)
        return gw, gh, [(0, 0, 0)], [1], [1], [(gh, gw)]
    hmax, vmax = max(hs), max(vs)
    grids = [(-(-(-(-height * vs[c] // vmax)) // 8), -(-(-(-width * hs[c] // hmax)) // 8)) for c in range(ncomp)]
    layout = [(c, x, y) for c in range(ncomp) for y in range(vs[c]) for x in range(hs[c])]
    return -(-width // (8 * hmax)), -(-height // (8 * vmax)), layout, hs, vs, grids


def decode_file(data):
    """(Y, CbCr | None, quant [ncomp][64]) of a baseline file, all in this module."""
    f = parse(data)
    mcus_x, mcus_y, layout, hs, vs, grids = _geometry(f["ncomp"], f["width"], f["height"], f["hs"], f["vs"])
    nmcu, ri = mcus_x * mcus_y, f["restart"]
    assert len(f["runs"]) == (-(-nmcu // ri) if ri else 1), "run count"
    per_run = []
    for j, run in enumerate(f["runs"]):
        mcu0 = j * ri
        n = min(ri, nmcu - mcu0) if ri else nmcu
        per_run.append((mcu0, walk_run(run, n, [c for c, _, _ in layout], f["dc"], f["ac"])))
    planes = place(per_run, f["ncomp"], mcus_x, layout, hs, vs, grids)
    return planes[0], (np.stack(planes[1:]) if f["ncomp"] == 3 else None), np.asarray(f["quant"], np.int16)


def decode_plan(plan, i):
    """(Y, CbCr | None) of file i from the plan's OWN buffers (dct_manip.JpegBatchPlan)."""
    im = plan.images[i].numpy()
    ncomp, mcus_x, mcus_y, nblk, status = (int(v) for v in im[:5])
    assert status == 0, (status, plan.messages[i])
    dc_tab, ac_tab, hs, vs = (im[5 + 3 * j:8 + 3 * j].tolist() for j in range(4))
    layout = [(int(im[17 + b]), int(im[27 + b]), int(im[37 + b])) for b in range(nblk)]
    nruns = int(im[47])
    tabs = {}

    def table(t):
        if t not in tabs:
            tabs[t] = Table.from_plan(plan.tables[t].numpy())
        return tabs[t]

    dc = [table(dc_tab[c]) for c in range(ncomp)]
    ac = [table(ac_tab[c]) for c in range(ncomp)]
    runs = plan.runs[:plan.nruns].numpy()
    mine = [r for r in runs if int(r[2]) == i and int(r[4]) > 0]
    assert len(mine) == nruns
    stream = plan.stream.numpy()
    per_run, covered = [], 0
    for r in mine:
        off, nbytes, mcu0, nmcu = int(r[0]) & 0xFFFFFFFF, int(r[1]) & 0xFFFFFFFF, int(r[3]), int(r[4])
        assert off % 4 == 0 and off + ((nbytes + 3) & ~3) + 4 <= plan.stream_bytes, "a run must be aligned and tail-padded"
        assert mcu0 == covered
        covered += nmcu
        per_run.append((mcu0, walk_run(bytes(stream[off:off + nbytes]), nmcu, [c for c, _, _ in layout], dc, ac)))
    assert covered == mcus_x * mcus_y
    hb, wb = plan.grid
    grids = [(hb, wb), ((hb + 1) // 2, (wb + 1) // 2), ((hb + 1) // 2, (wb + 1) // 2)]
    planes = place(per_run, ncomp, mcus_x, layout, hs, vs, grids)
    return planes[0], (np.stack(planes[1:]) if ncomp == 3 else None)
