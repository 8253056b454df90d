"""A baseline JPEG writer from quantised coefficients, in plain Python: the counterpart of tests/jpeg_ref.py.

The device-decode tests' other inputs come from Pillow's encoder and reach only what it emits.  This writer puts ANY coefficients
behind ANY legal Huffman tables, so that a test decides which codes, sizes, zero runs, stuffed bytes, sampling layouts and table
assignments a file holds.  Written from ITU-T T.81 (B.2 marker segments, F.1.2 Huffman encoding, Annex C code generation); slow and
simple on purpose; not imported by the package.

    write(planes, quant, sampling, tables, width, height, restart=0, **options) -> bytes

    planes    per component an integer array [Hp, Wp, 64] in natural order on the MCU-PADDED grid (padded_grids): the blocks beyond
              the kept grid (kept_grids) are coded like any other and a decoder must drop them.  One component: the kept grid.
    quant     per component 64 values in natural order; equal tables are written once.
    sampling  per component (h, v).
    tables    per component ((bits[16], vals), (bits[16], vals)): DC then AC.  Equal tables are written once.
    restart   the restart interval in MCUs (0: none).

Options, each one thing a legal file may do: comp_ids; split_dht / split_dqt (one segment per table instead of one for all);
dqt16 (16-bit quantisation entries); com / app (payload of a COM / an APP1 segment); fill (fill bytes FF in front of every RSTn and
of EOI); gray_sampling (the sampling byte of a one-component frame, which a decoder must ignore); scans="separate" (one scan per
component, not interleaved); zrl_before_eob {(component, by, bx): n}: n ZRL symbols between the block's last coefficient and its
EOB, which no encoder writes and every decoder must accept.  A frame that needs more than two Huffman tables of a class or 16-bit
quantisation entries is written as SOF1 (extended sequential), as T.81 demands; everything else as SOF0."""
import numpy as np

from jpeg_ref import ZIGZAG


# ---- Huffman codes ------------------------------------------------------------------------------------------------------------
def prefix_code(lengths):
    """lengths: the code length (1..16) of every symbol, in the order the symbols shall get their codes within a length.  Returns
    bits[16] of the canonical code (T.81 C.2), or raises ValueError where the lengths are over-subscribed or would need the all-ones
    code of the longest length, which T.81 reserves (libjpeg refuses such a table)."""
    bits = [0] * 16
    for n in lengths:
        if not 1 <= n <= 16:
            raise ValueError(f"code length {n}")
        bits[n - 1] += 1
    check_bits(bits)
    return bits


def check_bits(bits):
    code, last = 0, 0
    for length in range(1, 17):
        code += bits[length - 1]
        if code > (1 << length):
            raise ValueError(f"over-subscribed code: {bits[length - 1]} codes of length {length} do not fit")
        if bits[length - 1]:
            last = length
        if length == last and code == (1 << length) and not any(bits[length:]):
            raise ValueError(f"the all-ones code of length {length} is reserved")
        code <<= 1
    if sum(bits) > 256 or not last:
        raise ValueError("1 to 256 codes")


def table_from_lengths(pairs):
    """pairs: [(symbol, length)].  (bits, vals) with the symbols of one length in the order given."""
    bits = prefix_code([n for _, n in pairs])
    vals = [s for n in range(1, 17) for s, m in pairs if m == n]
    if len(set(vals)) != len(vals):
        raise ValueError("a symbol twice")
    return bits, vals


def codes_of(bits, vals):
    """{symbol: (length, code)} of a DHT table; refuses what prefix_code refuses."""
    bits = [int(b) for b in bits]
    check_bits(bits)
    if len(vals) != sum(bits):
        raise ValueError("bits and vals disagree")
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[int(vals[k])] = (length, code)
            code += 1
            k += 1
        code <<= 1
    return out


def bits_vals(table):
    """(bits, vals) of a jpeg_ref.Table, e.g. one that jpeg_ref.parse took from a file."""
    order = sorted(table.codes)
    bits = [0] * 16
    for length, _ in order:
        bits[length - 1] += 1
    return bits, [table.codes[k] for k in order]


# ---- geometry (T.81 A.1.1, A.2) -----------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def kept_grids(width, height, sampling):
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    return [(_cdiv(_cdiv(height * v, vmax), 8), _cdiv(_cdiv(width * h, hmax), 8)) for h, v in sampling]


def mcu_grid(width, height, sampling):
    """(MCU rows, MCU columns) of the interleaved scan; of a one-component frame: its block grid."""
    if len(sampling) == 1:
        return _cdiv(height, 8), _cdiv(width, 8)
    hmax, vmax = max(h for h, _ in sampling), max(v for _, v in sampling)
    return _cdiv(height, 8 * vmax), _cdiv(width, 8 * hmax)


def padded_grids(width, height, sampling):
    my, mx = mcu_grid(width, height, sampling)
    if len(sampling) == 1:
        return [(my, mx)]
    return [(my * v, mx * h) for h, v in sampling]


# ---- entropy coding (T.81 F.1.2) ----------------------------------------------------------------------------------------------
class _Run:
    """The bits of one restart interval."""

    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, n):
        self.acc = (self.acc << n) | value
        self.n += n

    def bytes(self):
        """Padded with 1-bits to a whole byte (F.1.2.3); not yet stuffed."""
        pad = -self.n % 8
        return ((self.acc << pad) | ((1 << pad) - 1)).to_bytes((self.n + pad) // 8, "big")


def _magnitude(v):
    s = abs(v).bit_length()
    return s, (v if v >= 0 else v + (1 << s) - 1)


def _block(run, blk, pred, dc, ac, extra_zrl):
    """One block in natural order.  Returns its DC value, the next predictor."""
    d = int(blk[0]) - pred
    s, v = _magnitude(d)
    if s > 11:
        raise ValueError(f"DC difference {d} needs category {s}")
    run.put(dc[s][1], dc[s][0])
    run.put(v, s)
    zeros = 0
    for k in range(1, 64):
        c = int(blk[ZIGZAG[k]])
        if c == 0:
            zeros += 1
            continue
        while zeros > 15:
            run.put(ac[0xF0][1], ac[0xF0][0])
            zeros -= 16
        s, v = _magnitude(c)
        if s > 10:
            raise ValueError(f"AC coefficient {c} needs size {s}")
        run.put(ac[(zeros << 4) | s][1], ac[(zeros << 4) | s][0])
        run.put(v, s)
        zeros = 0
    if zeros:
        if extra_zrl * 16 >= zeros:
            raise ValueError("the extra ZRLs would end the block before its EOB")
        for _ in range(extra_zrl):
            run.put(ac[0xF0][1], ac[0xF0][0])
        run.put(ac[0][1], ac[0][0])
    elif extra_zrl:
        raise ValueError("extra ZRLs need trailing zeros")
    return int(blk[0])


def _scan_bytes(units, nmcu, restart, fill):
    """units(mcu) -> [(component slot, block, extra ZRLs, dc codes, ac codes)]; returns the entropy-coded segment with RSTn."""
    out = bytearray()
    nruns = _cdiv(nmcu, restart) if restart else 1
    for j in range(nruns):
        first = j * restart
        last = min(nmcu, first + restart) if restart else nmcu
        run, pred = _Run(), {}
        for mcu in range(first, last):
            for slot, blk, extra, dc, ac in units(mcu):
                pred[slot] = _block(run, blk, pred.get(slot, 0), dc, ac, extra)
        out += run.bytes().replace(b"\xff", b"\xff\x00")
        if j + 1 < nruns:
            out += b"\xff" * (fill + 1) + bytes([0xD0 + (j & 7)])
    return bytes(out)


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def _assign(items, limit, what):
    """ids of equal items: ([id per item], [distinct items])."""
    distinct, ids = [], []
    for it in items:
        if it not in distinct:
            distinct.append(it)
        ids.append(distinct.index(it))
    if len(distinct) > limit:
        raise ValueError(f"more than {limit} {what}")
    return ids, distinct


def write(planes, quant, sampling, tables, width, height, restart=0, comp_ids=None, split_dht=False, split_dqt=False, dqt16=False,
          com=None, app=None, fill=0, gray_sampling=0x11, scans="interleaved", zrl_before_eob=None):
    nc = len(planes)
    if nc not in (1, 3) or not (len(quant) == len(sampling) == len(tables) == nc):
        raise ValueError("one or three components, each with planes, quant, sampling and tables")
    if not 0 <= restart <= 65535:
        raise ValueError("restart interval")
    sampling = [(int(h), int(v)) for h, v in sampling]
    planes = [np.asarray(p) for p in planes]
    for p, g in zip(planes, padded_grids(width, height, sampling)):
        if p.shape != (g[0], g[1], 64):
            raise ValueError(f"plane of shape {p.shape}, padded grid {g}")
    comp_ids = list(comp_ids) if comp_ids else [1, 2, 3][:nc]
    extra = dict(zrl_before_eob or {})
    qids, qdistinct = _assign([tuple(int(x) for x in q) for q in quant], 4, "quantisation tables")
    if any(not 1 <= x <= (65535 if dqt16 else 255) for q in qdistinct for x in q):
        raise ValueError("quantisation value out of range")
    dcids, dcdistinct = _assign([(tuple(t[0][0]), tuple(t[0][1])) for t in tables], 4, "DC tables")
    acids, acdistinct = _assign([(tuple(t[1][0]), tuple(t[1][1])) for t in tables], 4, "AC tables")
    dccodes = [codes_of(*t) for t in dcdistinct]
    accodes = [codes_of(*t) for t in acdistinct]
    extended = dqt16 or len(dcdistinct) > 2 or len(acdistinct) > 2

    out = bytearray(b"\xff\xd8")
    if app is not None:
        out += _segment(0xE1, app)
    if com is not None:
        out += _segment(0xFE, com)
    dqt = []
    for t, q in enumerate(qdistinct):
        zz = [q[ZIGZAG[k]] for k in range(64)]
        dqt.append(bytes([(16 if dqt16 else 0) | t]) + (b"".join(x.to_bytes(2, "big") for x in zz) if dqt16 else bytes(zz)))
    out += b"".join(_segment(0xDB, d) for d in dqt) if split_dqt else _segment(0xDB, b"".join(dqt))
    sof = bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") + bytes([nc])
    for c in range(nc):
        hv = gray_sampling if nc == 1 else (sampling[c][0] << 4) | sampling[c][1]
        sof += bytes([comp_ids[c], hv, qids[c]])
    out += _segment(0xC1 if extended else 0xC0, sof)
    dht = [bytes([t]) + bytes(b) + bytes(v) for t, (b, v) in enumerate(dcdistinct)]
    dht += [bytes([16 | t]) + bytes(b) + bytes(v) for t, (b, v) in enumerate(acdistinct)]
    out += b"".join(_segment(0xC4, d) for d in dht) if split_dht else _segment(0xC4, b"".join(dht))
    if restart:
        out += _segment(0xDD, restart.to_bytes(2, "big"))

    def sos(comps):
        s = bytes([len(comps)])
        for c in comps:
            s += bytes([comp_ids[c], (dcids[c] << 4) | acids[c]])
        return _segment(0xDA, s + bytes([0, 63, 0]))

    if scans == "interleaved":
        my, mx = mcu_grid(width, height, sampling)
        layout = [(0, 0, 0)] if nc == 1 else [(c, x, y) for c in range(nc) for y in range(sampling[c][1]) for x in range(sampling[c][0])]
        hv = [(1, 1)] if nc == 1 else sampling

        def units(mcu):
            for c, x, y in layout:
                by, bx = (mcu // mx) * hv[c][1] + y, (mcu % mx) * hv[c][0] + x
                yield c, planes[c][by, bx], extra.get((c, by, bx), 0), dccodes[dcids[c]], accodes[acids[c]]

        out += sos(range(nc)) + _scan_bytes(units, my * mx, restart, fill)
    elif scans == "separate":                       # T.81 A.2.2: a scan of one component walks ITS kept grid, one block per MCU
        for c, (gh, gw) in enumerate(kept_grids(width, height, sampling)):
            def units(mcu, c=c, gw=gw):
                by, bx = mcu // gw, mcu % gw
                yield c, planes[c][by, bx], extra.get((c, by, bx), 0), dccodes[dcids[c]], accodes[acids[c]]

            out += sos([c]) + _scan_bytes(units, gh * gw, restart, fill)
    else:
        raise ValueError(scans)
    out += b"\xff" * (fill + 1) + b"\xd9"
    return bytes(out)
