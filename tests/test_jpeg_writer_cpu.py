"""The synthetic JPEG files of tests/jpeg_cases.py, without a GPU.  tests/jpeg_writer.py writes them from chosen coefficients, so
three things are checked here before the device tests (tests/test_jpeg_decode_symbols.py) rely on them:

  - the writer: the host libjpeg reader (dm.read_coefficients_bytes), a decoder this project did not write, returns the source
    coefficients and quantisation tables bit for bit; so does the plain-Python jpeg_ref.decode_file;
  - the host half of the device decode: prepare_jpeg_batch accepts every file, and its plan's own buffers decode to the source;
  - the coverage the cases were made for, as assertions: an instrumented jpeg_ref.Bits records every (table, length, code, symbol,
    value bits) it decodes, and the lists of the cases' docstrings are asserted on that record.

Seeded defects: a copy of the Python walk with one change at a time.  Every defect changes the output of some synthetic file.  The
files made by Pillow (golden, jpeg_cases.pillow_files and small_batch) cannot show "Cr reads Cb's tables", because Pillow gives
both the same pair; that gap is asserted, and what they catch of the other defects is printed (run with -s): with the Pillow this was written
against they also miss the off-by-one value index at code length 13 (the standard tables have no such code), and catch the
others; without small_batch, lengths 14 and 15 are missed as well."""
import functools

import numpy as np
import pytest

import jpeg_cases as JC
import jpeg_ref as JR
import jpeg_writer as JW
from rgb_no_more_amd import dct_manip as dm

CASES = JC.synthetic()
ALL_AC = {JC.EOB, JC.ZRL} | {(r << 4) | s for r in range(16) for s in range(1, 11)}


def host(data):
    _, quant, Y, CbCr = dm.read_coefficients_bytes(data)
    hb, wb = Y.shape[1:3]
    return (Y.numpy().reshape(hb, wb, 64), None if CbCr is None else CbCr.numpy().reshape(2, CbCr.shape[1], CbCr.shape[2], 64),
            quant.numpy().reshape(-1, 64), (hb, wb))


def same(got_y, got_c, s):
    return np.array_equal(got_y, s.Y) and (got_c is None) == (s.C is None) and (got_c is None or np.array_equal(got_c, s.C))


def check_plan(plan, i, s):
    assert int(plan.status[i]) == 0, (s.name, plan.messages[i])
    assert same(*JR.decode_plan(plan, i), s), s.name
    q = plan.quant[i].numpy().reshape(3, 64)
    assert np.array_equal(q[:len(s.quant)], s.quant) and (q[len(s.quant):] == 1).all()


def check_source(s):
    Yh, Ch, Qh, grid = host(s.data)
    assert grid == tuple(s.grid) and Yh.dtype == s.Y.dtype == np.int16
    assert same(Yh, Ch, s), f"{s.name}: libjpeg does not read what the writer was given"
    assert np.array_equal(Qh, s.quant)
    Y, C, Q = JR.decode_file(s.data)
    assert same(Y, C, s) and np.array_equal(Q, s.quant)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_decoder_returns_the_source_coefficients(name):
    s = CASES[name]
    check_source(s)
    plan = dm.prepare_jpeg_batch([s.data], grid=tuple(s.grid))
    assert plan.nbad == 0, plan.messages
    check_plan(plan, 0, s)
    assert plan.nruns == len(JR.parse(s.data)["runs"])


def test_the_layouts_named_as_accepted_are_accepted():
    """prepare refuses none of 4:4:4 at (1, 1), 4:2:2 at (1, 5), 4:4:0 at (5, 1), gray with a sampling byte of 0x22, other component
    ids; the image records hold the block layouts the walk then meets for the first time."""
    lay = JC.layouts()
    want = {"444_grid_1x1": (3, [1, 1, 1], [1, 1, 1]), "422_grid_1x5": (4, [2, 1, 1], [1, 1, 1]), "440_grid_5x1": (4, [1, 1, 1], [2, 1, 1]),
            "420_ids": (6, [2, 1, 1], [2, 1, 1]), "gray_0x22": (1, [1, 0, 0], [1, 0, 0]), "gray_0x41": (1, [1, 0, 0], [1, 0, 0])}
    for name, (nblk, hs, vs) in want.items():
        plan = dm.prepare_jpeg_batch([lay[name].data], grid=tuple(lay[name].grid))
        im = plan.images[0].tolist()
        assert im[4] == 0 and im[3] == nblk and im[11:14] == hs and im[14:17] == vs, (name, im[:17])
    assert lay["gray_0x22"].data != lay["gray_0x11"].data
    assert lay["420_padding"].grid == (5, 11) and JW.padded_grids(83, 35, JC.S420)[0] == (6, 12)


def test_many_runs_batch():
    files = JC.many_runs()
    for s in files:
        check_source(s)
    plan = dm.prepare_jpeg_batch([s.data for s in files], grid=(5, 7), threads=4)
    assert plan.nbad == 0 and plan.nruns > 8192
    for i, s in enumerate(files):
        check_plan(plan, i, s)
    nruns, dc = plan.images[:plan.n, 47].tolist(), plan.images[:plan.n, 5:11].tolist()
    assert all(n % 2 == 1 for n in nruns), "an odd number of runs per file, so that lane pairs straddle files"
    assert all(a != b for a, b in zip(dc, dc[1:])), "neighbouring files name different table sets"
    assert sum(1 for s in files if s.C is not None) == 5 and plan.ntables == 10        # 4 standard and 6 custom tables


# ---- what the files make a decoder do --------------------------------------------------------------------------------------
class Recording(JR.Bits):
    """jpeg_ref.Bits that notes [table, length, code, symbol, value bits] of every symbol it decodes."""
    log = None

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            if (length, code) in table.codes:
                Recording.log.append([table.label, length, code, table.codes[(length, code)], None])
                return table.codes[(length, code)]
        raise ValueError("unassigned Huffman code")

    def take(self, n):
        v = super().take(n)
        Recording.log[-1][4] = v
        return v


@functools.lru_cache(maxsize=None)
def record(data):
    """The decode of a file by jpeg_ref's walk: (tables {("dc" | "ac", component): Table}, per run a list of the symbols)."""
    f = JR.parse(data)
    mcus_x, mcus_y, layout, _, _, _ = JR._geometry(f["ncomp"], f["width"], f["height"], f["hs"], f["vs"])
    tables = {}
    for kind in ("dc", "ac"):
        for c in range(f["ncomp"]):                       # one object per component, also where two components share a table
            tables[(kind, c)] = JR.Table(f[kind][c].codes)
            tables[(kind, c)].label = (kind, c)
    nmcu, ri, runs = mcus_x * mcus_y, f["restart"], []
    keep, JR.Bits = JR.Bits, Recording
    try:
        for j, run in enumerate(f["runs"]):
            Recording.log = []
            n = min(ri, nmcu - j * ri) if ri else nmcu
            JR.walk_run(run, n, [c for c, _, _ in layout], [tables[("dc", c)] for c in range(f["ncomp"])],
                        [tables[("ac", c)] for c in range(f["ncomp"])])
            runs.append(Recording.log)
    finally:
        JR.Bits = keep
    return tables, runs


def decoded(data, label):
    """{(length, code)} decoded from the table `label`."""
    return {(e[1], e[2]) for run in record(data)[1] for e in run if e[0] == label}


def blocks_of(data):
    """Per block [component, symbols of the block]."""
    out = []
    for run in record(data)[1]:
        for e in run:
            if e[0][0] == "dc":
                out.append([e[0][1], []])
            out[-1][1].append(e)
    return out


def long_codes_of(table):
    return {k for k in table.codes if k[0] >= 10}


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_sweep_decodes_every_ac_symbol_of_both_standard_tables(variant):
    s = JC.sweep()[variant]
    tables, runs = record(s.data)
    assert len(runs) == (1, 42, 11)[variant]
    for c in range(3):
        t = tables[("ac", c)]
        assert set(t.codes.values()) == ALL_AC and len(t.codes) == 162
        got = decoded(s.data, ("ac", c))
        assert {t.codes[k] for k in got} == ALL_AC, f"component {c}: AC symbols never decoded"
        assert long_codes_of(t) <= got
    assert len(long_codes_of(tables[("ac", 0)])) == 139 and len(long_codes_of(tables[("ac", 1)])) == 135
    # each size, both signs, both ends of the range -- in the coefficients libjpeg returned
    for c, plane in enumerate((s.Y, s.C[0], s.C[1])):
        ac = set(plane[..., 1:].ravel().tolist())
        for size in range(1, 11):
            assert set(JC.ends(size)) <= ac, (c, size)


def test_sweep_dc_categories_zrl_chains_and_block_shapes():
    s = JC.sweep()[0]
    blocks = blocks_of(s.data)
    for c in range(3):
        mine = [b for comp, b in blocks if comp == c]
        dc = {(e[3], e[4] >= (1 << (e[3] - 1)) if e[3] else None) for e in (b[0] for b in mine)}
        assert dc == {(0, None)} | {(cat, sign) for cat in range(1, 12) for sign in (False, True)}, (c, sorted(dc, key=str))
        chains = set()
        for b in mine:
            n = 0
            for e in b[1:]:
                if e[3] == JC.ZRL:
                    n += 1
                else:
                    chains.add((n, "EOB" if e[3] == JC.EOB else "coefficient"))
                    n = 0
        assert {(n, what) for n in (1, 2, 3) for what in ("EOB", "coefficient")} <= chains, (c, chains)
        assert any(len(b) == 2 and b[0][3] and b[1][3] == JC.EOB for b in mine), "a DC-only block"
        assert any(len(b) > 2 and b[-1][3] != JC.EOB for b in mine), "a block that ends at coefficient 63 without EOB"
    for plane in (s.Y, s.C[0], s.C[1]):
        flat = plane.reshape(-1, 64)
        assert (flat == 0).all(1).any(), "an all-zero block"
        assert (flat[:, 1:] != 0).all(1).any(), "a block with all 63 AC coefficients"
    # the three restart variants hold the same coefficients
    for other in JC.sweep()[1:]:
        assert same(other.Y, other.C, s)


def test_long_codes_reach_first_and_last_code_of_every_length_in_six_tables():
    s = JC.long_codes()
    tables, _ = record(s.data)
    assert len({tuple(sorted(t.codes.items())) for t in tables.values()}) == 6
    plan = dm.prepare_jpeg_batch([s.data], grid=tuple(s.grid))
    assert plan.ntables == 6 and len(set(plan.images[0, 5:11].tolist())) == 6
    assert {k[0] for t in tables.values() for k in t.codes} == set(range(1, 17)), "every code length occurs"
    straddle = 0
    for label, t in tables.items():
        got = decoded(s.data, label)
        assert got == set(t.codes), f"{label}: codes never decoded"
        for length in range(10, 17):
            codes = sorted(c for n, c in t.codes if n == length)
            if label[0] == "ac":
                assert len(codes) >= 2, (label, length)
            if codes:
                assert (length, codes[0]) in got and (length, codes[-1]) in got
        nine, ten = [c for n, c in got if n == 9], [c for n, c in got if n == 10]
        straddle += sum(1 for a in nine for b in ten if a >> 1 == b >> 2)
    assert straddle, "a 9-bit and a 10-bit code with the same first 8 bits: the edge of the first-level table"
    assert not np.array_equal(s.C[0], s.C[1])


def test_stuffing_files_end_runs_in_ff_at_every_length_residue():
    gray0, gray2, colour = JC.stuffing()
    assert same(gray0.Y, gray0.C, gray2) and len(gray2.data) == len(gray0.data) + 2 * 35
    for s, fill in ((gray0, 0), (gray2, 2), (colour, 2)):
        f = JR.parse(s.data)
        runs = f["runs"]
        assert f["had_stuffing"] and {len(r) % 4 for r in runs} == {0, 1, 2, 3}, s.name
        assert runs[-1][-1] == 0xFF and any(r[-1] == 0xFF for r in runs[:-1]), "FF as last byte in front of EOI and of RSTn"
        assert s.data.endswith(b"\xff\x00" + b"\xff" * (fill + 1) + b"\xd9")
        assert any(b"\xff\x00" + b"\xff" * (fill + 1) + bytes([0xD0 + k]) in s.data for k in range(8))
        if fill:
            assert b"\xff\xff\xff\xd0" in s.data and b"\xff\xff\xff\xd9" in s.data
        body = b"".join(runs)
        assert body.count(b"\xff") * 10 >= len(body), f"{s.name}: {body.count(bytes([255]))} FF among {len(body)} bytes"
    runs = JR.parse(gray0.data)["runs"]
    assert {len(r) % 4 for r in runs if r[-1] == 0xFF} == {0, 1, 2, 3} == {len(r) % 4 for r in runs if r[-1] != 0xFF}
    assert runs[0] == b"\x2b", "the one-byte run: DC difference 0 (00), EOB (1010), two padding bits"


# ---- the writer's own refusals ------------------------------------------------------------------------------------------------
def test_prefix_code_helper():
    assert JW.prefix_code([3, 1, 2]) == [1, 1, 1] + [0] * 13
    assert JW.codes_of(*JW.table_from_lengths([(5, 2), (7, 1), (9, 3)])) == {7: (1, 0), 5: (2, 2), 9: (3, 6)}
    for bad in ([1, 1, 1], [1, 2, 2, 2], [2] * 5, [16] * 3 + [1, 1]):
        with pytest.raises(ValueError, match="over-subscribed"):
            JW.prefix_code(bad)
    for bad in ([1, 1], [1, 2, 2], [1, 2, 3, 3], [1] + list(range(2, 17)) + [16]):
        with pytest.raises(ValueError, match="all-ones"):
            JW.prefix_code(bad)
    luma = JC.standard_tables()[0]
    over = ([2] + [0] * 15, [0, 1])
    with pytest.raises(ValueError, match="all-ones"):
        JW.write([np.zeros((1, 1, 64), int)], [JC.QUANT_Y], [(1, 1)], [(over, luma[1])], 8, 8)
    with pytest.raises(ValueError, match="size 11"):
        JW.write([np.full((1, 1, 64), 1024)], [JC.QUANT_Y], [(1, 1)], [luma], 8, 8)
    for t in JC.standard_tables() + tuple(JC.long_tables()):
        for bits, vals in t:
            assert JW.bits_vals(JR.Table.from_dht(bits, vals)) == (list(bits), list(vals))


# ---- refusals of the host half ------------------------------------------------------------------------------------------------
def test_three_scan_file_is_refused_alone():
    a, b, three = JC.standard_420(1), JC.standard_420(2), JC.three_scans()
    Yh, Ch, Qh, grid = host(three.data)
    assert grid == (8, 8) and same(Yh, Ch, three) and np.array_equal(Qh, three.quant)     # libjpeg reads it
    assert three.data.count(b"\xff\xda") == 3
    plan = dm.prepare_jpeg_batch([a.data, three.data, b.data], grid=(8, 8))
    assert plan.status[:3].tolist() == [0, -12, 0] and "several scans" in plan.messages[1]
    check_plan(plan, 0, a)
    check_plan(plan, 2, b)
    runs = plan.runs[:plan.nruns].numpy()
    assert set(runs[runs[:, 4] > 0][:, 2].tolist()) == {0, 2}


def test_over_subscribed_huffman_table_is_refused_before_it_is_derived():
    """162 codes of length 1 in the AC table: deriving the look-up table of such counts would index past it (the first-level table
    has 512 entries; code 161 of length 1 would land at entry 41216).  libjpeg refuses the file; so must prepare, touching
    nothing beyond the plan's table slot.  tools/jpeg_scan_check.cpp runs the same file under the address sanitizer."""
    data = JC.over_subscribed()
    with pytest.raises(dm.libjpeg_exception):
        dm.read_coefficients_bytes(data)
    a = JC.standard_420(1)
    out = dm.JpegBatchPlan(2, (8, 8), tables_cap=5)
    out.tables.fill_(0x5A)
    plan = dm.prepare_jpeg_batch([data, a.data], grid=(8, 8), out=out)
    assert plan.status[:2].tolist() == [-11, 0] and "prefix code" in plan.messages[0], plan.messages
    check_plan(plan, 1, a)
    assert plan.ntables == 4 and (out.tables[4] == 0x5A).all(), "the slot behind the used tables is untouched"


# ---- seeded defects -----------------------------------------------------------------------------------------------------------
DEFECTS = ["cr reads cb's tables"] + [f"value index off by one at length {n}" for n in range(10, 17)] + \
    ["zrl skips 15", "extend threshold <=", "predictors not reset per run"]


def defective_decode(data, defect):
    """jpeg_ref.decode_file with a copy of walk_run that has ONE change (None: none).  Planes, or the exception's name."""
    f = JR.parse(data)
    mcus_x, mcus_y, layout, hs, vs, grids = JR._geometry(f["ncomp"], f["width"], f["height"], f["hs"], f["vs"])
    off_by_one = int(defect.rsplit(" ", 1)[1]) if defect and defect.startswith("value index") else 0
    pred = [0, 0, 0]

    def symbol(br, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | br.bit()
            if (length, code) in table.codes:
                if length == off_by_one:                  # vals[code + valoff + 1]: the symbol of the next code in canonical order
                    order = sorted(table.codes)
                    i = order.index((length, code)) + 1
                    return table.codes[order[i]] if i < len(order) else 0
                return table.codes[(length, code)]
        raise ValueError("unassigned Huffman code")

    def extend(v, s):
        if defect == "extend threshold <=":
            return v - (1 << s) + 1 if s and v <= (1 << (s - 1)) else v
        return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v

    def walk_run(run, nmcu):
        br = JR.Bits(run)
        if defect != "predictors not reset per run":
            pred[:] = [0, 0, 0]
        out = []
        for _ in range(nmcu):
            for comp, _, _ in layout:
                t = 1 if comp == 2 and defect == "cr reads cb's tables" else comp
                blk = [0] * 64
                s = symbol(br, f["dc"][t])
                pred[comp] += extend(br.take(s), s)
                blk[0] = pred[comp]
                k = 1
                while k < 64:
                    sym = symbol(br, f["ac"][t])
                    r, s = sym >> 4, sym & 15
                    if s:
                        k += r
                        blk[JR.ZIGZAG[k]] = extend(br.take(s), s)
                        k += 1
                    elif r == 15:
                        k += 15 if defect == "zrl skips 15" else 16
                    else:
                        break
                out.append((comp, blk))
        if not 0 <= 8 * len(run) - br.pos < 8:
            raise ValueError("bits left over")
        return out

    nmcu, ri = mcus_x * mcus_y, f["restart"]
    try:
        per_run = [(j * ri, walk_run(run, min(ri, nmcu - j * ri) if ri else nmcu)) for j, run in enumerate(f["runs"])]
        return JR.place(per_run, f["ncomp"], mcus_x, layout, hs, vs, grids)
    except (ValueError, IndexError, AssertionError) as e:
        return type(e).__name__


def catches(data, defect, clean):
    got = defective_decode(data, defect)
    return isinstance(got, str) or any(not np.array_equal(a, b) for a, b in zip(got, clean))


@functools.lru_cache(maxsize=None)
def clean_decode(data):
    got = defective_decode(data, None)
    assert not isinstance(got, str)
    return got


def first_catch(files, defect):
    for name, data in files.items():
        if catches(data, defect, clean_decode(data)):
            return name
    return None


def test_the_undamaged_copy_of_the_walk_is_a_decoder():
    for s in CASES.values():
        planes = clean_decode(s.data)
        assert same(planes[0], np.stack(planes[1:]) if len(planes) == 3 else None, s)


@pytest.mark.parametrize("defect", DEFECTS)
def test_each_seeded_defect_changes_a_synthetic_file(defect):
    name = first_catch({k: s.data for k, s in CASES.items()}, defect)
    print(f"{defect}: first shown by {name}")
    assert name is not None


def test_what_the_pillow_files_show_of_the_seeded_defects():
    """The gap this file closes: every Pillow-made file names one table pair for Cb and Cr, so a decoder that reads Cr through Cb's
    tables returns the right bits for all of them.  The other defects: printed, not asserted (they depend on the installed Pillow)."""
    files = {**JC.g1_files(), **JC.pillow_files(), **{f"batch{i}": d for i, d in enumerate(JC.small_batch())}}
    for data in files.values():
        f = JR.parse(data)
        assert f["ncomp"] == 1 or (f["dc"][1] is f["dc"][2] and f["ac"][1] is f["ac"][2])
    assert first_catch(files, DEFECTS[0]) is None
    for defect in DEFECTS[1:]:
        print(f"{defect}: {first_catch(files, defect) or 'NOT shown by any Pillow-made file'}")
    std = record(files["q75"])[0]
    for c, which in ((0, "luma"), (1, "chroma")):
        t, got = std[("ac", c)], set()
        for data in files.values():
            for label, other in record(data)[0].items():
                if label[0] == "ac" and other.codes == t.codes:
                    got |= decoded(data, label)
        print(f"codes of 10 bits or more decoded from the standard {which} AC table by these files: "
              f"{len(got & long_codes_of(t))}/{len(long_codes_of(t))}")
