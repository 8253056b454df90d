"""Host half of the device JPEG decode, without a GPU: dct_manip.prepare_jpeg_batch (librgbnm.so, csrc/jpeg_scan.h) must put into
its plan everything a decoder needs.  The plan's OWN buffers -- un-stuffed stream, run records, image record, look-up tables -- are
walked by the plain-Python restatement tests/jpeg_ref.py, and the result must equal the host libjpeg reader
(dm.read_coefficients_bytes) bit for bit.  Refusals are per file and leave the rest of the batch alone."""
import io

import numpy as np
import pytest
import torch
from PIL import Image

import jpeg_cases as JC
import jpeg_ref as JR
from rgb_no_more_amd import dct_manip as dm

CASES = {**JC.g1_files(), **JC.pillow_files()}


def host(data):
    """libjpeg's coefficients of one file: (Y [Hb, Wb, 64], CbCr [2, Hbc, Wbc, 64] | None, quant [C, 64], grid)."""
    _, quant, Y, CbCr = dm.read_coefficients_bytes(data)
    hb, wb = Y.shape[1:3]
    return (Y.numpy().reshape(hb, wb, 64), None if CbCr is None else CbCr.numpy().reshape(2, CbCr.shape[1], CbCr.shape[2], 64),
            quant.numpy().reshape(-1, 64), (hb, wb))


def check_against_host(plan, i, data):
    Yh, Ch, Qh, _ = host(data)
    Y, C = JR.decode_plan(plan, i)
    assert np.array_equal(Y, Yh)
    assert (C is None) == (Ch is None) and (C is None or np.array_equal(C, Ch))
    q = plan.quant[i].numpy().reshape(3, 64)
    assert np.array_equal(q[:len(Qh)], Qh) and (q[len(Qh):] == 1).all()       # unit tables in the unused chroma slots


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_decodes_to_the_host_readers_coefficients(name):
    data = CASES[name]
    Yh, Ch, Qh, grid = host(data)
    plan = dm.prepare_jpeg_batch([data], grid=grid)
    assert plan.nbad == 0 and int(plan.status[0]) == 0, plan.messages
    check_against_host(plan, 0, data)
    # the yardstick on its own feet: its own marker parse and un-stuffing give the same coefficients
    Y, C, Q = JR.decode_file(data)
    assert np.array_equal(Y, Yh) and (C is None) == (Ch is None) and (C is None or np.array_equal(C, Ch)) and np.array_equal(Q, Qh)
    f = JR.parse(data)
    assert plan.nruns == len(f["runs"])
    want = {"rst_blocks1": 35, "rst_blocks2": 18, "rst_blocks3": 12, "rst_rows1": 5, "gray_rst": 30}.get(name, 1)
    assert plan.nruns == want
    # the un-stuffed bytes of every run, as the yardstick found them
    runs, stream = plan.runs[:plan.nruns].numpy(), plan.stream.numpy()
    for r, ref in zip(runs, f["runs"]):
        assert bytes(stream[int(r[0]):int(r[0]) + int(r[1])]) == ref


def test_some_scan_holds_a_stuffed_ff():
    assert any(JR.parse(d)["had_stuffing"] for d in CASES.values())


def test_tables_are_stored_once_per_batch():
    p = JC.pillow_files()
    plan = dm.prepare_jpeg_batch([p["q30"], p["q75"]], grid=(9, 13))
    assert plan.nbad == 0 and plan.ntables == 4                 # the four standard tables, shared by both files
    assert plan.images[0, 5:11].tolist() == plan.images[1, 5:11].tolist()
    plan = dm.prepare_jpeg_batch([p["q30"], p["optimize"], p["q75"]], grid=(9, 13))
    assert plan.nbad == 0 and 4 < plan.ntables <= 8             # the optimised file adds its own
    assert plan.images[0, 5:11].tolist() == plan.images[2, 5:11].tolist() != plan.images[1, 5:11].tolist()
    for i, k in enumerate(("q30", "optimize", "q75")):
        check_against_host(plan, i, p[k])


def _save(img, **kw):
    buf = io.BytesIO()
    img.save(buf, format="JPEG", **kw)
    return buf.getvalue()


def test_refusals_are_per_file():
    good = JC.encode(JC.noisy(64, 64, 3), quality=80)
    good2 = JC.encode(JC.noisy(64, 64, 4), quality=70, restart_marker_blocks=2)
    rgb = Image.fromarray(JC.noisy(64, 64, 5))
    sos = good2.index(b"\xff\xda")
    at = good2.index(b"\xff\xd1", sos)
    bad = {
        "progressive": (_save(rgb, quality=80, progressive=True), -12),
        "cmyk": (_save(rgb.convert("CMYK"), quality=80), -12),
        "444": (_save(rgb, quality=80, subsampling="4:4:4"), -13),           # its chroma grid is 8 x 8, the batch's 4 x 4
        "wrong grid": (JC.encode(JC.noisy(48, 64, 6), quality=80), -13),
        "cut in the header": (good[:good.index(b"\xff\xc4") + 9], -10),
        "cut inside the scan": (good[:good.index(b"\xff\xda") + 14 + 200], -10),
        "wrong RSTn": (good2[:at + 1] + b"\xd3" + good2[at + 2:], -14),
        "not a jpeg": (b"this is not a jpeg file at all", -11),
    }
    names = list(bad)
    batch = [good] + [bad[k][0] for k in names] + [good2]
    plan = dm.prepare_jpeg_batch(batch, grid=(8, 8))
    st = plan.status[:plan.n].tolist()
    assert st[0] == 0 and st[-1] == 0 and plan.nbad == len(names)
    for j, k in enumerate(names):
        assert st[1 + j] == bad[k][1], (k, st[1 + j], plan.messages[1 + j])
        assert plan.messages[1 + j], k
    # the good files of the mixed batch decode as they do alone
    check_against_host(plan, 0, good)
    check_against_host(plan, len(batch) - 1, good2)
    # every record of the plan is either a good file's run or empty (skipped by the device)
    runs = plan.runs[:plan.nruns].numpy()
    assert set(runs[runs[:, 4] > 0][:, 2].tolist()) == {0, len(batch) - 1}


def test_capacity_is_a_per_file_refusal_and_buffers_are_reused():
    p = JC.pillow_files()
    out = dm.JpegBatchPlan(2, (9, 13), stream_cap=len(p["q30"]) + 64, runs_cap=4)
    plan = dm.prepare_jpeg_batch([p["q30"], p["q100"]], grid=(9, 13), out=out)         # the second does not fit any more
    assert plan is out and plan.status[:2].tolist() == [0, -15]
    check_against_host(plan, 0, p["q30"])
    small = JC.encode(JC.noisy(72, 104, 7), quality=20)                                # fits: the buffers are filled again
    assert len(small) < len(p["q30"])
    plan = dm.prepare_jpeg_batch([small], grid=(9, 13), out=out, threads=4)
    assert plan.n == 1 and plan.nbad == 0
    check_against_host(plan, 0, small)
    with pytest.raises(ValueError):
        dm.prepare_jpeg_batch([p["q75"]] * 3, grid=(9, 13), out=out)


def test_threads_give_the_same_plan():
    files = list(JC.pillow_files().values())
    files = [f for f in files if host(f)[3] == (9, 13) and host(f)[1] is not None]
    a = dm.prepare_jpeg_batch(files, grid=(9, 13), threads=1)
    b = dm.prepare_jpeg_batch(files, grid=(9, 13), threads=5)
    assert a.nbad == b.nbad == 0 and a.nruns == b.nruns and a.stream_bytes == b.stream_bytes
    assert torch.equal(a.runs[:a.nruns], b.runs[:b.nruns]) and torch.equal(a.images[:a.n], b.images[:b.n])
    for r in a.runs[:a.nruns].numpy():
        o, n = int(r[0]), int(r[1])
        assert torch.equal(a.stream[o:o + n], b.stream[o:o + n])
