"""CPU side of the split device JPEG decode for crop boxes (include/rgbnm.h: rgbnm_jpeg_decode_batch_split_crop): the ABI, what the
call refuses before any HIP call, the scratch bound, the Python keywords and their defaults, the loader's new value and its refusals,
the numpy restatement of the live test (tests/jpeg_split_crop_ref.py) checked by hand, the stand-alone sanitizer build of the shared
text (tools/jpeg_split_crop_check.cpp) on a small share of its damaged inputs -- and that no comparison of the GPU tests
(tests/test_jpeg_split_crop_kernels.py) can pass vacuously: every (file set, setting, box) they use has an image the segment lanes
write, and, for every box but the largest, live and skipped segments."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

import jpeg_cases as JC
import jpeg_crop_ref as CR
import jpeg_split_crop_ref as XR
import jpeg_split_ref as SR
from rgb_no_more_amd import custom_transforms as CT
from rgb_no_more_amd import dct_manip as dm
from rgb_no_more_amd import lib as L
from rgb_no_more_amd.loader import DCTBatchLoader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "rgbnm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+rgbnm_jpeg_decode_batch_split_crop\s*\(([^)]*)\)\s*;", code)
    assert m, "rgbnm_jpeg_decode_batch_split_crop is not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const rgbnm_jpeg_device_plan* plan", "int n", "int Hb", "int Wb", "int Hbc", "int Wbc", "const int32_t* boxes",
                    "const long long* y_off", "const long long* c_off", "int16_t* Ypacked", "size_t y_elems", "int16_t* Cpacked",
                    "size_t c_elems", "int32_t* status", "int32_t* path", "uint32_t* walked", "uint32_t* seg_live", "void* scratch",
                    "size_t scratch_bytes", "int seg_bits", "int rounds", "void* stream"]
    res, argt = L.PROTOTYPES["rgbnm_jpeg_decode_batch_split_crop"]
    want = [C.POINTER(L.JpegDevicePlan)] + [C.c_int] * 5 + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p, C.c_size_t] + [C.c_void_p] * 5 + \
        [C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    assert res is C.c_int and list(argt) == want
    assert re.search(r"size_t\s+rgbnm_jpeg_split_crop_scratch_bytes\s*\(size_t stream_bytes, int nruns, int seg_bits\);", code)
    assert L.PROTOTYPES["rgbnm_jpeg_split_crop_scratch_bytes"] == (C.c_size_t, [C.c_size_t, C.c_int, C.c_int])
    assert L.lib().rgbnm_jpeg_decode_batch_split_crop and L.lib().rgbnm_jpeg_split_crop_scratch_bytes      # AttributeError if not exported
    # the existing calls keep their declarations
    assert re.search(r"int\s+rgbnm_jpeg_decode_batch\s*\(const rgbnm_jpeg_device_plan\* plan, int n, int Hb, int Wb, int Hbc, int Wbc, "
                     r"int16_t\* Y, int16_t\* CbCr,\s*int32_t\* status, void\* stream\);", code)
    assert re.search(r"size_t\s+rgbnm_jpeg_split_scratch_bytes\s*\(size_t stream_bytes, int nruns, int seg_bits\);", code)
    assert re.search(r"int\s+rgbnm_jpeg_decode_batch_split\s*\(const rgbnm_jpeg_device_plan\* plan, int n, int Hb, int Wb, int Hbc, int Wbc, "
                     r"int16_t\* Y, int16_t\* CbCr,\s*int32_t\* status, int32_t\* path, void\* scratch, size_t scratch_bytes, int seg_bits, "
                     r"int rounds,\s*void\* stream\);", code)
    assert re.search(r"int\s+rgbnm_jpeg_decode_batch_crop\s*\(const rgbnm_jpeg_device_plan\* plan, int n, int Hb, int Wb, int Hbc, int Wbc, "
                     r"const int32_t\* boxes,\s*const long long\* y_off, const long long\* c_off, int16_t\* Ypacked, size_t y_elems, "
                     r"int16_t\* Cpacked,\s*size_t c_elems, int32_t\* status, uint32_t\* walked, void\* stream\);", code)
    assert "The split decode takes no box" not in text and "rgbnm_jpeg_decode_batch_split_crop below" in text


def test_scratch_bound():
    split, crop = L.lib().rgbnm_jpeg_split_scratch_bytes, L.lib().rgbnm_jpeg_split_crop_scratch_bytes
    for stream_bytes, nruns, seg_bits in ((0, 0, 2048), (1, 1, 128), (4096, 3, 256), (1 << 20, 256, 2048), (123457, 8275, 65536), (1 << 30, 1, 128)):
        s, c = split(stream_bytes, nruns, seg_bits), crop(stream_bytes, nruns, seg_bits)
        slots = stream_bytes * 8 // seg_bits + nruns + 1
        assert s > 0 and c >= s + 4 * slots + 8 * nruns + 4 and c % 16 == 0 and c <= s + 4 * slots + 8 * nruns + 64, (stream_bytes, nruns, seg_bits)
    for stream_bytes, nruns, seg_bits in ((4096, -1, 256), (4096, 3, 96), (4096, 3, 100), (4096, 3, 65568), (4096, 3, 0), ((1 << 40) + 1, 3, 256),
                                          (1 << 40, 3, 128)):
        assert split(stream_bytes, nruns, seg_bits) == 0 and crop(stream_bytes, nruns, seg_bits) == 0, (stream_bytes, nruns, seg_bits)


def test_refusals_are_decided_before_any_device_call():
    """Host memory stands in for every buffer: a refused call touches none of it."""
    f = L.lib().rgbnm_jpeg_decode_batch_split_crop
    need = L.lib().rgbnm_jpeg_split_crop_scratch_bytes(4096, 3, 256)
    buf = torch.zeros((1 << 16) + need, dtype=torch.uint8)
    base = (buf.data_ptr() + 63) & ~63                           # 64-byte aligned addresses inside buf
    Y, Cc, st, bx, yo, co, wk, pl, pa, lv, sc = (base + 4096 * k for k in range(11))
    dp = L.JpegDevicePlan(stream=pl, stream_bytes=4096, runs=pl + 64, images=pl + 128, tables=pl + 256, nruns=3, ntables=2)

    def call(plan=dp, n=2, grid=(4, 4, 2, 2), bx=bx, yo=yo, co=co, Y=Y, ye=1024, Cc=Cc, ce=512, st=st, pa=pa, wk=wk, lv=lv, sc=sc, nb=need,
             sb=256, rounds=4):
        return f(C.byref(plan) if plan is not None else None, n, *grid, bx, yo, co, Y, ye, Cc, ce, st, pa, wk, lv, sc, nb, sb, rounds, None)

    # whatever the crop call refuses
    assert call(plan=None) == -1 and call(n=0) == -1 and call(n=-3) == -1
    for grid in ((0, 4, 2, 2), (4, 0, 2, 2), (4, 4, 0, 2), (4, 4, 2, 0), (4097, 4, 2, 2), (4, 4097, 2, 2), (4, 4, 4097, 2), (4, 4, 2, 4097)):
        assert call(grid=grid) == -1, grid
    assert call(Y=None) == -1 and call(Cc=None) == -1 and call(st=None) == -1
    assert call(bx=None) == -1 and call(yo=None) == -1 and call(co=None) == -1
    assert call(Y=Y + 8) == -1 and call(Cc=Cc + 2) == -1 and call(st=st + 2) == -1
    assert call(bx=bx + 2) == -1 and call(yo=yo + 4) == -1 and call(co=co + 4) == -1 and call(wk=wk + 2) == -1
    assert call(ye=0) == -1 and call(ce=0) == -1
    for field, value in (("nruns", -1), ("ntables", -1), ("stream", None), ("runs", None), ("images", None), ("tables", None),
                         ("stream", pl + 2), ("tables", pl + 264), ("runs", pl + 66), ("images", pl + 130)):
        bad = L.JpegDevicePlan(stream=pl, stream_bytes=4096, runs=pl + 64, images=pl + 128, tables=pl + 256, nruns=3, ntables=2)
        setattr(bad, field, value)
        assert call(plan=bad) == -1, field
    # whatever the split call refuses
    assert call(pa=None) == -1 and call(pa=pa + 2) == -1 and call(sc=None) == -1 and call(sc=sc + 8) == -1
    assert call(rounds=-1) == -1 and call(rounds=65) == -1
    for sb in (0, 96, 100, 65568, -256):
        assert call(sb=sb) == -1, sb
    # the new ones: seg_live misaligned; scratch below the NEW bound (the split call's bound is not enough)
    assert call(lv=lv + 2) == -1 and call(lv=lv + 1) == -1
    assert call(nb=need - 1) == -1 and call(nb=L.lib().rgbnm_jpeg_split_scratch_bytes(4096, 3, 256)) == -1 and call(nb=0) == -1
    assert not buf.any()


def test_python_keywords_and_their_defaults():
    sig = inspect.signature(dm.jpeg_split_crop_scratch).parameters
    assert list(sig) == ["plan", "seg_bits", "device"] and sig["seg_bits"].default is None and sig["device"].default == "cuda"
    sig = inspect.signature(dm.launch_jpeg_split_crop).parameters
    assert list(sig) == ["plan", "dev", "out", "boxes", "packed_out", "path", "scratch", "seg_bits", "rounds", "walked", "seg_live"]
    assert [sig[k].default for k in ("path", "scratch", "seg_bits", "rounds", "walked", "seg_live")] == [None] * 6
    sig = inspect.signature(dm.decode_jpeg_batch_split_crop).parameters
    assert list(sig) == ["plan", "device", "boxes", "out", "seg_bits", "rounds", "return_path"]
    assert [sig[k].default for k in list(sig)[1:]] == ["cuda", None, None, None, None, False]
    sig = inspect.signature(dm.read_coefficients_batch_crop_device).parameters
    assert list(sig) == ["paths_or_bytes", "boxes", "grid", "device", "split"] and sig["split"].default is False
    assert (dm.JPEG_SPLIT_SEG_BITS, dm.JPEG_SPLIT_ROUNDS) == (2048, 16)                 # the split decode's defaults serve this call too
    files = [JC.pillow_files()["q75"]] * 2
    plan = dm.prepare_jpeg_batch(files, grid=(9, 13))
    boxes = [[0, 0, 8, 12], [2, 4, 2, 2]]
    # the two refusals that existing tests pin stay, and now say where to go
    with pytest.raises(ValueError, match="split=False.*decode_jpeg_batch_split_crop"):
        dm.decode_jpeg_batch(plan, "cpu", split=True, boxes=boxes)
    packed = tuple(torch.zeros(s, dtype=t) for s, t in (((2 * 9 * 13 * 64,), torch.int16), ((2 * 2 * 5 * 7 * 64,), torch.int16),
                                                        ((2, 3, 8, 8), torch.int16), ((2,), torch.int32)))
    with pytest.raises(ValueError, match="split=False.*launch_jpeg_split_crop"):
        dm.launch_jpeg_decode(plan, plan.buffers(), packed, split=True, boxes=boxes)
    # a bad box raises the host crop reader's text before anything is prepared or launched
    for bad in ([[0, 0, 8, 12], [1, 4, 2, 2]], [[0, 0, 10, 12], [2, 4, 2, 2]], [[0, 0, 8, 14], [2, 4, 2, 2]], [[0, 0, 8, 12], [2, 4, 0, 2]],
                [[0, 0, 8, 12], [-2, 4, 2, 2]]):
        with pytest.raises(ValueError, match=r"crop box outside the coefficient grid \(or not even\)"):
            dm.read_coefficients_batch_crop_device(files, bad, grid=(9, 13), device="cpu", split=True)
        with pytest.raises(ValueError, match=r"crop box outside the coefficient grid \(or not even\)"):
            dm.decode_jpeg_batch_split_crop(plan, "cpu", boxes=bad)
    with pytest.raises(ValueError, match="boxes are required"):
        dm.decode_jpeg_batch_split_crop(plan, "cpu")
    bx = torch.tensor(boxes, dtype=torch.int32)
    y_off, c_off, ny, ncc = dm.packed_offsets(bx)
    with pytest.raises(ValueError, match="capturable"):
        dm.launch_jpeg_split_crop(plan, plan.buffers(), packed, boxes, None)
    with pytest.raises(L.RgbnmError, match="no CPU fallback"):       # there is no CPU path behind this launch either
        dm.launch_jpeg_split_crop(plan, plan.buffers(), packed, bx, (y_off, c_off, ny, ncc))
    with pytest.raises(L.RgbnmError, match="seg_bits"):
        dm.jpeg_split_crop_scratch(plan, seg_bits=100, device="cpu")
    assert dm.jpeg_split_crop_scratch(plan, device="cpu").numel() >= dm.jpeg_split_scratch(plan, device="cpu").numel()
    for tool, flag in (("pipeline_bench.py", '"split"'), ("jpeg_decode_step.py", "seg_live")):
        assert flag in open(os.path.join(ROOT, "tools", tool)).read(), tool


def test_loader_accepts_split_and_refuses_what_true_refuses():
    tf = CT.TrainTransform_DCT(size=28, num_ops=2, magnitude=9, ops_list=["Brightness", "Contrast", "Sharpness"])
    paths, labels = ["a.jpg", "b.jpg"], [0, 1]
    ok = DCTBatchLoader(paths, labels, 2, device="cuda", transform=tf, decode="device", crop_on_device="split")
    assert ok.crop_on_device is True and ok.crop_split is True and ok.jpeg_split is False and ok.crop_on_host is False
    assert DCTBatchLoader(paths, labels, 2, device="cuda", transform=tf, decode="device", crop_on_device=True).crop_split is False
    assert DCTBatchLoader(paths, labels, 2, device="cpu").crop_split is False
    with pytest.raises(ValueError, match="choose one"):
        DCTBatchLoader(paths, labels, 2, device="cuda", transform=tf, decode="device", crop_on_device="split", crop_on_host=True)
    with pytest.raises(ValueError, match="jpeg_split"):
        DCTBatchLoader(paths, labels, 2, device="cuda", transform=tf, decode="device", crop_on_device="split", jpeg_split=True)
    with pytest.raises(ValueError, match='crop_on_device="split"'):          # ... and True's refusal now names the new value
        DCTBatchLoader(paths, labels, 2, device="cuda", transform=tf, decode="device", crop_on_device=True, jpeg_split=True)
    with pytest.raises(ValueError, match='decode="device"'):
        DCTBatchLoader(paths, labels, 2, device="cuda", transform=tf, decode="host", crop_on_device="split")
    with pytest.raises(ValueError, match="TrainTransform_DCT"):
        DCTBatchLoader(paths, labels, 2, device="cuda", transform=None, decode="device", crop_on_device="split")
    with pytest.raises(ValueError, match="HIP device"):
        DCTBatchLoader(paths, labels, 2, device="cpu", transform=tf, decode="device", crop_on_device="split")
    ev = CT.TrainTransform_DCT(size=28, num_ops=2, magnitude=9, ops_list=["Brightness"], eval_mode=True)
    with pytest.raises(ValueError, match="eval transform"):
        DCTBatchLoader(paths, labels, 2, device="cuda", transform=ev, decode="device", crop_on_device="split")
    with pytest.raises(ValueError, match="crop_on_device must be"):
        DCTBatchLoader(paths, labels, 2, device="cuda", transform=tf, decode="device", crop_on_device="spilt")


def test_live_restatement_by_hand():
    """A 3 x 2-MCU 4:2:0 run (mcus_x 3, 6 blocks per MCU, 36 blocks): MCU m = (my, mx) holds luma blocks (2 my .. 2 my + 1,
    2 mx .. 2 mx + 1) and chroma block (my, mx).  Blocks 6 m .. 6 m + 5 belong to MCU m."""
    S = CR.S420

    def live(b0, nstart, box, mcu0=0, nmcu=6):
        return XR.seg_is_live(b0, nstart, mcu0, nmcu, 6, 3, S, box)

    one = (2, 2, 2, 2)                                           # the box of MCU (1, 1), index 4: blocks 24..29
    assert XR.need(range(6), 3, S, one).tolist() == [False, False, False, False, True, False]
    assert live(24, 6, one) and live(29, 1, one) and live(0, 25, one) and live(23, 2, one) and live(29, 7, one)
    assert not live(0, 24, one) and not live(30, 6, one) and not live(23, 1, one) and not live(30, 1, one)
    assert not live(24, 0, one) and not live(10, 0, one)         # a segment in which no block starts
    assert live(0, 1000, one) and not live(30, 1000, one) and not live(36, 5, one)       # cut to the run's 36 blocks
    col = (0, 4, 4, 2)                                           # MCU column 2: MCUs 2 and 5, blocks 12..17 and 30..35
    assert XR.need(range(6), 3, S, col).tolist() == [False, False, True, False, False, True]
    assert live(17, 1, col) and live(18, 13, col) and not live(18, 12, col) and not live(0, 12, col) and live(35, 1, col)
    row = (0, 0, 2, 6)                                           # MCU row 0
    assert live(0, 1, row) and live(17, 1, row) and not live(18, 18, row)
    # the run starts at MCU 3 of the image (a restart interval of one MCU row): block 0 of the run is block 0 of MCU 3
    assert live(6, 1, one, mcu0=3, nmcu=3) and not live(0, 6, one, mcu0=3, nmcu=3) and not live(12, 6, one, mcu0=3, nmcu=3)
    assert not live(0, 18, row, mcu0=3, nmcu=3)
    # one component: an MCU is one block; the box (2, 2, 2, 2) on a 7-wide grid is blocks 16, 17, 23, 24
    g = lambda b0, n: XR.seg_is_live(b0, n, 0, 35, 1, 7, CR.GRAY, one)      # noqa: E731
    assert g(16, 1) and g(17, 1) and not g(18, 5) and g(18, 6) and g(24, 1) and not g(25, 10) and not g(0, 16)
    # 4:2:2 (hs 2, vs 1), 4 MCUs per row, 4 blocks per MCU: luma box (2, 2, 2, 2) -> MCUs 9 and 13, chroma box (1, 1, 1, 1) -> MCU 5
    S422 = [(2, 1), (1, 1), (1, 1)]
    h = lambda b0, n: XR.seg_is_live(b0, n, 0, 16, 4, 4, S422, one)         # noqa: E731
    assert h(20, 1) and h(36, 4) and h(52, 1) and not h(24, 12) and not h(0, 20) and not h(40, 12) and not h(56, 8)


CASES = [(name, sb, ms) for name in ("pillow", "small", "padding", "tables", "many") for sb, ms in XR.SETTINGS]


@pytest.mark.parametrize("name,sb,ms", CASES, ids=[f"{n}-seg{sb}" for n, sb, _ in CASES])
def test_no_gpu_comparison_is_vacuous(name, sb, ms):
    """For every file set and setting of test_jpeg_split_crop_kernels.test_boxes and every box: an image with path 1; but for the
    largest box, a live and a skipped segment.  Where the longest split run has at most 65 segments, the rounds the tests choose make
    convergence certain and every split image must report path 1."""
    files, grid = XR.file_sets()[name]
    plan = dm.prepare_jpeg_batch(files, grid=grid)
    assert plan.nbad == 0
    min_seg = ms or SR.MIN_SEG
    rounds = XR.rounds_for(plan, sb, min_seg)
    recs = XR.records(plan, sb, rounds, min_seg, check=plan.nruns < 1000)
    assert 1 in recs[0], (name, sb, recs[0])
    if rounds >= XR.longest(plan, sb, min_seg) - 1:
        assert 2 not in recs[0], (name, sb, recs[0])
    total = XR.total_segments(recs, plan)
    for box_name, box in CR.boxes_for(grid).items():
        live, walked = XR.expected(plan, recs, [box] * plan.n)
        assert live.sum() > 0, (name, sb, box_name)
        if box_name != "largest":
            assert 0 < live.sum() < total, (name, sb, box_name, int(live.sum()), total)
    if name == "many":
        assert plan.nruns > 8000 and (walked > 0).sum() > 1000   # unsplit runs in the same call


@pytest.mark.parametrize("sb,ms", XR.SETTINGS, ids=["seg256", "seg1024"])
def test_the_other_gpu_inputs_are_not_vacuous_either(sb, ms):
    min_seg = ms or SR.MIN_SEG
    files, grid = XR.damaged_set()
    plan = dm.prepare_jpeg_batch(files, grid=grid)
    assert plan.nbad == 0                                        # the damage is in the scan: the parser accepts every file
    boxes = list(CR.boxes_for(grid).values())
    mixed = [boxes[i % len(boxes)] for i in range(plan.n)]
    for rounds in (0, 1, XR.rounds_for(plan, sb, min_seg)):
        recs = XR.records(plan, sb, rounds, min_seg)
        assert 2 in recs[0]
        if rounds > 1:
            live, _ = XR.expected(plan, recs, mixed)
            assert 1 in recs[0] and 0 < live.sum() < XR.total_segments(recs, plan)
    # the two files whose live segments must share one wave of 64 lanes (seg_bits 256, jpeg_min_seg 2)
    plan = dm.prepare_jpeg_batch([JC.standard_420(7, 96, 64, restart=0).data, JC.long_codes().data], grid=(8, 12))
    recs = XR.records(plan, 256, XR.rounds_for(plan, 256, 2), 2)
    live, _ = XR.expected(plan, recs, [CR.boxes_for((8, 12))["mcu_column"], CR.boxes_for((8, 12))["mcu_row"]])
    assert recs[0] == [1, 1] and live[0] > 0 and live[1] > 0 and live.sum() <= 64 and plan.ntables > 4


def test_damage_keeps_the_markers():
    data = JC.encode(JC.noisy(64, 64, 31), quality=92)
    first, end = XR.scan_span(data)
    bad = XR.damage(data, 0.5)
    assert len(bad) == len(data) and bad[:first] == data[:first] and bad[end:] == data[end:] and bad != data
    assert sum(a != b for a, b in zip(data, bad)) <= 3 and bad.count(b"\xff") == data.count(b"\xff")


@pytest.fixture(scope="module")
def split_crop_check(tmp_path_factory):
    """tools/jpeg_split_crop_check.cpp under the host sanitizers, as a program of its own; skipped where the compiler has no runtime for them."""
    d = tmp_path_factory.mktemp("split_crop_check")
    exe = str(d / "jpeg_split_crop_check")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread"]
    r = subprocess.run(["g++"] + flags + [str(probe), "-o", str(d / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(d / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ has no address / undefined-behaviour sanitizer runtime here")
    r = subprocess.run(["g++"] + flags + [os.path.join(ROOT, "tools", "jpeg_split_crop_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    files = d / "files"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "jpeg_scan_files.py"), str(files)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe, sorted(str(f) for f in files.iterdir())


def test_shared_text_under_the_host_sanitizers(split_crop_check):
    """Every file as given and a tenth of the truncations and mutations: the contract (a) to (d), seg_live, walked, the guard bands
    and the independence of the order of the runs in the list hold for every box and configuration (the program stops at the first
    that does not), and the sanitizers stay silent."""
    exe, files = split_crop_check
    r = subprocess.run([exe, "--share", "10"] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    pat = (r"{}\s+(\d+) decoded, (\d+) refused by the parser, (\d+) by the walk; (\d+) calls: (\d+) clean \((\d+) of them hide a later "
           r"error\), (\d+) not split, (\d+) split, (\d+) split then one-lane; (\d+) of (\d+) segments live")
    m = re.search(pat.format("as given:"), r.stdout)
    assert m, r.stdout[-2000:]
    decoded, _, by_walk, calls, clean, hidden, p0, p1, p2, live, segs = (int(v) for v in m.groups())
    assert decoded >= 35 and by_walk == 0 and calls == clean > 500 and hidden == 0 and p1 > 100 and p2 > 100 and 0 < live < segs
    m = re.search(pat.format("mutations:"), r.stdout)
    assert m, r.stdout[-2000:]
    decoded, _, by_walk, calls, clean, hidden, p0, p1, p2, live, segs = (int(v) for v in m.groups())
    # damaged streams reached every path; some boxes met the error and some lay in front of it
    assert decoded > 100 and by_walk > 50 and calls > clean > 0 and hidden > 20 and p0 > 0 and p1 > 0 and p2 > 0 and 0 < live < segs
