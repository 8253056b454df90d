"""CPU side of the crop form of the device JPEG decode (include/rgbnm.h: rgbnm_jpeg_decode_batch_crop): the ABI, what the call
refuses before any HIP call, the Python keywords and their defaults, the loader's refusals, the numpy restatement of the MCUs a lane
walks (tests/jpeg_crop_ref.py) checked by hand, and the stand-alone sanitizer build of the shared walk (tools/jpeg_crop_check.cpp) on
a small share of its damaged inputs."""
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
from rgb_no_more_amd import custom_transforms as CT
from rgb_no_more_amd import dct_manip as dm
from rgb_no_more_amd import lib as L
from rgb_no_more_amd.loader import DCTBatchLoader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "rgbnm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+rgbnm_jpeg_decode_batch_crop\s*\(([^)]*)\)\s*;", code)
    assert m, "rgbnm_jpeg_decode_batch_crop is not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const rgbnm_jpeg_device_plan* plan", "int n", "int Hb", "int Wb", "int Hbc", "int Wbc", "const int32_t* boxes",
                    "const long long* y_off", "const long long* c_off", "int16_t* Ypacked", "size_t y_elems", "int16_t* Cpacked",
                    "size_t c_elems", "int32_t* status", "uint32_t* walked", "void* stream"]
    res, argt = L.PROTOTYPES["rgbnm_jpeg_decode_batch_crop"]
    want = [C.POINTER(L.JpegDevicePlan)] + [C.c_int] * 5 + [C.c_void_p] * 4 + [C.c_size_t, C.c_void_p, C.c_size_t] + [C.c_void_p] * 3
    assert res is C.c_int and list(argt) == want
    assert L.lib().rgbnm_jpeg_decode_batch_crop                 # AttributeError if the symbol is not exported
    # the new status code is the next free one, in the header and in the binding's table
    codes = {name: int(v) for name, v in re.findall(r"#define\s+(RGBNM_JPEG_E\w+)\s+\((-\d+)\)", text)}
    assert codes["RGBNM_JPEG_EBOX"] == min(codes.values()) == -26 and len(set(codes.values())) == len(codes)
    assert set(L.JPEG_STATUS) == set(codes.values()) and "box" in L.JPEG_STATUS[-26]
    # the existing calls keep their declarations
    assert re.search(r"int\s+rgbnm_jpeg_decode_batch\s*\(const rgbnm_jpeg_device_plan\* plan, int n, int Hb, int Wb, int Hbc, int Wbc, "
                     r"int16_t\* Y, int16_t\* CbCr,\s*int32_t\* status, void\* stream\);", code)
    assert re.search(r"int\s+rgbnm_jpeg_decode_batch_split\s*\(const rgbnm_jpeg_device_plan\* plan, int n, int Hb, int Wb, int Hbc, int Wbc, "
                     r"int16_t\* Y, int16_t\* CbCr,\s*int32_t\* status, int32_t\* path, void\* scratch, size_t scratch_bytes, int seg_bits, "
                     r"int rounds,\s*void\* stream\);", code)


def test_refusals_are_decided_before_any_device_call():
    """Host memory stands in for every buffer: a refused call touches none of it."""
    f = L.lib().rgbnm_jpeg_decode_batch_crop
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    base = (buf.data_ptr() + 63) & ~63                           # 64-byte aligned addresses inside buf
    Y, Cc, st, bx, yo, co, wk, pl = (base + 4096 * k for k in range(8))
    dp = L.JpegDevicePlan(stream=pl, stream_bytes=4096, runs=pl + 64, images=pl + 128, tables=pl + 256, nruns=3, ntables=2)

    def call(plan=dp, n=2, grid=(4, 4, 2, 2), bx=bx, yo=yo, co=co, Y=Y, ye=1024, Cc=Cc, ce=512, st=st, wk=wk):
        return f(C.byref(plan) if plan is not None else None, n, *grid, bx, yo, co, Y, ye, Cc, ce, st, wk, None)

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
    # nothing to do: 0 without a launch, `walked` optional
    empty = L.JpegDevicePlan(stream=None, stream_bytes=0, runs=None, images=None, tables=None, nruns=0, ntables=0)
    assert call(plan=empty) == 0 and call(plan=empty, wk=None) == 0
    assert not buf.any()


def test_python_keywords_exist_and_default_to_the_plain_call():
    sig = inspect.signature(dm.launch_jpeg_decode).parameters
    assert [sig[k].default for k in ("split", "seg_bits", "rounds", "path", "scratch", "boxes", "packed_out", "walked")] == \
        [False, None, None, None, None, None, None, None]
    sig = inspect.signature(dm.decode_jpeg_batch).parameters
    assert [sig[k].default for k in ("device", "out", "split", "seg_bits", "rounds", "return_path", "boxes")] == \
        ["cuda", None, False, None, None, False, None]
    sig = inspect.signature(dm.read_coefficients_batch_crop_device).parameters
    assert list(sig)[:2] == ["paths_or_bytes", "boxes"] and sig["grid"].default == (64, 64) and sig["device"].default == "cuda"
    assert inspect.signature(DCTBatchLoader.__init__).parameters["crop_on_device"].default is False
    files = [JC.pillow_files()["q75"]] * 2
    plan = dm.prepare_jpeg_batch(files, grid=(9, 13))
    boxes = [[0, 0, 8, 12], [2, 4, 2, 2]]
    with pytest.raises(ValueError, match="split=False"):
        dm.decode_jpeg_batch(plan, "cpu", split=True, boxes=boxes)
    packed = tuple(torch.zeros(s, dtype=t) for s, t in (((2 * 9 * 13 * 64,), torch.int16), ((2 * 2 * 5 * 7 * 64,), torch.int16),
                                                        ((2, 3, 8, 8), torch.int16), ((2,), torch.int32)))
    with pytest.raises(ValueError, match="split=False"):
        dm.launch_jpeg_decode(plan, plan.buffers(), packed, split=True, boxes=boxes)
    with pytest.raises(ValueError, match="belong to boxes"):
        dm.launch_jpeg_decode(plan, plan.buffers(), packed, walked=torch.zeros(plan.nruns, dtype=torch.int32))
    with pytest.raises(L.RgbnmError, match="no CPU fallback"):       # there is no CPU path behind the crop launch either
        dm.launch_jpeg_decode(plan, plan.buffers(), packed, boxes=boxes)
    # a bad box raises the host crop reader's text before anything is prepared or launched
    for bad in ([[0, 0, 8, 12], [1, 4, 2, 2]], [[0, 0, 10, 12], [2, 4, 2, 2]], [[0, 0, 8, 14], [2, 4, 2, 2]], [[0, 0, 8, 12], [2, 4, 0, 2]],
                [[0, 0, 8, 12], [-2, 4, 2, 2]]):
        with pytest.raises(ValueError, match=r"crop box outside the coefficient grid \(or not even\)"):
            dm.read_coefficients_batch_crop_device(files, bad, grid=(9, 13), device="cpu")
        with pytest.raises(ValueError, match=r"crop box outside the coefficient grid \(or not even\)"):
            dm.decode_jpeg_batch(plan, "cpu", boxes=bad)
    with pytest.raises(ValueError, match=r"boxes must be \(len\(paths\), 4\)"):
        dm.read_coefficients_batch_crop_device(files, [[0, 0, 8, 12]], grid=(9, 13), device="cpu")
    for tool, flag in (("pipeline_bench.py", '"--crop-on-device"'), ("jpeg_decode_step.py", "walked")):
        assert flag in open(os.path.join(ROOT, "tools", tool)).read(), tool


def test_loader_refusals():
    tf = CT.TrainTransform_DCT(size=28, num_ops=2, magnitude=9, ops_list=["Brightness", "Contrast", "Sharpness"])
    paths, labels = ["a.jpg", "b.jpg"], [0, 1]
    ok = DCTBatchLoader(paths, labels, 2, device="cuda", transform=tf, decode="device", crop_on_device=True)
    assert ok.crop_on_device is True and ok.crop_on_host is False and ok.last_packed is None
    assert DCTBatchLoader(paths, labels, 2, device="cpu").crop_on_device is False
    with pytest.raises(ValueError, match="choose one"):
        DCTBatchLoader(paths, labels, 2, device="cuda", transform=tf, decode="device", crop_on_device=True, crop_on_host=True)
    with pytest.raises(ValueError, match="jpeg_split"):
        DCTBatchLoader(paths, labels, 2, device="cuda", transform=tf, decode="device", crop_on_device=True, jpeg_split=True)
    with pytest.raises(ValueError, match='decode="device"'):
        DCTBatchLoader(paths, labels, 2, device="cuda", transform=tf, decode="host", crop_on_device=True)
    with pytest.raises(ValueError, match="TrainTransform_DCT"):
        DCTBatchLoader(paths, labels, 2, device="cuda", transform=None, decode="device", crop_on_device=True)
    with pytest.raises(ValueError, match="HIP device"):
        DCTBatchLoader(paths, labels, 2, device="cpu", transform=tf, decode="device", crop_on_device=True)
    ev = CT.TrainTransform_DCT(size=28, num_ops=2, magnitude=9, ops_list=["Brightness"], eval_mode=True)
    with pytest.raises(ValueError, match="eval transform"):
        DCTBatchLoader(paths, labels, 2, device="cuda", transform=ev, decode="device", crop_on_device=True)
    # crop_on_host with the device decode keeps raising, and now says where the crop of the device decode is
    with pytest.raises(ValueError, match="crop_on_device"):
        DCTBatchLoader(paths, labels, 2, device="cuda", transform=tf, decode="device", crop_on_host=True)
    # DFT-plane ops: the parameter sampler the producer uses refuses them, as for crop_on_host
    dft = CT.TrainTransform_DCT(size=28, num_ops=2, magnitude=9, ops_list=["Brightness", "Rotate"], dft_ops=True)
    with pytest.raises(NotImplementedError, match="DFT-plane"):
        CT.FastParamSampler(dft, seed=[0, 0, 0])


def test_expected_walked_by_hand():
    """4:2:0 with 7 MCUs per row (the sweep files' grid): MCU (my, mx) holds luma blocks (2 my .. 2 my + 1, 2 mx .. 2 mx + 1)."""
    S = CR.S420
    one = (2, 4, 2, 2)                                           # the box of one MCU: (1, 2), index 9
    assert CR.expected_walked(7, 7, 7, S, one) == 3              # its MCU row as a run: MCUs 7, 8, 9
    assert CR.expected_walked(0, 7, 7, S, one) == 0              # the row above: outside
    assert CR.expected_walked(14, 28, 7, S, one) == 0            # everything below: outside
    assert CR.expected_walked(0, 42, 7, S, one) == 10            # the whole scan as one run stops after MCU 9
    assert CR.expected_walked(9, 1, 7, S, one) == 1 and CR.expected_walked(8, 1, 7, S, one) == 0 and CR.expected_walked(10, 1, 7, S, one) == 0
    box = (2, 2, 4, 6)                                           # MCU rows 1..2, columns 1..3: the last needed MCU is 2 * 7 + 3 = 17
    assert CR.expected_walked(12, 8, 7, S, box) == 6             # MCUs 12..19 cross from row 1 into row 2; the box ends inside: 12..17
    assert CR.expected_walked(16, 4, 7, S, box) == 2             # 16, 17
    assert CR.expected_walked(18, 3, 7, S, box) == 0             # columns 4..6 of row 2
    assert CR.expected_walked(4, 4, 7, S, box) == 0              # columns 4..6 of row 0, column 0 of row 1
    assert CR.expected_walked(8, 4, 7, S, box) == 3              # columns 1..4 of row 1: 8, 9, 10
    assert CR.expected_walked(11, 4, 7, S, box) == 0             # 11..13 right of the box in row 1, 14 left of it in row 2
    assert CR.expected_walked(11, 5, 7, S, box) == 5             # ... and 15 is inside again: no MCU in between can be skipped
    # one component: an MCU is one block
    assert CR.expected_walked(0, 35, 7, CR.GRAY, (2, 4, 2, 2)) == 3 * 7 + 6 and CR.expected_walked(21, 4, 7, CR.GRAY, (2, 4, 2, 2)) == 0
    # 4:2:2 (hs 2, vs 1), 4 MCUs per row: the luma box (2, 2, 2, 2) is MCU rows 2..3 of column 1 (MCUs 9 and 13), the chroma box
    # (1, 1, 1, 1) is MCU (1, 1) (MCU 5): the union of the two, not a rectangle
    S422 = [(2, 1), (1, 1), (1, 1)]
    assert CR.expected_walked(0, 12, 4, S422, (2, 2, 2, 2)) == 10 and CR.expected_walked(0, 16, 4, S422, (2, 2, 2, 2)) == 14
    assert CR.expected_walked(4, 4, 4, S422, (2, 2, 2, 2)) == 2 and CR.expected_walked(6, 3, 4, S422, (2, 2, 2, 2)) == 0
    assert CR.expected_walked(14, 2, 4, S422, (2, 2, 2, 2)) == 0 and CR.expected_walked(0, 4, 4, S422, (2, 2, 2, 2)) == 0


def test_expected_walked_on_prepared_plans():
    """The record fields the numpy function reads, on real plans: the sweep files as 1, 42 and 11 runs, and a gray file."""
    files = [s.data for s in JC.sweep()]
    plan = dm.prepare_jpeg_batch(files, grid=(11, 13))
    assert plan.nbad == 0 and plan.nruns == 1 + 42 + 11
    w = CR.plan_walked(plan, [(2, 4, 2, 2)] * 3)
    assert w[0] == 10 and w[1:43].tolist() == [0] * 9 + [1] + [0] * 32 and w[43:].tolist() == [0, 0, 2] + [0] * 8
    w = CR.plan_walked(plan, [(0, 0, 10, 12)] * 3)               # the largest box: the last MCU row and column are not needed
    assert w[0] == 4 * 7 + 6 and w[1:43].sum() == 30 and w[43:].tolist() == [4, 4, 4, 4, 4, 4, 3, 4, 2, 0, 0]
    gray = dm.prepare_jpeg_batch([JC.pillow_files()["gray_rst"]], grid=(9, 13))        # 9 x 13 blocks, four per run
    w = CR.plan_walked(gray, [(8 - 2, 12 - 2, 2, 2)])
    # blocks 88, 89 (run 22) and 101, 102 (run 25) are in the box; the two runs between them hold none and are skipped
    assert gray.nruns == 30 and w.tolist() == [0] * 22 + [2, 0, 0, 3, 0, 0, 0, 0]


@pytest.fixture(scope="module")
def crop_check(tmp_path_factory):
    """tools/jpeg_crop_check.cpp under the host sanitizers, as a program of its own; skipped where the compiler has no runtime for them."""
    d = tmp_path_factory.mktemp("crop_check")
    exe = str(d / "jpeg_crop_check")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread"]
    r = subprocess.run(["g++"] + flags + [str(probe), "-o", str(d / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(d / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ has no address / undefined-behaviour sanitizer runtime here")
    r = subprocess.run(["g++"] + flags + [os.path.join(ROOT, "tools", "jpeg_crop_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    files = d / "files"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "jpeg_scan_files.py"), str(files)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe, sorted(str(f) for f in files.iterdir())


def test_shared_crop_walk_under_the_host_sanitizers(crop_check):
    """Every file as given and a tenth of the truncations and mutations: invariants (a) to (c), the walked counts and the guard bands
    hold for every box (the program stops at the first that does not), and the sanitizers stay silent."""
    exe, files = crop_check
    r = subprocess.run([exe, "--share", "10"] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    pat = (r"{}\s+(\d+) decoded, (\d+) refused by the parser, (\d+) by the walk; (\d+) boxes: (\d+) clean \((\d+) of them hide a later "
           r"error\), (\d+) runs: (\d+) skipped, (\d+) stopped early, (\d+) of (\d+) MCUs walked")
    m = re.search(pat.format("as given:"), r.stdout)
    assert m, r.stdout[-2000:]
    decoded, _, by_walk, boxes, clean, hidden, runs, skipped, early, walked, mcus = (int(v) for v in m.groups())
    assert decoded >= 35 and by_walk == 0 and boxes == clean > 300 and hidden == 0
    assert skipped > runs // 4 and early > 100 and walked < mcus
    m = re.search(pat.format("mutations:"), r.stdout)
    assert m, r.stdout[-2000:]
    decoded, _, by_walk, boxes, clean, hidden, runs, skipped, early, walked, mcus = (int(v) for v in m.groups())
    # damaged streams reached the crop walk, some boxes met the error and some lay in front of it
    assert decoded > 100 and by_walk > 50 and boxes > clean > 0 and hidden > 20 and skipped > 0 and early > 0
