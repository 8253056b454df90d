"""CPU side of the split device JPEG decode (include/rgbnm.h: rgbnm_jpeg_decode_batch_split, rgbnm_jpeg_split_scratch_bytes): the ABI,
what the call refuses before any HIP call, the Python keywords and their defaults, the plain-Python restatement of the scheme
(tests/jpeg_split_ref.py), and the stand-alone sanitizer build of the shared segment walk (tools/jpeg_split_check.cpp) on a small
share of its damaged inputs."""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import pytest
import torch

import jpeg_cases as JC
import jpeg_split_ref as SR
from rgb_no_more_amd import dct_manip as dm
from rgb_no_more_amd import lib as L
from rgb_no_more_amd.loader import DCTBatchLoader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_agree():
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbnm.h")).read(), flags=re.S)
    assert re.search(r"size_t\s+rgbnm_jpeg_split_scratch_bytes\s*\(\s*size_t\s+stream_bytes,\s*int\s+nruns,\s*int\s+seg_bits\s*\)\s*;", code)
    m = re.search(r"int\s+rgbnm_jpeg_decode_batch_split\s*\(([^)]*)\)\s*;", code)
    assert m, "rgbnm_jpeg_decode_batch_split is not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const rgbnm_jpeg_device_plan* plan", "int n", "int Hb", "int Wb", "int Hbc", "int Wbc", "int16_t* Y", "int16_t* CbCr",
                    "int32_t* status", "int32_t* path", "void* scratch", "size_t scratch_bytes", "int seg_bits", "int rounds", "void* stream"]
    res, argt = L.PROTOTYPES["rgbnm_jpeg_decode_batch_split"]
    want = [C.POINTER(L.JpegDevicePlan)] + [C.c_int] * 5 + [C.c_void_p] * 5 + [C.c_size_t, C.c_int, C.c_int, C.c_void_p]
    assert res is C.c_int and list(argt) == want
    assert L.PROTOTYPES["rgbnm_jpeg_split_scratch_bytes"] == (C.c_size_t, [C.c_size_t, C.c_int, C.c_int])
    lib = L.lib()                                               # AttributeError if a symbol is not exported
    assert lib.rgbnm_jpeg_split_scratch_bytes and lib.rgbnm_jpeg_decode_batch_split
    # the plain call's declaration is what it was
    assert re.search(r"int\s+rgbnm_jpeg_decode_batch\s*\(const rgbnm_jpeg_device_plan\* plan, int n, int Hb, int Wb, int Hbc, int Wbc, "
                     r"int16_t\* Y, int16_t\* CbCr,\s*int32_t\* status, void\* stream\);", code)
    assert L.get_option("jpeg_min_seg") == 0 and L.get_option("jpeg_split_wgs") == 0 and L.get_option("jpeg_lanes") == 0


def test_scratch_bytes_is_monotone_and_refuses_bad_segment_sizes():
    f = L.lib().rgbnm_jpeg_split_scratch_bytes
    for bad in (0, 32, 96, 127, 130, 1000, 65536 + 32, 1 << 20, -1024):
        assert f(1 << 20, 10, bad) == 0, bad
    assert f(1 << 20, -1, 1024) == 0
    assert f(0, 0, 1024) > 0                                    # an empty plan still has a slot
    sizes = [0, 1, 4096, 1 << 20, 22 << 20]
    for sb in (128, 256, 1024, 4096, 65536):
        for nruns in (0, 1, 256, 8192):
            got = [f(s, nruns, sb) for s in sizes]
            assert got == sorted(got) and got[0] > 0 and got[-1] > got[0], (sb, nruns, got)
        for s in sizes:
            got = [f(s, nruns, sb) for nruns in (0, 1, 256, 8192)]
            assert got == sorted(got) and len(set(got)) == 4, (sb, s, got)
    for s in sizes:                                             # smaller segments: more of them
        got = [f(s, 256, sb) for sb in (65536, 4096, 1024, 256, 128)]
        assert got == sorted(got)
    # about 76 bytes per segment: the README's 21.6 MB batch at 1024 bits
    assert 76 * (21_600_000 * 8 // 1024) <= f(21_600_000, 256, 1024) <= 80 * (21_600_000 * 8 // 1024 + 300)


def test_refusals_are_decided_before_any_device_call():
    """Host memory stands in for every buffer: a refused call touches none of it."""
    f = L.lib().rgbnm_jpeg_decode_batch_split
    need = L.lib().rgbnm_jpeg_split_scratch_bytes(4096, 3, 256)
    buf = torch.zeros(1 << 16, dtype=torch.uint8)
    base = (buf.data_ptr() + 63) & ~63                           # 64-byte aligned addresses inside buf
    Y, Cc, st, path, scr, pl = (base + 4096 * k for k in range(6))
    dp = L.JpegDevicePlan(stream=pl, stream_bytes=4096, runs=pl + 64, images=pl + 128, tables=pl + 256, nruns=3, ntables=2)

    def call(plan=dp, n=2, grid=(4, 4, 2, 2), Y=Y, Cc=Cc, st=st, path=path, scr=scr, nbytes=need, sb=256, rounds=2):
        return f(C.byref(plan) if plan is not None else None, n, *grid, Y, Cc, st, path, scr, nbytes, sb, rounds, None)

    assert call(plan=None) == -1 and call(n=0) == -1 and call(grid=(0, 4, 2, 2)) == -1 and call(grid=(4, 4097, 2, 2)) == -1
    assert call(Y=None) == -1 and call(Cc=None) == -1 and call(st=None) == -1
    assert call(Y=Y + 8) == -1 and call(Cc=Cc + 2) == -1 and call(st=st + 2) == -1
    assert call(path=None) == -1 and call(path=path + 2) == -1
    assert call(scr=None) == -1 and call(scr=scr + 8) == -1 and call(nbytes=need - 1) == -1 and call(nbytes=0) == -1
    for sb in (0, 96, 127, 260, 65536 + 32):
        assert call(sb=sb, nbytes=1 << 30) == -1, sb
    assert call(rounds=-1) == -1 and call(rounds=65) == -1
    assert call(sb=128, nbytes=need) == -1                       # smaller segments need more scratch than `need`
    for field, value in (("nruns", -1), ("ntables", -1), ("stream", None), ("runs", None), ("images", None), ("tables", None),
                         ("stream", pl + 2), ("tables", pl + 264), ("runs", pl + 66), ("images", pl + 130)):
        bad = L.JpegDevicePlan(stream=pl, stream_bytes=4096, runs=pl + 64, images=pl + 128, tables=pl + 256, nruns=3, ntables=2)
        setattr(bad, field, value)
        assert call(plan=bad) == -1, field
    assert not buf.any()


def test_python_keywords_exist_and_default_to_the_plain_call():
    sig = inspect.signature(dm.launch_jpeg_decode).parameters
    assert [sig[k].default for k in ("split", "seg_bits", "rounds", "path")] == [False, None, None, None]
    sig = inspect.signature(dm.decode_jpeg_batch).parameters
    assert [sig[k].default for k in ("split", "seg_bits", "rounds", "return_path")] == [False, None, None, False]
    assert inspect.signature(dm.read_coefficients_batch_device).parameters["split"].default is False
    assert inspect.signature(DCTBatchLoader.__init__).parameters["jpeg_split"].default is False
    assert dm.JPEG_SPLIT_SEG_BITS % 32 == 0 and 128 <= dm.JPEG_SPLIT_SEG_BITS <= 65536 and 0 <= dm.JPEG_SPLIT_ROUNDS <= 64
    files = [JC.pillow_files()["q75"]] * 2
    with pytest.raises(ValueError, match='decode="device"'):
        DCTBatchLoader(["a.jpg", "b.jpg"], [0, 1], 2, device="cpu", decode="host", jpeg_split=True)
    assert DCTBatchLoader(["a.jpg", "b.jpg"], [0, 1], 2, device="cpu").jpeg_split is False
    plan = dm.prepare_jpeg_batch(files, grid=(9, 13))
    with pytest.raises(ValueError, match="split=True"):
        dm.decode_jpeg_batch(plan, "cpu", return_path=True)
    out = tuple(torch.zeros(s, dtype=t) for s, t in (((2, 1, 9, 13, 8, 8), torch.int16), ((2, 2, 5, 7, 8, 8), torch.int16),
                                                     ((2, 3, 8, 8), torch.int16), ((2,), torch.int32)))
    for kw in ({}, {"split": True}):                              # both reach the device check: there is no CPU path behind either
        with pytest.raises(L.RgbnmError, match="no CPU fallback"):
            dm.launch_jpeg_decode(plan, plan.buffers(), out, **kw)
    src = open(os.path.join(ROOT, "tools", "pipeline_bench.py")).read()
    assert '"--jpeg-split"' in src


def test_restatement_converges_by_the_contract_and_falls_back_without_rounds():
    """The scheme in plain Python on the plan's own buffers: with rounds >= segments - 1 every well-formed run passes; with no round
    a run of more than one segment passes only if every guessed entry happened to be true."""
    p = JC.pillow_files()
    files = [p["q75"], p["q30"], p["rst_rows1"], p["gray_rst"]]
    plan = dm.prepare_jpeg_batch(files, grid=(9, 13))
    assert plan.nbad == 0
    for sb in (256, 1024):
        _, longest, _ = SR.predict(plan, sb, 0, min_seg=2)
        assert longest - 1 <= 64
        paths, _, per_seg = SR.predict(plan, sb, longest - 1, min_seg=2)
        assert paths == [1, 1, 1, 1 if sb == 256 else 0], (sb, paths)       # gray_rst: runs of four blocks, one segment of 1024 bits each
        assert 1.0 <= per_seg <= longest
        assert SR.predict(plan, sb, 0, min_seg=2)[0][:2] == [2, 2]
    assert SR.predict(plan, 1024, 8, min_seg=1 << 20)[0] == [0, 0, 0, 0]
    # the walk of segment 0 alone is the true walk: one segment that holds the whole run passes without a round
    assert SR.run_passes(SR.runs_of(plan, 0)[0], 65536, 0)[:2] == (True, 1)


@pytest.fixture(scope="module")
def split_check(tmp_path_factory):
    """tools/jpeg_split_check.cpp under the host sanitizers, as a program of its own; skipped where the compiler has no runtime for them."""
    d = tmp_path_factory.mktemp("split_check")
    exe = str(d / "jpeg_split_check")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread"]
    r = subprocess.run(["g++"] + flags + [str(probe), "-o", str(d / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(d / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ has no address / undefined-behaviour sanitizer runtime here")
    r = subprocess.run(["g++"] + flags + [os.path.join(ROOT, "tools", "jpeg_split_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    files = d / "files"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "jpeg_scan_files.py"), str(files)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe, sorted(str(f) for f in files.iterdir())


def test_shared_segment_walk_under_the_host_sanitizers(split_check):
    """A twentieth of the truncations and mutations, every file as given: outputs, status and path equal the one-lane walk's in all
    six configurations (seg_bits 256 / 2048, rounds 0 / 2 / 64), and the sanitizers stay silent."""
    exe, files = split_check
    r = subprocess.run([exe, "--share", "20"] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"mutations:\s+(\d+) decoded, (\d+) refused by the parser, (\d+) by the walk; per configuration: (\d+) not split, "
                  r"(\d+) split, (\d+) split then one-lane", r.stdout)
    assert m, r.stdout[-2000:]
    decoded, _, by_walk, _, split, fell_back = (int(v) for v in m.groups()[:6])
    assert decoded > 100 and by_walk > 30 and split > 100 and fell_back > 100      # both ends of the split path were exercised
