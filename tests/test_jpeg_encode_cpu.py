"""CPU side of the device JPEG encode (include/rgbnm.h: rgbnm_jpeg_encode_batch and its three host-only companions): the ABI, the
header bytes against the reference's files (tests/golden/g26_jpeg_write.npz), the size functions, what the batch call refuses before
any HIP call, and the stand-alone sanitizer build of the shared emit code (tools/jpeg_encode_check.cpp), whose files must equal the
reference's byte for byte and, with restart markers, the plain-Python writer's (tests/jpeg_writer.py) from the SOS header on."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from rgb_no_more_amd import dct_manip as dm
from rgb_no_more_amd import lib as L

from jpeg_encode_ref import CASES, case, scan_start, writer_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_agree():
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbnm.h")).read(), flags=re.S)
    m = re.search(r"int\s+rgbnm_jpeg_encode_batch\s*\(([^)]*)\)\s*;", code)
    assert m, "rgbnm_jpeg_encode_batch is not declared"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const int16_t* Y", "const int16_t* CbCr", "const int16_t* quant", "const int32_t* dims", "int n", "int Hb", "int Wb",
                    "int Hbc", "int Wbc", "int restart", "uint8_t* out", "size_t stride", "int32_t* nbytes", "int32_t* status",
                    "void* scratch", "size_t scratch_bytes", "void* stream"]
    res, argt = L.PROTOTYPES["rgbnm_jpeg_encode_batch"]
    assert res is C.c_int and list(argt) == [C.c_void_p] * 4 + [C.c_int] * 6 + [C.c_void_p, C.c_size_t] + [C.c_void_p] * 3 + \
        [C.c_size_t, C.c_void_p]
    assert L.PROTOTYPES["rgbnm_jpeg_encode_bound"] == (C.c_size_t, [C.c_int] * 6)
    assert L.PROTOTYPES["rgbnm_jpeg_encode_scratch_bytes"] == (C.c_size_t, [C.c_int] * 7 + [C.c_size_t])
    assert L.PROTOTYPES["rgbnm_jpeg_encode_header"] == (C.c_int, [C.c_int] * 3 + [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t])
    assert re.search(r"#define\s+RGBNM_JPEG_ERANGE\s+\(-25\)", code) and re.search(r"#define\s+RGBNM_ABI_VERSION\s+3\b", code)
    assert dm.jpeg_status_text(-25) == "DCT coefficient out of range"
    assert L.get_option("jpeg_encode_wgs") == 0
    sig = inspect.signature(dm.encode_jpeg_batch).parameters
    assert list(sig)[:7] == ["Y", "CbCr", "quant", "dims", "restart", "stride", "out"]
    assert [sig[k].default for k in ("dims", "restart", "stride", "out")] == [None, 0, None, None]
    assert list(inspect.signature(dm.write_coefficients).parameters) == ["path", "dimensions", "quantization", "Y", "CbCr"]
    assert list(inspect.signature(dm.write_coefficients_batch).parameters) == ["paths", "dims", "quant", "Y", "CbCr", "restart"]


def test_header_bytes_equal_the_reference_files(golden):
    g = golden("g26_jpeg_write.npz")
    for name in CASES:
        h, w, quant, _, Cc, data = case(g, name)
        n = scan_start(data)
        assert n == (623 if Cc is not None else 328)
        assert dm.jpeg_encode_header(h, w, quant) == data[:n], name
    # with a restart interval: DRI between the last DHT and SOS, nothing else changes; the writer agrees on DRI and the SOS header
    # (it orders the DHT segments differently)
    h, w, quant, Y, Cc, data = case(g, "r24x40")
    n = scan_start(data)
    for ri in (1, 4, 65535):
        got = dm.jpeg_encode_header(h, w, quant, restart=ri)
        assert got == data[:n - 14] + b"\xff\xdd\x00\x04" + ri.to_bytes(2, "big") + data[n - 14:n]
        ref = writer_file(h, w, quant, Y, Cc, ri)
        assert got[-20:] == ref[scan_start(ref) - 20:scan_start(ref)]
    assert dm.jpeg_encode_header(h, w, quant, restart="row") == dm.jpeg_encode_header(h, w, quant, restart=3)      # 40 px: 3 MCUs


def test_header_refuses_bad_arguments():
    f = L.lib().rgbnm_jpeg_encode_header
    q = torch.full((3, 64), 7, dtype=torch.int16)
    buf = (C.c_uint8 * 640)()
    assert f(3, 16, 16, q.data_ptr(), 0, buf, 640) == 623 and f(1, 16, 16, q.data_ptr(), 0, buf, 640) == 328
    assert f(3, 16, 16, q.data_ptr(), 5, buf, 640) == 629
    for args in ((2, 16, 16, q.data_ptr(), 0, buf, 640), (3, 0, 16, q.data_ptr(), 0, buf, 640), (3, 16, 65536, q.data_ptr(), 0, buf, 640),
                 (3, 16, 16, None, 0, buf, 640), (3, 16, 16, q.data_ptr(), 0, None, 640), (3, 16, 16, q.data_ptr(), -1, buf, 640),
                 (3, 16, 16, q.data_ptr(), 65536, buf, 640), (3, 16, 16, q.data_ptr(), 0, buf, 622)):
        assert f(*args) == -1, args
    for bad in (0, 256, -3):
        q2 = q.clone()
        q2[1, 63] = bad
        assert f(3, 16, 16, q2.data_ptr(), 0, buf, 640) == -1
        q2 = q.clone()
        q2[2, 0] = bad                                              # the third table is not written: table 1 serves both chroma planes
        assert f(3, 16, 16, q2.data_ptr(), 0, buf, 640) == 623


def test_bound_and_scratch_bytes(golden):
    bound, scratch = L.lib().rgbnm_jpeg_encode_bound, L.lib().rgbnm_jpeg_encode_scratch_bytes
    for bad in ((0, 4, 0, 2, 3, 0), (4, 4097, 2, 2049, 3, 0), (4, 4, 2, 2, 2, 0), (4, 4, 2, 3, 3, 0), (5, 4, 2, 2, 3, 0), (4, 4, 2, 2, 3, -1),
                (4, 4, 2, 2, 3, 65536), (4096, 4096, 2048, 2048, 3, 0)):      # the last: more bits per image than 32-bit positions hold
        assert bound(*bad) == 0, bad
        assert scratch(2, *bad, 4096) == 0, bad
    assert scratch(0, 4, 4, 2, 2, 3, 0, 4096) == 0 and scratch(-1, 4, 4, 2, 2, 3, 0, 4096) == 0 and scratch(2, 4, 4, 2, 2, 3, 0, 0) == 0
    # header + 2 * 208 bytes per block of the padded scan + RSTn + EOI
    assert bound(4, 4, 2, 2, 3, 0) == 623 + 2 * 208 * 24 + 2
    assert bound(3, 3, 2, 2, 3, 0) == bound(4, 4, 2, 2, 3, 0)                # the padding is coded
    assert bound(4, 4, 2, 2, 3, 1) == 629 + 2 * 208 * 24 + 2 * 3 + 2
    assert bound(4, 4, 2, 2, 3, 9) == 629 + 2 * 208 * 24 + 2                  # an interval above the MCU count: one run
    assert bound(3, 5, 0, 0, 1, 2) == 334 + 2 * 208 * 15 + 2 * 7 + 2
    assert bound(64, 64, 32, 32, 3, 0) < 1 << 22
    # scratch grows with n, the grid, the number of runs and (up to the bound) the stride
    s = [scratch(n, 4, 4, 2, 2, 3, 0, 4096) for n in (1, 2, 64)]
    assert s == sorted(s) and len(set(s)) == 3
    assert scratch(2, 4, 4, 2, 2, 3, 1, 4096) > scratch(2, 4, 4, 2, 2, 3, 0, 4096)
    assert scratch(2, 8, 8, 4, 4, 3, 0, 4096) > scratch(2, 4, 4, 2, 2, 3, 0, 4096)
    assert scratch(2, 4, 4, 2, 2, 3, 0, 8192) > scratch(2, 4, 4, 2, 2, 3, 0, 4096)
    assert scratch(2, 4, 4, 2, 2, 3, 0, 1 << 30) == scratch(2, 4, 4, 2, 2, 3, 0, bound(4, 4, 2, 2, 3, 0))
    # the bound covers every fixture file, and so does the Python wrapper's
    g = golden("g26_jpeg_write.npz")
    for name in CASES:
        _, _, _, Y, Cc, data = case(g, name)
        hb, wb = Y.shape[1:3]
        assert len(data) <= bound(hb, wb, (hb + 1) // 2, (wb + 1) // 2, 1 if Cc is None else 3, 0) \
            == dm.jpeg_encode_bound((hb, wb), 1 if Cc is None else 3), name


def test_refusals_are_decided_before_any_device_call():
    """Host memory stands in for every buffer: a refused call touches none of it."""
    f = L.lib().rgbnm_jpeg_encode_batch
    need = L.lib().rgbnm_jpeg_encode_scratch_bytes(2, 4, 4, 2, 2, 3, 0, 1024)
    buf = torch.zeros(1 << 17, dtype=torch.uint8)
    base = (buf.data_ptr() + 63) & ~63
    Y, Cc, q, d, out, nb, st, scr = (base + 8192 * k for k in range(8))

    def call(Y=Y, Cc=Cc, q=q, d=d, n=2, grid=(4, 4, 2, 2), ri=0, out=out, stride=1024, nb=nb, st=st, scr=scr, nbytes=need):
        return f(Y, Cc, q, d, n, *grid, ri, out, stride, nb, st, scr, nbytes, None)

    assert call(Y=None) == -1 and call(q=None) == -1 and call(d=None) == -1 and call(out=None) == -1 and call(nb=None) == -1
    assert call(st=None) == -1 and call(scr=None) == -1 and call(n=0) == -1 and call(stride=0) == -1 and call(stride=1 << 31) == -1
    assert call(Y=Y + 8) == -1 and call(Cc=Cc + 2) == -1 and call(q=q + 1) == -1 and call(d=d + 2) == -1 and call(nb=nb + 2) == -1
    assert call(st=st + 1) == -1 and call(scr=scr + 8) == -1 and call(nbytes=need - 1) == -1 and call(nbytes=0) == -1
    assert call(grid=(0, 4, 0, 2)) == -1 and call(grid=(4, 4, 2, 3)) == -1 and call(grid=(4, 4097, 2, 2049)) == -1
    assert call(ri=-1) == -1 and call(ri=65536) == -1
    assert call(ri=1) == -1 and call(stride=2048) == -1            # more runs / a longer slot need more scratch than `need`
    assert not buf.any()
    Yc = torch.zeros((1, 1, 2, 2, 8, 8), dtype=torch.int16)
    with pytest.raises(L.RgbnmError, match="no CPU fallback"):
        dm.encode_jpeg_batch(Yc, None, torch.ones((1, 8, 8), dtype=torch.int16))
    with pytest.raises(ValueError, match="restart"):
        dm.jpeg_encode_bound((4, 4), 3, "column")


@pytest.fixture(scope="module")
def encode_check(tmp_path_factory):
    """tools/jpeg_encode_check.cpp under the host sanitizers, as a program of its own; skipped where the compiler has no runtime for them."""
    d = tmp_path_factory.mktemp("encode_check")
    exe = str(d / "jpeg_encode_check")
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    r = subprocess.run(["g++"] + flags + [str(probe), "-o", str(d / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(d / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ has no address / undefined-behaviour sanitizer runtime here")
    r = subprocess.run(["g++"] + flags + [os.path.join(ROOT, "tools", "jpeg_encode_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(items):
        """items: [(height, width, quant, Y, C | None, restart)] -> [file bytes, or the status the program printed]"""
        argv, outs = [exe], []
        for k, (h, w, quant, Y, Cc, ri) in enumerate(items):
            src, dst = d / f"in{k}.bin", d / f"out{k}.jpg"
            if dst.exists():
                dst.unlink()
            nc = 1 if Cc is None else 3
            with open(src, "wb") as fh:
                fh.write(np.array([nc, h, w, ri], np.int32).tobytes() + np.ascontiguousarray(quant[:nc], np.int16).tobytes()
                         + np.ascontiguousarray(Y, np.int16).tobytes() + (b"" if Cc is None else np.ascontiguousarray(Cc, np.int16).tobytes()))
            argv += [str(src), str(dst)]
            outs.append(dst)
        r = subprocess.run(argv, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines = r.stdout.strip().splitlines()
        assert len(lines) == len(items)
        return [o.read_bytes() if " ok " in ln else int(ln.rsplit(" ", 1)[1]) for o, ln in zip(outs, lines)]

    return run


def test_shared_emit_code_reproduces_the_reference_files(encode_check, golden):
    g = golden("g26_jpeg_write.npz")
    items = [case(g, name) for name in CASES]
    got = encode_check([it[:5] + (0,) for it in items])
    for name, it, data in zip(CASES, items, got):
        assert data == it[5], name
    stuffed = case(g, "stuffing")[5]
    assert stuffed[scan_start(stuffed):].count(b"\xff\x00") >= 20 and stuffed.endswith(b"\xff\x00\xff\xd9")


def test_shared_emit_code_with_restart_intervals_equals_the_python_writer(encode_check, golden):
    g = golden("g26_jpeg_write.npz")
    items, want = [], []
    for name in ("r24x40", "r17x9", "g24x40", "stuffing", "sparse", "r64x64"):
        h, w, quant, Y, Cc, _ = case(g, name)
        row = -(-w // (8 if Cc is None else 16))
        for ri in (1, 4, row):
            items.append((h, w, quant, Y, Cc, ri))
            ref = writer_file(h, w, quant, Y, Cc, ri)
            want.append(ref[scan_start(ref) - (10 if Cc is None else 14):])
    got = encode_check(items)
    for it, data, ref in zip(items, got, want):
        assert isinstance(data, bytes) and data[scan_start(data) - (10 if it[4] is None else 14):] == ref, (it[0], it[1], it[5])


def test_shared_emit_code_refuses_what_baseline_coding_cannot_express(encode_check, golden):
    g = golden("g26_jpeg_write.npz")
    h, w, quant, Y, Cc, data = case(g, "r24x40")
    items = []
    for plane, at, v in (("Y", (0, 2, 4, 3, 3), 1024), ("Y", (0, 0, 0, 7, 7), -1024), ("C", (1, 0, 2, 0, 1), -32768), ("Y", (0, 1, 1, 0, 0), 2500),
                         ("C", (0, 1, 0, 0, 0), -2400)):
        Y2, C2 = Y.copy(), Cc.copy()
        (Y2 if plane == "Y" else C2)[at] = v
        if at[3:] == (0, 0):                                        # a DC step beyond 2047 either side of it
            (Y2 if plane == "Y" else C2)[at[:3] + (0, 0)] = v
        items.append((h, w, quant, Y2, C2, 0))
    Y2 = Y.copy()
    Y2[0, 0, 0, 5, 5] = 1023
    Y2[0, 2, 4, 0, 0] = Y2[0, 2, 3, 0, 0] + 2047                    # the limits themselves are coded
    items.append((h, w, quant, Y2, Cc, 0))
    q2 = quant.copy()
    q2[1, 3, 3] = 256
    items.append((h, w, q2, Y, Cc, 0))
    items.append((h, w, quant, Y, Cc, 0))
    got = encode_check(items)
    assert got[:5] == [-25] * 5 and isinstance(got[5], bytes) and got[6] == -25 and got[7] == data
    assert dm.read_coefficients_bytes(got[5])[2].numpy().tobytes() == Y2.tobytes()
